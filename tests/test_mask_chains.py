"""The three binary-mask chains of a predict -- bad-pixel mask, reliable mask, contact / background masks -- as one launch each
(csrc/k_maskchain.hip, test hook "fused_masks", bits 1 / 2 / 4, default 7) against the separate kernels they replace and against the CPU
references of tests/mask_chain_cases.py, exactly: masks, counts, thresholds (as bits) and status.  The chains are launched directly through
vistaf_ftp_test_bad_chain / _reliable_chain / _contact_chain (csrc/test_hooks_masks.h) on the hard masks of tests/mask_cases.py; the dispatch rule is checked on the
CPU; whole sessions are compared with the tier on and off.  Each test asserts the tier taken and, from the reference, that a case is what it
is there for."""
import ctypes
import os

import numpy as np
import pytest

import mask_cases as M
import mask_chain_cases as C

BAD, REL, CON = 1, 2, 4
E_INVALID = -1
MIN_FRAC, MAX_FRAC = 0.005, 0.35


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _diff(got, want):
    bad = np.argwhere(got != want)
    return "%d pixels differ, first at %s" % (len(bad), tuple(bad[0]) if len(bad) else None)


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


# =======================================================================================================================================
# 1. each chain directly, fused and separate, against the CPU reference

def gpu_bad(pkg, img, grad, valid, hi, g, ksize, iters, fused):
    import torch
    n, h, w = img.shape
    bad1 = torch.full((n, h, w), 7, dtype=torch.uint8, device="cuda")
    cnt = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    t = [_dev(img), _dev(grad), _dev(valid), _dev(np.asarray(hi, np.float32)), _dev(np.asarray(g, np.float32))]
    tier = pkg._lib.load().vistaf_ftp_test_bad_chain(*[_ptr(x) for x in t], ksize, iters, _ptr(bad1), _ptr(cnt), n, h, w, fused, None)
    assert tier >= 0, pkg._lib.load().vistaf_ftp_last_error()
    return bad1.cpu().numpy(), cnt.cpu().numpy(), tier


def gpu_reliable(pkg, q, roi, thr, ksize, iters, margin, status, fused):
    import torch
    n, h, w = q.shape
    rel0 = torch.full((n, h, w), 7, dtype=torch.uint8, device="cuda")
    rel = torch.full((n, h, w), 7, dtype=torch.uint8, device="cuda")
    cnt = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    st = _dev(np.asarray(status, np.int32))
    t = [_dev(q), _dev(roi), _dev(np.asarray(thr, np.float32))]
    tier = pkg._lib.load().vistaf_ftp_test_reliable_chain(*[_ptr(x) for x in t], ksize, iters, margin, _ptr(rel0), _ptr(rel), _ptr(cnt), _ptr(st), n, h,
                                                          w, fused, None)
    assert tier >= 0, pkg._lib.load().vistaf_ftp_last_error()
    return rel0.cpu().numpy(), rel.cpu().numpy(), cnt.cpu().numpy(), st.cpu().numpy(), tier


def gpu_contact(pkg, res, rel, t3, rc, ksize, iters, fused, min_frac=MIN_FRAC, max_frac=MAX_FRAC):
    import torch
    n, h, w = res.shape
    cd = torch.full((n, h, w), 7, dtype=torch.uint8, device="cuda")
    bg = torch.full((n, h, w), 7, dtype=torch.uint8, device="cuda")
    used = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    bgc = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    t = [_dev(res), _dev(rel), _dev(np.asarray(t3, np.float32)), _dev(np.asarray(rc, np.int32))]
    tier = pkg._lib.load().vistaf_ftp_test_contact_chain(*[_ptr(x) for x in t], min_frac, max_frac, ksize, iters, _ptr(used), _ptr(cd), _ptr(bg),
                                                         _ptr(bgc), n, h, w, fused, None)
    assert tier >= 0, pkg._lib.load().vistaf_ftp_last_error()
    return used.cpu().numpy(), cd.cpu().numpy(), bg.cpu().numpy(), bgc.cpu().numpy(), tier


def check_bad(pkg, masks_a, masks_b, valid, ksize, iters, seed, nan_thr=False):
    rng = np.random.default_rng(seed)
    n = len(masks_a)
    hi = (rng.random(n) * 100 + 50).astype(np.float32)
    g = (rng.random(n) * 10 + 5).astype(np.float32)
    img = np.stack([C.field_from_mask(m, t, rng) for m, t in zip(masks_a, hi)])
    grad = np.stack([C.field_from_mask(m, t, rng) for m, t in zip(masks_b, g)])
    if nan_thr:
        hi[0] = np.nan
    want = [C.ref_bad(img[b], grad[b], valid, hi[b], g[b], ksize, iters) for b in range(n)]
    got = {f: gpu_bad(pkg, img, grad, valid, hi, g, ksize, iters, f) for f in (1, 0)}
    assert got[1][2] == 1 and got[0][2] == 0, (got[1][2], got[0][2])
    for f in (1, 0):
        for b in range(n):
            assert np.array_equal(got[f][0][b], want[b][0]), (f, b, _diff(got[f][0][b], want[b][0]))
            assert int(got[f][1][b]) == want[b][1], (f, b)
    return want


def check_reliable(pkg, masks, roi, ksize, iters, margin, seed, status=None, thr_nan=None, want_tier=1, sprinkle=True):
    rng = np.random.default_rng(seed)
    n = len(masks)
    thr = (rng.random(n) * 4 + 1).astype(np.float32)
    q = np.stack([C.field_from_mask(m, t, rng, sprinkle) for m, t in zip(masks, thr)])
    if thr_nan is not None:
        thr[thr_nan] = np.nan
    status = np.zeros(n, np.int32) if status is None else np.asarray(status, np.int32)
    want = [C.ref_reliable(q[b], roi, thr[b], ksize, iters, margin, status[b]) for b in range(n)]
    got = {f: gpu_reliable(pkg, q, roi, thr, ksize, iters, margin, status, f) for f in (1, 0)}
    assert got[1][4] == want_tier and got[0][4] == 0, (got[1][4], got[0][4])
    for f in (1, 0):
        for b in range(n):
            assert np.array_equal(got[f][0][b], want[b][0]), ("rel0", f, b, _diff(got[f][0][b], want[b][0]))
            assert np.array_equal(got[f][1][b], want[b][1]), ("reliable", f, b, _diff(got[f][1][b], want[b][1]))
            assert int(got[f][2][b]) == want[b][2] and int(got[f][3][b]) == want[b][3], (f, b, got[f][2], got[f][3], want[b][2:4])
    return want


def check_contact(pkg, res, rel, t3, rc, ksize, iters, want_tier=1, **frac):
    n = len(res)
    kw = dict(min_frac=frac.get("min_frac", MIN_FRAC), max_frac=frac.get("max_frac", MAX_FRAC))
    want = [C.ref_contact(res[b], rel[b], t3[b], rc[b], kw["min_frac"], kw["max_frac"], ksize, iters) for b in range(n)]
    got = {f: gpu_contact(pkg, res, rel, t3, rc, ksize, iters, f, **kw) for f in (1, 0)}
    assert got[1][4] == want_tier and got[0][4] == 0, (got[1][4], got[0][4])
    for f in (1, 0):
        for b in range(n):
            assert _bits(got[f][0][b]) == _bits(want[b][0]), ("thr_used", f, b, got[f][0][b], want[b][0])
            assert np.array_equal(got[f][1][b], want[b][1]), ("contact_d", f, b, _diff(got[f][1][b], want[b][1]))
            assert np.array_equal(got[f][2][b], want[b][2]), ("background", f, b, _diff(got[f][2][b], want[b][2]))
            assert int(got[f][3][b]) == want[b][3], ("bg_count", f, b)
    return want


def residuals(masks, rng):
    """float32 residual planes with NaN and infinities sprinkled, and the reliable planes (0 / 1) they go with"""
    rel = np.stack(masks).astype(np.uint8)
    res = rng.standard_normal(rel.shape).astype(np.float32)
    r = rng.random(rel.shape)
    res[r < 0.01] = np.nan
    res[(r >= 0.01) & (r < 0.015)] = np.inf
    res[(r >= 0.015) & (r < 0.02)] = -np.inf
    return res, rel


def pct3(res, rel, qs=(90.0, 95.0, 98.0)):
    """the three thresholds a session would hand over: order statistics of |res| over reliable & finite, so pixels sit exactly on them"""
    out = np.zeros((len(res), 3), np.float32)
    for b in range(len(res)):
        v = np.abs(res[b])[(rel[b] != 0) & np.isfinite(res[b])]
        if v.size:
            out[b] = [np.sort(v)[min(v.size - 1, int(v.size * q / 100.0))] for q in qs]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", C.SMALL_SHAPES, ids=["%dx%d" % s for s in C.SMALL_SHAPES])
def test_bad_chain_equals_reference(pkg, h, w):
    cat = C.catalogue(h, w)
    names = list(cat)
    valid = C.disc(h, w)
    for i, grp in enumerate(C.batches(names)):
        k, it, _ = C.COMBOS[i % len(C.COMBOS)]
        other = [names[(names.index(x) + 5) % len(names)] for x in grp]
        check_bad(pkg, [cat[x] for x in grp], [cat[x] for x in other], valid, k, it, 11 * i + h, nan_thr=(i == 1))
    # no dilation at all (kernel size 1), and all ones inside an all-ones valid plane: the full mask
    check_bad(pkg, [cat["ones"], cat["zeros"]], [cat["zeros"], cat["zeros"]], np.ones((h, w), np.uint8), 1, 1, 5)


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", C.SMALL_SHAPES, ids=["%dx%d" % s for s in C.SMALL_SHAPES])
def test_reliable_chain_equals_reference(pkg, h, w):
    cat = C.catalogue(h, w)
    roi = C.disc(h, w)
    ones = np.ones((h, w), np.uint8)
    seen_empty_after_erosion = False
    for i, grp in enumerate(C.batches(cat)):
        for j in (0, 1):        # every batch with two of the element / iteration / margin combinations, under the disc and under no roi
            k, it, margin = C.COMBOS[(2 * i + j) % len(C.COMBOS)]
            want = check_reliable(pkg, [cat[x] for x in grp], roi if j else ones, k, it, margin, 13 * i + j + w, status=[0, 5, 0][:len(grp)],
                                  thr_nan=(2 if (i == 2 and j == 0) else None))
            for b, wnt in enumerate(want):
                if wnt[4]["before_erosion"] > 0 and wnt[2] == 0:
                    seen_empty_after_erosion = True
                    assert wnt[3] == (1 if b != 1 else 5)       # status 1, and a status already set stays
    assert seen_empty_after_erosion         # a largest component that the erosion removes entirely
    # empty and full
    want = check_reliable(pkg, [cat["zeros"], cat["ones"]], ones, 3, 1, 1, 3)
    assert want[0][2] == 0 and want[0][3] == 1 and want[1][2] > 0 and want[1][0].sum() > 0.9 * h * w       # (full but for the sprinkled non-finite pixels)
    # two components of equal area: the smaller root wins
    if "two_equal_squares" in cat:
        want = check_reliable(pkg, [cat["two_equal_squares"], cat["tie_equal_areas"]], ones, 3, 1, 0, 4, sprinkle=False)
        f = want[0][4]
        assert len(f["areas"]) == 2 and f["areas"][0] == f["areas"][1] and f["roots"][0] < f["roots"][1]
        assert want[0][1].ravel()[f["roots"][0]] == 1 and want[0][1].ravel()[f["roots"][1]] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", C.SMALL_SHAPES, ids=["%dx%d" % s for s in C.SMALL_SHAPES])
def test_contact_chain_equals_reference(pkg, h, w):
    cat = C.catalogue(h, w)
    rng = np.random.default_rng(h * 1000 + w)
    for i, grp in enumerate(C.batches(cat)):
        k, it, _ = C.COMBOS[i % len(C.COMBOS)]
        res, rel = residuals([cat[x] for x in grp], rng)
        check_contact(pkg, res, rel, pct3(res, rel), rel.reshape(len(rel), -1).sum(1), k, it)
    # every branch of the threshold choice and of the background, on a disc
    d = C.disc(h, w)
    res, rel = residuals([d, d, d], rng)
    rc = rel.reshape(3, -1).sum(1)
    t = pct3(res, rel)
    t_in, t_min, t_max, t_nan = t.copy(), t.copy(), t.copy(), t.copy()
    t_min[:, 0] = 1e30
    t_max[:, 0] = 0.0
    t_nan[:, 0] = np.nan
    t_nan[2, 1] = np.inf            # neither the first nor the second is finite: the mask is empty
    for t3, branch in ((t_in, "in"), (t_min, "min"), (t_max, "max")):
        want = check_contact(pkg, res, rel, t3, rc, 3, 1)
        assert all(branch in wnt[4] and "bg_fallback" not in wnt[4] for wnt in want), [wnt[4] for wnt in want]
    want = check_contact(pkg, res, rel, t_nan, rc, 3, 1)
    assert all("nonfinite" in wnt[4] for wnt in want) and not want[2][1].any()
    # the 15 % background fallback: most of the mask is contact and the dilation takes the rest
    t_lo = pct3(res, rel, (30.0, 95.0, 98.0))
    want = check_contact(pkg, res, rel, t_lo, rc, 7, 2, max_frac=1.0)
    assert all("bg_fallback" in wnt[4] and "in" in wnt[4] for wnt in want), [wnt[4] for wnt in want]
    assert all(np.array_equal(wnt[2], d) and wnt[3] < int(0.15 * rc[0]) for wnt in want)
    # rel_count 0: an empty reliable plane
    res0, rel0 = residuals([np.zeros((h, w), np.uint8)] * 2, rng)
    want = check_contact(pkg, res0, rel0, pct3(res, rel)[:2], np.zeros(2, np.int32), 5, 1)
    assert not want[0][1].any() and not want[0][2].any() and want[0][3] == 0
    # no dilation: contact_d is the contact mask
    check_contact(pkg, res, rel, t_in, rc, 5, 0)


@pytest.mark.gpu
def test_reliable_chain_single_column(pkg):
    """w = 1: every pixel is a row of the bit plane (the accessor's row arithmetic has its own rule there) and components run down the column"""
    h, w = 70, 1
    cat = C.catalogue(h, w)
    ones = np.ones((h, w), np.uint8)
    want = check_reliable(pkg, [cat["random_0.41"], cat["ones"], cat["random_0.6"]], ones, 3, 1, 0, 70, sprinkle=False)
    assert 0 < want[0][2] < int(cat["random_0.41"].sum()) + h and want[1][2] == h
    check_reliable(pkg, [cat["random_0.95"], cat["zeros"]], ones, 5, 1, 1, 71)


@pytest.mark.gpu
def test_chains_224(pkg):
    """224 x 224 once per chain: four words per row, the last holds 32 columns; the reliable chain's forest and planes take 122 KB of LDS"""
    h = w = 224
    big = C.big_masks(h, w, 224)
    masks = [big[k] for k in ("random_0.41", "checker", "comb_joined_last_row")]
    check_bad(pkg, masks, masks[::-1], C.disc(h, w), 5, 2, 1)
    check_reliable(pkg, masks, C.disc(h, w, 4), 7, 1, 6, 2)
    rng = np.random.default_rng(3)
    res, rel = residuals([C.disc(h, w), masks[0], masks[2]], rng)
    check_contact(pkg, res, rel, pct3(res, rel), rel.reshape(3, -1).sum(1), 15, 2)


# =======================================================================================================================================
# 2. dispatch, and the entry points' signatures

def test_mask_chain_prototypes_match_their_signature_table(pkg):
    """csrc/test_hooks_masks.h against _lib.MASK_CHAIN_SIGNATURES: same names, same number of parameters, pointer against pointer, int
    against c_int, double against c_double; and the library exports every one"""
    import re
    text = open(os.path.join(os.path.dirname(pkg.__file__), "csrc", "test_hooks_masks.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = "\n".join(ln for ln in text.split("\n") if not ln.lstrip().startswith("#"))
    protos = {name: (ret.strip(), [" ".join(q.split()) for q in params.split(",")])
              for ret, name, params in re.findall(r"([A-Za-z_][\w \t\*]*?)\b(vistaf_\w+)\s*\(([^()]*)\)\s*;", text)}
    table = pkg._lib.MASK_CHAIN_SIGNATURES
    assert sorted(protos) == sorted(table) and len(table) == 4
    assert not set(table) & {n for grp in pkg._lib.SIGNATURES.values() for n in grp}
    lib = pkg._lib.load()
    for name, (ret, params) in protos.items():
        restype, argtypes = table[name]
        assert ret == "int" and restype is ctypes.c_int and len(params) == len(argtypes), name
        for q, a in zip(params, argtypes):
            want = ctypes.c_void_p if "*" in q else ctypes.c_double if q.split()[0] == "double" else ctypes.c_int
            assert q.split()[0] in ("const", "int", "double", "uint8_t", "int32_t", "float", "void") and a is want, (name, q, a)
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name

def test_mask_chain_fits_limits(pkg):
    fits = pkg._lib.load().vistaf_ftp_test_mask_chain_fits
    for chain in (BAD, REL, CON):
        assert fits(chain, 224, 224, 7, 2, 6) == 1, chain
        assert fits(chain, 64, 64, 15, 4, 1) == 1 and fits(chain, 64, 64, 15, 5, 1) == 0, chain      # at most four operations
        assert fits(chain, 9, 40, 3, 0, 0) == 1, chain
    # the forest: uint16 labels (256 x 256 has one pixel too many), and forest + three planes within 150 KB (255 x 257 = 65535 pixels
    # fits the labels but needs 131088 + 3 * 10200 bytes)
    assert fits(REL, 256, 256, 7, 2, 6) == 0 and fits(REL, 255, 257, 7, 2, 6) == 0
    assert fits(REL, 240, 240, 7, 2, 6) == 1            # 115216 + 3 * 7680 = 138256 bytes
    assert fits(BAD, 256, 256, 5, 2, 0) == 1 and fits(CON, 256, 256, 15, 2, 0) == 1
    assert fits(BAD, 1182, 1182, 5, 2, 0) == 0 and fits(CON, 1182, 1182, 15, 2, 0) == 0 and fits(REL, 1182, 1182, 7, 2, 6) == 0
    # an element the word-shift step refuses: the even ellipses a session may be given for the contact dilation are not symmetric
    assert fits(CON, 64, 64, 4, 1, 0) == 0 and fits(CON, 64, 64, 4, 0, 0) == 1 and fits(CON, 64, 64, 5, 1, 0) == 1
    # a margin with no chamfer ball (more than 33 rows)
    assert fits(REL, 64, 64, 7, 2, 16) == 1 and fits(REL, 64, 64, 7, 2, 40) == 0
    assert fits(3, 64, 64, 7, 2, 0) == 0 and fits(0, 64, 64, 7, 2, 0) == 0
    assert fits(REL, 64, 64, 34, 2, 0) == E_INVALID


@pytest.mark.gpu
def test_refused_tier_runs_the_separate_kernels(pkg):
    h, w = 64, 64
    cat = C.catalogue(h, w)
    rng = np.random.default_rng(9)
    masks = [cat["random_0.41"], cat["spiral"]]
    res, rel = residuals(masks, rng)
    rc = rel.reshape(2, -1).sum(1)
    check_contact(pkg, res, rel, pct3(res, rel), rc, 4, 1, want_tier=0)           # even element
    check_contact(pkg, res, rel, pct3(res, rel), rc, 3, 5, want_tier=0)           # five dilations
    check_reliable(pkg, masks, C.disc(h, w), 3, 3, 1, 10, want_tier=0)            # six operations
    lib = pkg._lib.load()
    assert lib.vistaf_ftp_test_contact_chain(None, None, None, None, 0.0, 1.0, 3, 1, None, None, None, None, 2, h, w, 1, None) == E_INVALID
    assert lib.vistaf_ftp_test_bad_chain(None, None, None, None, None, 3, 1, None, None, 2, h, w, 1, None) == E_INVALID
    assert lib.vistaf_ftp_test_reliable_chain(None, None, None, 3, 1, 1, None, None, None, None, 2, h, w, 1, None) == E_INVALID


# =======================================================================================================================================
# 3. sessions: fused_masks = 7 against 0

PLANES = ("bad1", "rel0", "reliable", "contact_d", "background", "kept")


def _run(sensor, frames, fused, refs=None):
    import torch
    sensor._test_set("fused_masks", fused)
    out = sensor.predict_batch(frames) if refs is None else sensor.predict_pairs(refs, frames)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for p in PLANES:
        got[p] = sensor.intermediate(p, len(frames), torch.uint8).cpu().numpy()
    got["thr_used"] = sensor.intermediate("thr_used", len(frames), torch.float32).cpu().numpy().view(np.uint32)
    return got


def _same(a, b):
    assert set(a) == set(b) and {"height_map_mm", "output_reliable", "scalars", "status"} <= set(a)
    for key in b:
        assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape, key
        assert np.array_equal(a[key], b[key], equal_nan=a[key].dtype.kind == "f"), key


SESSIONS = [
    ("64x64_b3", 64, 64, {}, [("multi", 901), ("single", 902), ("flat", 0)], 0),
    ("64x64_b3_empty_reliable", 64, 64, dict(reliable_edge_margin_px=40), [("multi", 901), ("single", 902), ("flat", 0)], 1),
    ("96x80_b2", 96, 80, {}, [("multi", 901), ("bump", 904)], 0),
    ("224x224", 224, 224, {}, [("multi", 901)], 0),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", SESSIONS, ids=[c[0] for c in SESSIONS])
def test_sessions_fused_masks_equal_separate_kernels(pkg, case):
    import test_backend_fused as F
    _, h, w, over, scenes, want_status = case
    g = os.path.join(os.path.dirname(__file__), "golden")
    model, neg = pkg.load_calibration(os.path.join(g, "calibration_phase_to_height.json"))
    fm = pkg.load_force_calibration(os.path.join(g, "calibration_height_to_force.json"))["best_model"]
    circle = (w // 2, h // 2, min(h, w) // 2 - 1)
    cfg = pkg.FtpConfig.scaled(min(h, w))
    for k, v in over.items():
        setattr(cfg, k, v)
    ref = F._scene(h, w, "ref", 900)
    frames = np.stack([F._scene(h, w, kind, seed) for kind, seed in scenes])
    sensor = pkg.FtpSensor(ref, circle, cfg, model, neg, fm, max_batch=len(frames))
    a = _run(sensor, frames, 7)
    b = _run(sensor, frames, 0)
    c = _run(sensor, frames, 7)         # and again on the planes the separate kernels left behind
    assert (b["status"] == want_status).all(), b["status"]
    if want_status:
        assert not b["reliable"].any()      # the frames with an empty reliable mask
    else:
        assert b["reliable"].any() and b["contact_d"].any() and b["background"].any()
    _same(a, b)
    _same(c, b)
    for bit in (BAD, REL, CON):         # each chain alone
        _same(_run(sensor, frames, bit), b)
    sensor.close()
    if h == 64 and not over:            # one pair-mode batch
        refs = np.stack([F._scene(h, w, "ref", 900 + i) for i in range(len(frames))])
        ps = pkg.FtpSensor(None, circle, cfg, model, neg, fm, max_batch=len(frames), frame_shape=(h, w))
        _same(_run(ps, frames, 7, refs), _run(ps, frames, 0, refs))
        ps.close()
