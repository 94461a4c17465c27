"""The mask topology kernels launched directly (csrc/test_hooks.h: vistaf_ftp_test_cc_label / _cc_largest / _chamfer_dispatch / _blob_filter)
on the hard masks of tests/mask_cases.py, every tier of each launcher against an independent CPU reference, exactly: connected components
against scipy.ndimage, the largest component and the blob filter against plain NumPy, the closed-form chamfer tiers against the oracle's
two-pass transform within the band they promise and against their own formula everywhere.  Each test asserts the tier the launcher took, and
asserts from the reference that a mask is what its name says."""
import collections
import ctypes

import numpy as np
import pytest

import mask_cases as M
from oracle import cvlite

B = 3
E_INVALID = -1


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _groups(names, n=B):
    """the names in groups of n, the last one filled up from the front"""
    names = list(names)
    out = [names[i:i + n] for i in range(0, len(names), n)]
    out[-1] = (out[-1] + names)[:n]
    return out


def _first_diff(got, want):
    bad = np.argwhere(got != want)
    y, x = bad[0]
    return "%d pixels differ, first at (%d, %d): got %r, want %r" % (len(bad), y, x, got[y, x], want[y, x])


_CAT = {}


def catalogue(h, w):
    """name -> (mask, reference labels) of the h x w catalogue: computed once, shared by the tests, never written to"""
    if (h, w) not in _CAT:
        cat = {k: (m, M.ref_labels(m)) for k, m in M.hard_masks(h, w, 1000 * h + w).items()}
        for m, lab in cat.values():
            m.setflags(write=False)
            lab.setflags(write=False)
        _CAT[(h, w)] = cat
    return _CAT[(h, w)]


def assert_claims(cat):
    """the masks are what their names say, by the reference"""
    for name, (m, lab) in cat.items():
        assert m.dtype == np.uint8 and np.array_equal(lab >= 0, m != 0), name
        roots, areas = M.component_areas(lab)
        if name in M.COMPONENTS:
            assert len(roots) == M.COMPONENTS[name], (name, len(roots))
        if name == "tie_equal_areas":
            assert areas[0] == areas[1] and roots[0] < roots[1], (roots, areas)
            assert np.flatnonzero(lab == roots[0])[1] > np.flatnonzero(lab == roots[1])[-1]      # all but its root come after the other blob
        if name == "larger_later":
            assert areas[1] > areas[0] and roots[0] < roots[1], (roots, areas)
        if name == "checker" and min(m.shape) >= 2:       # diagonal contacts only: 4-connectivity sees every pixel alone
            assert int(M.ndimage.label(m != 0)[1]) == int((m != 0).sum())
    if "random_0.41" in cat:
        assert set(np.unique(cat["random_0.41"][0])) == {0, 1, 2, 255} or cat["random_0.41"][0].size < 64


# =======================================================================================================================================
# labelling

def gpu_labels(pkg, masks, variant):
    """masks [n, h, w] uint8 -> (labels [n, h, w] int32, tier)"""
    import torch
    n, h, w = masks.shape
    dm = _dev(masks)
    lab = torch.full((n, h, w), -7, dtype=torch.int32, device="cuda")
    tier = pkg._lib.load().vistaf_ftp_test_cc_label(_ptr(dm), _ptr(lab), n, h, w, variant, None)
    assert tier >= 0, pkg._lib.load().vistaf_ftp_last_error()
    return lab.cpu().numpy(), tier


def check_labels(pkg, h, w, variant, want_tier):
    cat = catalogue(h, w)
    assert_claims(cat)
    for grp in _groups(cat):
        got, tier = gpu_labels(pkg, np.stack([cat[k][0] for k in grp]), variant)
        assert tier == want_tier, (tier, want_tier)
        for j, k in enumerate(grp):
            assert np.array_equal(got[j], cat[k][1]), (k, _first_diff(got[j], cat[k][1]))


# tier -> shapes.  0: the LDS forest with the mask staged behind it, up to 114 x 479 = 54606 pixels (forest + mask + 16 bytes <= 160 KB);
# 1: the LDS forest alone, from 203 x 269 = 54607 to 255 x 257 = 65535 pixels (uint16 labels); 2: the global union-find.  With an odd
# pixel count frames 1 and 2 of the batch start at unaligned addresses.
LABEL_SHAPES = {
    0: [(1, 1), (5, 7), (7, 2), (2, 7), (1, 300), (300, 1), (33, 65), (64, 64), (151, 203), (224, 224), (114, 479)],
    1: [(203, 269), (240, 240), (255, 257), (1, 65535), (65535, 1)],
    2: [(256, 256), (130, 505), (1, 70000), (70000, 1)],
}
LABEL_CASES = [(t, h, w) for t, shapes in LABEL_SHAPES.items() for h, w in shapes]


@pytest.mark.gpu
@pytest.mark.parametrize("tier,h,w", LABEL_CASES, ids=["tier%d_%dx%d" % c for c in LABEL_CASES])
def test_cc_label_dispatch_equals_reference(pkg, tier, h, w):
    check_labels(pkg, h, w, 0, tier)


# the global kernels at sizes a session labels in LDS: rows that wrap inside a 64-pixel segment of k_cc_init's ballot (w = 7, 63, 65),
# segments that are whole rows (64), rows of several segments (200, 203)
GLOBAL_SHAPES = [(5, 7), (7, 2), (2, 7), (3, 200), (33, 65), (70, 63), (64, 64), (151, 203)]


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", GLOBAL_SHAPES, ids=["%dx%d" % s for s in GLOBAL_SHAPES])
def test_cc_label_global_kernels_forced_equal_reference(pkg, h, w):
    check_labels(pkg, h, w, 1, 2)


# =======================================================================================================================================
# largest component

def gpu_largest(pkg, labels, and_static, variant):
    import torch
    n, h, w = labels.shape
    dl = _dev(labels)
    da = _dev(and_static) if and_static is not None else None
    out = torch.full((n, h, w), 77, dtype=torch.uint8, device="cuda")
    tier = pkg._lib.load().vistaf_ftp_test_cc_largest(_ptr(dl), _ptr(da), _ptr(out), n, h * w, variant, None)
    assert tier >= 0, pkg._lib.load().vistaf_ftp_last_error()
    return out.cpu().numpy(), tier


LARGEST_SUBSET = ["zeros", "tie_equal_areas", "larger_later", "interlocked_combs", "random_0.41", "checker", "random_0.6", "two_spirals", "ones"]
# (h, w, frames per launch, [(variant, tier it must report)]): both tiers forced on small frames, the dispatch where it takes the batch kernels
LARGEST_CASES = [(5, 7, 3, [(1, 1), (2, 2), (0, 1)]), (33, 65, 3, [(1, 1), (2, 2)]), (224, 224, 3, [(1, 1), (2, 2)]), (512, 512, 2, [(0, 2)])]


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,nb,variants", LARGEST_CASES, ids=["%dx%d" % c[:2] for c in LARGEST_CASES])
def test_cc_largest_equals_reference(pkg, h, w, nb, variants):
    cat = catalogue(h, w)
    if h * w > 65 * 33:                     # large frames: the masks this kernel can tell apart
        cat = {k: cat[k] for k in (LARGEST_SUBSET[:6] if nb == 2 else LARGEST_SUBSET)}
    names = list(cat)
    assert_claims(cat)
    static = M.and_static_plane(h, w)
    win = M.ref_largest(cat["larger_later"][1])
    assert (win & static).any() and (win & (1 - static)).any()              # the plane cuts the winner, and only partly
    want = {k: (M.ref_largest(cat[k][1]), M.ref_largest(cat[k][1], static)) for k in names}
    assert not want["zeros"][0].any() and not want["zeros"][1].any()
    groups = _groups(names, nb)
    assert "zeros" in groups[0] and len(set(groups[0])) > 1                 # an empty frame next to non-empty ones
    for grp in groups:
        masks = np.stack([cat[k][0] for k in grp])
        own, _ = gpu_labels(pkg, masks, 0)
        for source, labels in (("reference labels", np.stack([cat[k][1] for k in grp])), ("the GPU's own labels", own)):
            for variant, want_tier in variants:
                for col, plane in ((0, None), (1, static)):
                    got, tier = gpu_largest(pkg, labels, plane, variant)
                    assert tier == want_tier, (variant, tier)
                    for j, k in enumerate(grp):
                        assert np.array_equal(got[j], want[k][col]), (k, source, variant, col, _first_diff(got[j], want[k][col]))


# =======================================================================================================================================
# chamfer dispatch

# tier -> (h, w, cap_px).  0 k_chamfer_lds: a band of at most 16 rows, w <= 512, h * w <= 76800; (5, 7, 11): the band clamped to h; 64, 128 and
# 512 columns are whole ballot words, 65, 129 and 203 ragged ones, 150 x 512 the largest plane with all eight words.  2 k_rowdist +
# k_chamfer_cols: beyond 512 columns, 515 and 1301 with a ragged last chunk, 1280 whole chunks.  1 k_chamfer2: one case, to pin the dispatch.
CHAMFER_SHAPES = {
    0: [(5, 7, 3), (5, 7, 11), (7, 2, 3), (33, 65, 3), (17, 64, 11), (40, 128, 5), (40, 129, 5), (151, 203, 7), (224, 224, 5), (150, 512, 11)],
    2: [(40, 515, 3), (70, 515, 48), (20, 1280, 11), (9, 1301, 5)],
    1: [(64, 224, 48)],
}
CHAMFER_CASES = [(t, h, w, c) for t, shapes in CHAMFER_SHAPES.items() for h, w, c in shapes]
_CHREF = {}


def chamfer_reference(h, w):
    """name -> (mask, distance to the zero pixels, distance to the non-zero pixels) by the oracle's two-pass transform"""
    if (h, w) not in _CHREF:
        import test_backend_fused as F
        ms = {"basic_" + k: m for k, m in F._masks(h, w, 1000 * h + w).items()}
        ms.update(M.chamfer_masks(h, w))
        _CHREF[(h, w)] = {k: (m, cvlite.dist_l2_3x3(m), cvlite.dist_l2_3x3((m == 0).astype(np.uint8))) for k, m in ms.items()}
    return _CHREF[(h, w)]


def gpu_chamfer(pkg, masks, pair, invert, cap_px):
    import torch
    n, h, w = masks.shape
    dm = _dev(masks)
    da = torch.full((n, h, w), -1.0, dtype=torch.float32, device="cuda")
    db = torch.full((n, h, w), -1.0, dtype=torch.float32, device="cuda") if pair else None
    tier = pkg._lib.load().vistaf_ftp_test_chamfer_dispatch(_ptr(dm), pair, invert, _ptr(da), _ptr(db), n, h, w, cap_px, None)
    assert tier >= 0, pkg._lib.load().vistaf_ftp_last_error()
    return da.cpu().numpy(), (db.cpu().numpy() if pair else None), tier


@pytest.mark.gpu
@pytest.mark.parametrize("tier,h,w,cap_px", CHAMFER_CASES, ids=["tier%d_%dx%d_cap%d" % c for c in CHAMFER_CASES])
def test_chamfer_dispatch_keeps_its_contract(pkg, tier, h, w, cap_px):
    ref = chamfer_reference(h, w)
    count = collections.Counter()

    def check(got, name, col, how):
        m, want = ref[name][0], ref[name][col]
        if tier == 1:                   # the two-pass kernel is the transform itself
            assert np.array_equal(got, want), (name, how, _first_diff(got, want))
            count["in"] += int((want <= cap_px + 2).sum())
            count["out"] += int((want > cap_px + 2).sum())
            return
        msg, n_in, n_out = M.chamfer_contract(got, want, cap_px)
        assert msg is None, (name, how, msg)
        count["in"] += n_in
        count["out"] += n_out
        # and everywhere, beyond the band too, the bits of the closed form the kernels implement
        own = M.closed_form_chamfer((m == 0) if col == 1 else (m != 0), cap_px)
        assert np.array_equal(got.view(np.uint32), own.view(np.uint32)), (name, how, "closed form", _first_diff(got, own))

    for grp in _groups(ref):
        masks = np.stack([ref[k][0] for k in grp])
        for invert in (0, 1):
            da, _, t = gpu_chamfer(pkg, masks, 0, invert, cap_px)
            assert t == tier, (t, tier)
            for j, k in enumerate(grp):
                check(da[j], k, 1 + invert, "invert=%d" % invert)
        da, db, t = gpu_chamfer(pkg, masks, 1, 0, cap_px)
        assert t == tier, (t, tier)
        for j, k in enumerate(grp):
            check(da[j], k, 1, "pair, to the zero pixels")
            check(db[j], k, 2, "pair, to the non-zero pixels")
    assert count["in"] > 0 and count["out"] > 0, count
    # a lone zero leaves pixels beyond the band in every shape but the two whose band covers the frame (7 x 2: no pixel is further than
    # 3.28 from the middle of the first column)
    lone = ref["lone_zero_first_col"][1]
    assert (lone > cap_px + 2).any() or (h, w, cap_px) in ((5, 7, 11), (7, 2, 3))


# =======================================================================================================================================
# blob filter

def _blob_frame(mask, lab, thr, rng):
    """depth plane of one frame: random positive float32, the largest component's peak exactly thr, the second largest one's one ulp below"""
    depth = rng.uniform(0.05, 1.0, mask.shape).astype(np.float32)
    roots, areas = M.component_areas(lab)
    order = roots[np.argsort(-areas, kind="stable")]
    pinned = []
    for root, peak in zip(order[:2], (thr, np.nextafter(thr, np.float32(0.0)))):
        sel = lab == root
        depth[sel] = np.minimum(depth[sel], peak)
        idx = np.flatnonzero(sel.ravel())
        depth.ravel()[idx[len(idx) // 2]] = peak
        pinned.append((root, peak))
    return depth, pinned


BLOB_MASKS = ["interlocked_combs", "checker", "random_0.41", "tie_equal_areas"]
# (frames, gmax, min_peak_mm, rel_frac): the relative threshold wins, the absolute one wins, rel_frac < 0 switches the relative one off
BLOB_RUNS = [(BLOB_MASKS[:3], 0.9371, 0.2, 0.6), (BLOB_MASKS[1:], 0.9371, 0.61, 0.3), (BLOB_MASKS[:3], 0.9371, 0.55, -1.0)]


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", [(33, 65), (224, 224)], ids=["33x65", "224x224"])
def test_blob_filter_equals_reference(pkg, h, w):
    import torch
    cat = {k: catalogue(h, w)[k] for k in BLOB_MASKS}
    assert_claims(cat)
    rng = np.random.default_rng(h * w)
    lib = pkg._lib.load()
    for names, gmax, min_peak, rel_frac in BLOB_RUNS:
        gm = np.full(B, gmax, np.float32) * np.array([1.0, 0.5, 1.25], np.float32)
        depth, want_kept, want_depth = [], [], []
        for j, k in enumerate(names):
            mask, lab = cat[k]
            thr = M.blob_threshold(gm[j], min_peak, rel_frac)
            assert thr == np.float32(min_peak) if rel_frac < 0 else thr >= np.float32(min_peak)
            d, pinned = _blob_frame(mask, lab, thr, rng)
            kept, dout = M.ref_blob(d, mask, lab, gm[j], min_peak, rel_frac)
            # the component whose peak is exactly the threshold is kept, the one an ulp below removed
            assert kept[lab == pinned[0][0]].all() and d[lab == pinned[0][0]].max() == thr
            if len(pinned) > 1:
                assert not kept[lab == pinned[1][0]].any() and (dout[lab == pinned[1][0]] == 0).all()
            depth.append(d); want_kept.append(kept); want_depth.append(dout)
        assert any(k.any() for k in want_kept) and any(((m != 0) & (k == 0)).any() for k, m in zip(want_kept, (cat[n][0] for n in names)))
        dd = _dev(np.stack(depth))
        dc, dl, dg = _dev(np.stack([cat[k][0] for k in names])), _dev(np.stack([cat[k][1] for k in names])), _dev(gm)
        dk = torch.full((B, h, w), 77, dtype=torch.uint8, device="cuda")
        pkg._lib.check(lib.vistaf_ftp_test_blob_filter(_ptr(dd), _ptr(dc), _ptr(dl), _ptr(dg), min_peak, rel_frac, _ptr(dk), B, h * w, None))
        got_k, got_d = dk.cpu().numpy(), dd.cpu().numpy()
        for j, k in enumerate(names):
            assert np.array_equal(got_k[j], want_kept[j]), (k, rel_frac, _first_diff(got_k[j], want_kept[j]))
            assert np.array_equal(got_d[j].view(np.uint32), want_depth[j].view(np.uint32)), (k, rel_frac, _first_diff(got_d[j], want_depth[j]))


# =======================================================================================================================================
# CPU: the references against the oracle and against plain restatements; the hooks' argument checks

CPU_SHAPES = [(1, 1), (5, 7), (1, 300), (300, 1), (33, 65), (70, 63), (3, 200)]


def test_ref_labels_partition_equals_the_oracle_labelling():
    for h, w in CPU_SHAPES:
        cat = catalogue(h, w)
        assert_claims(cat)
        for name, (m, lab) in cat.items():
            num, cl, areas = cvlite.cc8(m)
            roots, counts = M.component_areas(lab)
            assert num - 1 == len(roots) and np.array_equal(cl > 0, lab >= 0), name
            pairs = np.unique(np.stack([cl[cl > 0], lab[cl > 0]]), axis=1)
            assert pairs.shape[1] == len(roots), name                       # one root per oracle label and the other way round
            # the oracle numbers components in raster order of their first pixel: the largest pick of shape_ftp.py is ref_largest
            if len(roots):
                assert np.array_equal(pairs[1], roots) and np.array_equal(areas[1:], counts), name
                assert np.array_equal(M.ref_largest(lab), (cl == 1 + int(np.argmax(areas[1:]))).astype(np.uint8)), name


def _flood_labels(mask):
    h, w = mask.shape
    out = np.full((h, w), -1, np.int32)
    for p in range(h * w):                  # ascending: the first pixel met of a component is its smallest index
        if mask.flat[p] == 0 or out.flat[p] >= 0:
            continue
        stack = [p]
        out.flat[p] = p
        while stack:
            y, x = divmod(stack.pop(), w)
            for yy in range(max(0, y - 1), min(h, y + 2)):
                for xx in range(max(0, x - 1), min(w, x + 2)):
                    if mask[yy, xx] and out[yy, xx] < 0:
                        out[yy, xx] = p
                        stack.append(yy * w + xx)
    return out


def test_ref_labels_equal_a_flood_fill_on_small_masks():
    for h, w in [(1, 1), (5, 7), (1, 300), (9, 11), (13, 15)]:
        for name, m in M.hard_masks(h, w, 7 * h + w).items():
            assert np.array_equal(M.ref_labels(m), _flood_labels(m)), (h, w, name)


def test_closed_form_restatement_keeps_the_contract_against_the_oracle_transform():
    rng = np.random.default_rng(20)
    for h, w, cap_px in [(5, 7, 3), (5, 7, 11), (33, 65, 3), (17, 64, 11), (40, 129, 5), (40, 515, 3), (9, 1301, 5)]:
        ms = {"random_%g" % p: (rng.random((h, w)) < p).astype(np.uint8) for p in (0.01, 0.1, 0.3, 0.5, 0.9, 0.99)}
        ms.update(M.chamfer_masks(h, w))
        n_in = n_out = 0
        for name, m in ms.items():
            for zero in (m == 0, m != 0):
                ref = cvlite.dist_l2_3x3((~zero).astype(np.uint8))
                msg, a, b = M.chamfer_contract(M.closed_form_chamfer(zero, cap_px), ref, cap_px)
                assert msg is None, (h, w, cap_px, name, msg)
                n_in, n_out = n_in + a, n_out + b
        assert n_in > 0 and (n_out > 0 or (h, w, cap_px) == (5, 7, 11))         # that band covers the whole frame


def test_ref_blob_threshold_and_peak_rule():
    lab = np.array([[0, 0, -1, 3], [-1, -1, -1, 3]], np.int32)
    cand = (lab >= 0).astype(np.uint8)
    thr = M.blob_threshold(np.float32(0.7), 0.1, 0.5)
    assert thr == np.float32(0.5 * float(np.float32(0.7))) and M.blob_threshold(0.7, 0.1, -1.0) == np.float32(0.1)
    depth = np.array([[0.1, thr, 9.0, 0.2], [9.0, 9.0, 9.0, np.nextafter(thr, np.float32(0))]], np.float32)
    kept, out = M.ref_blob(depth, cand, lab, np.float32(0.7), 0.1, 0.5)
    assert np.array_equal(kept, [[1, 1, 0, 0], [0, 0, 0, 0]])
    assert np.array_equal(out, np.array([[0.1, thr, 9.0, 0.0], [9.0, 9.0, 9.0, 0.0]], np.float32))


def test_mask_hooks_refuse_bad_scalar_arguments(pkg):
    """only scalars are wrong here: every plane is a live buffer, and a refused call touches none of them (no HIP call is made)"""
    lib = pkg._lib.load()
    buf = [np.zeros(64, np.int32) for _ in range(6)]
    p = [ctypes.c_void_p(b.ctypes.data) for b in buf]
    ok_label = dict(B=1, h=2, w=3, variant=0)
    for bad in (dict(B=0), dict(B=-1), dict(h=0), dict(w=0), dict(w=-5), dict(variant=2), dict(variant=-1), dict(h=65536, w=65536)):
        a = dict(ok_label, **bad)
        assert lib.vistaf_ftp_test_cc_label(p[0], p[1], a["B"], a["h"], a["w"], a["variant"], None) == E_INVALID, bad
    for bad in (dict(B=0), dict(P=0), dict(P=-3), dict(variant=3), dict(variant=-1)):
        a = dict(dict(B=1, P=6, variant=0), **bad)
        assert lib.vistaf_ftp_test_cc_largest(p[0], p[1], p[2], a["B"], a["P"], a["variant"], None) == E_INVALID, bad
    for bad in (dict(B=0), dict(h=0), dict(w=0), dict(cap_px=-1), dict(h=65536, w=65536)):
        a = dict(dict(B=1, h=2, w=3, cap_px=3), **bad)
        for pair in (0, 1):
            assert lib.vistaf_ftp_test_chamfer_dispatch(p[0], pair, 0, p[1], p[2], a["B"], a["h"], a["w"], a["cap_px"], None) == E_INVALID, bad
    for bad in (dict(B=0), dict(P=0), dict(P=-1)):
        a = dict(dict(B=1, P=6), **bad)
        assert lib.vistaf_ftp_test_blob_filter(p[0], p[1], p[2], p[3], 0.1, 0.3, p[4], a["B"], a["P"], None) == E_INVALID, bad
    # a null plane is refused the same way (and_static alone may be null)
    assert lib.vistaf_ftp_test_cc_label(None, p[1], 1, 2, 3, 0, None) == E_INVALID
    assert lib.vistaf_ftp_test_cc_label(p[0], None, 1, 2, 3, 0, None) == E_INVALID
    assert lib.vistaf_ftp_test_cc_largest(None, None, p[2], 1, 6, 0, None) == E_INVALID
    assert lib.vistaf_ftp_test_cc_largest(p[0], None, None, 1, 6, 0, None) == E_INVALID
    assert lib.vistaf_ftp_test_chamfer_dispatch(None, 0, 0, p[1], None, 1, 2, 3, 3, None) == E_INVALID
    assert lib.vistaf_ftp_test_chamfer_dispatch(p[0], 0, 0, None, None, 1, 2, 3, 3, None) == E_INVALID
    assert lib.vistaf_ftp_test_chamfer_dispatch(p[0], 1, 0, p[1], None, 1, 2, 3, 3, None) == E_INVALID
    for i in range(5):
        args = [p[0], p[1], p[2], p[3], p[4]]
        args[i] = None
        assert lib.vistaf_ftp_test_blob_filter(args[0], args[1], args[2], args[3], 0.1, 0.3, args[4], 1, 6, None) == E_INVALID, i
    assert b"bad argument" in lib.vistaf_ftp_last_error()
