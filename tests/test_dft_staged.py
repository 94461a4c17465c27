"""The LDS-staged demodulation kernels (csrc/k_dft.hip: k_dft_fwd1_staged, k_dft_inv2_staged; session hook "dft_staged", csrc/test_hooks.h)
against the kernels they stand in for, which read their operands from global memory.

Main bar: variant 2 (staged) equals variant 1 (the kernels before) BIT FOR BIT on T, patch, Q, field, amp, wrapped and prod -- the staged
kernels feed every accumulator the same k-steps in the same order with the same operands and leave the epilogue's expressions alone.  Both
variants are also held to the longdouble references and derived bounds of tests/kernel_refs.py (the checks of tests/test_dft_direct.py, whose
helpers run here), and every output is followed by sentinels that must survive.  Shapes sit on the edges of the staged kernels: one row past
a strip of 16, one column past a 64-column tile and past one and two 32-column table chunks, a second column tile that is mostly padding,
pw = 1, batches and segments that do not fill a workgroup's four strips, per-frame tables, per-frame extents below the layout."""
import ctypes
import os

import numpy as np
import pytest
import torch

import kernel_refs as R
import test_dft_direct as DD

pytestmark = pytest.mark.gpu
LD, S, SC = DD.LD, DD.S, DD.SC
_dev, _ptr, _full, _ratio, _parts, rand_tables = DD._dev, DD._ptr, DD._full, DD._ratio, DD._parts, DD.rand_tables
FWD1, INV2 = 1, 2                    # bits of vistaf_ftp_test_dft_staged_fits
XC = 32                              # k_dft_fwd1_staged: columns of the table per chunk


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype.itemsize % 8 == 0 else np.uint32)


def _same_bits(tag, a, b):
    assert a.shape == b.shape and a.dtype == b.dtype, tag
    ne = _bits(a) != _bits(b)
    print("  %-44s %d of %d words differ between the variants" % (tag, int(ne.sum()), ne.size))
    assert not ne.any(), tag


# =======================================================================================================================================
# what a shape takes

def test_the_hooks_have_matching_signatures(pkg):
    """csrc/test_hooks_dft.h against _lib.DFT_STAGED_SIGNATURES: the same functions, and a pointer where the header has one"""
    import re
    text = open(os.path.join(os.path.dirname(pkg.__file__), "csrc", "test_hooks_dft.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    protos = {name: [p.strip() for p in params.split(",")] for name, params in re.findall(r"\bint\s+(vistaf_\w+)\s*\(([^()]*)\)\s*;", text)}
    table = pkg._lib.DFT_STAGED_SIGNATURES
    assert sorted(protos) == sorted(table) and len(protos) == 3
    for name, params in protos.items():
        restype, argtypes = table[name]
        assert restype is ctypes.c_int and len(argtypes) == len(params), name
        for p, a in zip(params, argtypes):
            if "*" in p:
                assert a is ctypes.c_void_p, (name, p)
            else:
                assert a is (ctypes.c_size_t if p.startswith("size_t") else ctypes.c_int), (name, p)


def test_what_a_shape_takes(pkg):
    fits = pkg._lib.load().vistaf_ftp_test_dft_staged_fits
    assert fits(224, 224, 21, 21, 0) == FWD1 | INV2 and fits(224, 224, 21, 21, 1) == FWD1 | INV2
    assert fits(1182, 1182, 21, 21, 0) == FWD1 | INV2              # the table goes in chunks: the frame size excludes nothing
    assert fits(40, 40, 22, 24, 0) == FWD1 | INV2 and fits(40, 40, 23, 24, 0) == FWD1 and fits(40, 40, 22, 25, 0) == INV2
    assert fits(40, 40, 33, 33, 0) == 0 and fits(1, 1, 1, 1, 1) == FWD1 | INV2
    assert fits(0, 4, 2, 2, 0) < 0
    # variant 2 refuses a shape the staged kernel does not take, and launches nothing
    p = ctypes.c_void_p(torch.zeros(16384, dtype=torch.float64, device="cuda").data_ptr())
    lib = pkg._lib.load()
    assert lib.vistaf_ftp_test_dft_forward_v(p, None, p, p, 0, 0, p, 0, p, p, 25 * 25, 1, 4, 4, 25, 25, 2, None) < 0
    assert lib.vistaf_ftp_test_dft_inverse_v(p, 25 * 25, p, p, 0, 0, p, None, p, None, None, 0, None, None, None, 1, 4, 4, 25, 25, 2, None) < 0
    assert lib.vistaf_ftp_test_dft_forward_v(p, None, p, p, 0, 0, p, 0, p, p, 4, 1, 4, 4, 2, 2, 3, None) < 0


# =======================================================================================================================================
# forward transform

def run_forward(pkg, variant, iw, mu, Ex, Ey, win, per_frame, ph, pw, spare_rows=3, spare=5):
    B, h, w = iw.shape
    d = [_dev(x) if x is not None else None for x in (iw, mu, Ex, Ey, win)]
    T = _full((B * h + spare_rows, pw), torch.complex128)
    patch = _full((B, ph * pw + spare), torch.complex128)
    rc = pkg._lib.load().vistaf_ftp_test_dft_forward_v(_ptr(d[0]), _ptr(d[1]), _ptr(d[2]), _ptr(d[3]), w * pw if per_frame else 0, ph * h if per_frame else 0,
                                                       _ptr(d[4]), ph * pw if per_frame else 0, _ptr(T), _ptr(patch), ph * pw + spare, B, h, w, ph, pw, variant,
                                                       None)
    pkg._lib.check(rc)
    return T.cpu().numpy(), patch.cpu().numpy()


def check_forward(pkg, seed, B, h, w, ph, pw, per_frame, with_mu=True):
    """both variants against the reference (the bounds of test_dft_direct.check_forward), sentinels, then against each other"""
    rng = np.random.default_rng(seed)
    iw = rng.standard_normal((B, h, w)).astype(np.float32) * np.float32(3.0)
    mu = (rng.standard_normal(B) * 0.5).astype(np.float32) if with_mu else None
    tb = (B,) if per_frame else ()
    Ex, Ey = rand_tables(rng, tb + (w, pw)), rand_tables(rng, tb + (ph, h))
    win = rng.uniform(-1, 1, tb + (ph, pw)).astype(np.float32)
    a = R.fsub32(iw, mu)
    tr, ti, btr, bti = R.cprod((a if per_frame else a.reshape(B * h, w), None), _parts(Ex))
    sh = (B, h, pw)
    pr, pi, bpr, bpi = R.cprod(_parts(Ey), (tr.reshape(sh), ti.reshape(sh)), bB=(btr.reshape(sh), bti.reshape(sh)))
    wl = win.astype(LD)
    tag = "B=%d h=%d w=%d ph=%d pw=%d %s" % (B, h, w, ph, pw, "per-frame" if per_frame else "shared")
    print(tag)
    got = {}
    for variant in (1, 2, 0):
        T, patch = run_forward(pkg, variant, iw, mu, Ex, Ey, win, per_frame, ph, pw)
        assert (T[B * h:] == SC).all(), "rows past the last segment were written"
        assert (patch[:, ph * pw:] == SC).all(), "the padding behind a patch was written"
        r1 = _ratio("variant %d row stage T" % variant, T[:B * h].reshape(tr.shape), (tr, ti), btr, bti)
        r2 = _ratio("variant %d patch" % variant, patch[:, :ph * pw].reshape(B, ph, pw), (pr * wl, pi * wl), bpr * np.abs(wl), bpi * np.abs(wl))
        assert r1 <= 1.0 and r2 <= 1.0, (tag, variant, r1, r2)
        got[variant] = (T, patch)
    for variant in (2, 0):
        _same_bits("T, variant %d against 1" % variant, got[variant][0], got[1][0])
        _same_bits("patch, variant %d against 1" % variant, got[variant][1], got[1][1])


@pytest.mark.parametrize("h,w", [(17, 2 * XC + 1), (64, 64), (40, 72), (17, XC + 1)])       # 2 XC + 1 = 65: also one past a 64-column tile
@pytest.mark.parametrize("ph,pw", [(21, 21), (5, 9), (7, 1)])
def test_forward_edge_shapes(pkg, h, w, ph, pw):
    """B = 5 with one table: 5 h rows in one segment, strips that are no multiple of a workgroup's four and (h = 17, 40) a frame boundary
    inside a strip; w one past a 64-column tile, not a multiple of 4, one past the table chunk and one past two chunks; 2 pw = 42 (three
    column tiles, the last of ten columns), 18 (a second tile that is mostly padding; K = 2 ph = 10 is for the inverse below) and 2"""
    check_forward(pkg, 1000 * h + 10 * w + pw, 5, h, w, ph, pw, False)


def test_forward_one_frame_without_mu(pkg):
    check_forward(pkg, 77, 1, 17, 65, 21, 21, False, with_mu=False)


def test_forward_per_frame_tables(pkg):
    """B = 3 at h = 40: three segments of 2.5 strips, so every frame's last strip is half empty, its workgroup has a wave without a strip and no
    strip may take rows of the next frame's table"""
    check_forward(pkg, 78, 3, 40, 72, 21, 21, True)
    check_forward(pkg, 79, 3, 40, 33, 5, 9, True)


# =======================================================================================================================================
# inverse transform

def run_inverse(pkg, variant, patch, Gx, Gy, per_frame, B, h, w, ph, pw, want_field=True, cref=None, amp_ref=None, ref_stride=0, gi=None):
    d = [_dev(x) if x is not None else None for x in (patch, Gx, Gy, cref, amp_ref)]
    Q = _full((B, ph, w), torch.complex128)
    tail = 3                                                       # sentinel elements behind every plane
    field = _full((B * h * w + tail,), torch.complex128) if want_field else None
    amp, prod, wrapped = (_full((B * h * w + tail,), torch.float32) for _ in range(3))
    gi_arr = np.ascontiguousarray(gi, np.int32) if gi is not None else None
    rc = pkg._lib.load().vistaf_ftp_test_dft_inverse_v(_ptr(d[0]), patch.shape[1], _ptr(d[1]), _ptr(d[2]), pw * w if per_frame else 0,
                                                       h * ph if per_frame else 0, _ptr(Q), _ptr(field), _ptr(amp), _ptr(d[3]), _ptr(d[4]), ref_stride,
                                                       _ptr(prod), _ptr(wrapped), gi_arr.ctypes.data_as(ctypes.c_void_p) if gi_arr is not None else None,
                                                       B, h, w, ph, pw, variant, None)
    pkg._lib.check(rc)
    out = {"Q": Q.cpu().numpy()}
    for name, t in (("field", field), ("amp", amp), ("prod", prod), ("wrapped", wrapped)):
        if t is None:
            out[name] = None
            continue
        a = t.cpu().numpy()
        assert (a[B * h * w:] == (SC if name == "field" else np.float32(S))).all(), "the elements behind %s were written" % name
        out[name] = a[:B * h * w].reshape(B, h, w)
    return out


def check_inverse(pkg, seed, B, h, w, ph, pw, per_frame, with_ref, ext=None, zero_frame=None):
    rng = np.random.default_rng(seed)
    tb = (B,) if per_frame else ()
    pt = rand_tables(rng, (B, ph, pw))
    if zero_frame is not None:
        pt[zero_frame] = 0
    patch = np.full((B, ph * pw + 3), SC, np.complex128)
    patch[:, :ph * pw] = pt.reshape(B, -1)
    Gx, Gy = rand_tables(rng, tb + (pw, w)), rand_tables(rng, tb + (h, ph))
    gi = None
    if ext is not None:
        gi = np.zeros((B, 10), np.int32)
        gi[:, 2:4] = ext
    cref = amp_ref = None
    if with_ref:
        cref = rng.standard_normal((B, h, w)) + 1j * rng.standard_normal((B, h, w))
        amp_ref = rng.uniform(0, 3, (B, h, w)).astype(np.float32)
    qs, fs = DD.inverse_ref(pt, Gx, Gy, ext)
    tag = "B=%d h=%d w=%d ph=%d pw=%d %s%s" % (B, h, w, ph, pw, "per-frame" if per_frame else "shared", " cref" if with_ref else "")
    print(tag)
    got = {}
    for variant in (1, 2, 0):
        out = run_inverse(pkg, variant, patch, Gx, Gy, per_frame, B, h, w, ph, pw, want_field=True, cref=cref, amp_ref=amp_ref,
                          ref_stride=h * w if with_ref else 0, gi=gi)
        DD.check_inverse_outputs("%s variant %d" % (tag, variant), out, qs, fs, B, ext)
        if not with_ref:
            assert (out["prod"] == np.float32(S)).all() and (out["wrapped"] == np.float32(S)).all()
        else:
            assert np.isfinite(out["wrapped"]).all() and (np.abs(out["wrapped"]) <= np.float32(np.pi)).all()
            assert np.array_equal(_bits(out["prod"]), _bits(amp_ref * out["amp"]))
        if zero_frame is not None:
            # atan2 of two zeros is 0 or +-pi by their signs (tests/test_dft_direct.py pins them against NumPy); here the variants must agree
            assert (out["amp"][zero_frame] == 0).all() and (out["field"][zero_frame] == 0).all()
            if with_ref:
                assert np.isin(np.abs(out["wrapped"][zero_frame]), [np.float32(0), np.float32(np.pi)]).all()
        got[variant] = out
    for variant in (2, 0):
        for name in ("Q", "field", "amp") + (("wrapped", "prod") if with_ref else ()):
            _same_bits("%s, variant %d against 1" % (name, variant), got[variant][name], got[1][name])
    # without the float64 field: the same float32 planes
    out = run_inverse(pkg, 2, patch, Gx, Gy, per_frame, B, h, w, ph, pw, want_field=False, cref=cref, amp_ref=amp_ref,
                      ref_stride=h * w if with_ref else 0, gi=gi)
    for name in ("amp",) + (("wrapped", "prod") if with_ref else ()):
        _same_bits("%s without field" % name, out[name], got[1][name])


@pytest.mark.parametrize("h,w", [(17, 2 * XC + 1), (64, 64), (40, 72), (17, XC + 1)])       # 2 XC + 1 = 65: also one past a 64-column tile
@pytest.mark.parametrize("ph,pw", [(21, 21), (5, 9), (7, 1)])
@pytest.mark.parametrize("with_ref", [False, True], ids=["cref_null", "cref"])
def test_inverse_edge_shapes(pkg, h, w, ph, pw, with_ref):
    """h one past a strip, a full workgroup of strips, 2.5 strips; w one past a 64-column block (a block of one column: the second pass over the
    column tiles is skipped), inside one (w = 33: one pass of two tiles, the second a single column), 72 (a block of eight columns);
    K = 2 ph = 42, 10 (not a multiple of 4: the k guard) and 14; B = 5; with and without a reference field"""
    check_inverse(pkg, 2000 * h + 20 * w + ph + int(with_ref), 5, h, w, ph, pw, False, with_ref)


def test_inverse_one_frame_and_an_all_zero_patch(pkg):
    check_inverse(pkg, 81, 1, 17, 65, 21, 21, False, False)
    check_inverse(pkg, 85, 1, 17, 65, 22, 3, False, True)          # the largest patch height the staged kernel takes: 48 KB of LDS
    check_inverse(pkg, 82, 2, 17, 65, 21, 21, False, True, zero_frame=1)


def test_inverse_per_frame_tables_and_extents(pkg):
    """per-frame tables with B = 3 at h = 40; then per-frame extents below an 8 x 7 layout (one frame beyond it: clamped; one 5 x 4, whose rows
    5..7 of Q keep their sentinels and whose k-steps change from real to imaginary parts at 5)"""
    check_inverse(pkg, 83, 3, 40, 72, 21, 21, True, True)
    check_inverse(pkg, 84, 3, 17, 65, 8, 7, True, True, ext=[(8, 7), (5, 4), (1, 1)])


def test_224_batch_of_two(pkg):
    """the workload's frame and patch once, both transforms"""
    check_forward(pkg, 91, 2, 224, 224, 21, 21, False)
    check_inverse(pkg, 92, 2, 224, 224, 21, 21, False, True)


# =======================================================================================================================================
# sessions

def _outputs(out):
    return {k: v.cpu().numpy().copy() for k, v in out.items()}


def test_sessions_give_the_same_outputs_with_and_without_the_tier(pkg):
    """predict_batch and predict_pairs on 4 frames of 224 x 224 with dft_staged 1, 0 and 1 again: identical outputs"""
    g = os.path.join(os.path.dirname(__file__), "golden")
    model, neg = pkg.load_calibration(os.path.join(g, "calibration_phase_to_height.json"))
    fm = pkg.load_force_calibration(os.path.join(g, "calibration_height_to_force.json"))["best_model"]
    n, nb = 224, 4
    cfg = pkg.FtpConfig.scaled(n)
    ref = pkg.synth.reference_frame(n, config=3)
    frames = pkg.synth.deformed_batch(n, 500, nb, config=3)
    periods = [pkg.synth.NATIVE_PERIOD_PX * n / pkg.synth.NATIVE_CROP, 11.3]
    refs = np.stack([pkg.synth._base(n, 0.0, np.random.default_rng(880000 + b), periods[b % 2]) for b in range(nb)])
    defs = np.stack([pkg.synth.deformed_frame(n, 4100 + b, config=3, period=periods[b % 2], amp_scale=1.0 + 0.5 * (b % 3)) for b in range(nb)])
    batch = pkg.FtpSensor(ref, pkg.synth.roi_circle(n), cfg, model, neg, fm, max_batch=nb)
    pairs = pkg.FtpSensor(None, pkg.synth.roi_circle(n), cfg, model, neg, fm, max_batch=nb, frame_shape=(n, n))
    res = []
    for tier in (1, 0, 1):
        batch._test_set("dft_staged", tier)
        pairs._test_set("dft_staged", tier)
        a, b = _outputs(batch.predict_batch(frames)), _outputs(pairs.predict_pairs(refs, defs))
        torch.cuda.synchronize()
        assert (a["status"] == 0).all() and (b["status"] == 0).all()
        res.append((a, b))
    batch.close()
    pairs.close()
    for other in (res[0], res[2]):
        for got, want in zip(other, res[1]):
            assert set(got) == set(want) and {"height_map_mm", "output_reliable", "scalars", "status"} <= set(got)
            for key in want:
                assert got[key].tobytes() == want[key].tobytes(), key
