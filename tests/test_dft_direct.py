"""The demodulation kernels launched directly (csrc/test_hooks.h: vistaf_ftp_test_dft_forward / _dft_inverse / _dft_full_mag / _build_tables /
_build_full_tables / _top_peaks / _carrier_choose) on planes, tables and peak lists no fringe image produces, against the longdouble references
of tests/kernel_refs.py and the cases of tests/dft_cases.py.

Tolerances come from the reference, not from the kernels: a float64 sum of K real k-steps is held to (K + 3) 2^-53 (|A| . |B|) per output
element (plus what the bound of the stage before propagates), a table entry to the bound derived next to its reference, a float32 output to
the float32 rounding of the reference (either neighbour where the reference is within the float64 bound of a rounding boundary), a refined
peak to the sensitivity of the parabola times 2 ulp of the logarithms.  Integer results, orders and untouched memory are exact.  Every
measured maximum is printed next to its bound before it is asserted (run with -s to see them).  Outputs are filled with sentinels before
every call."""
import ctypes

import numpy as np
import pytest
import torch

import dft_cases as D
import kernel_refs as R
from oracle import cvlite
from oracle import ftp_oracle as O

pytestmark = pytest.mark.gpu
LD = R.LD
S = -7777.0                     # sentinel of every output plane
SC = complex(S, S)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _full(shape, dtype):
    return torch.full(shape, SC if dtype == torch.complex128 else S, dtype=dtype, device="cuda")


def _ratio(tag, got, ref, bre, bim=None):
    """max over the elements of |got - ref| / bound (a complex `got`: ref = (re, im), both parts against their own bound); printed, returned.
    An error where the bound is zero counts as infinite"""
    got = np.asarray(got)
    if bim is None:
        err, b = np.abs(got.astype(LD) - ref).ravel(), np.broadcast_to(np.asarray(bre, LD), got.shape).ravel()
    else:
        assert got.shape == np.shape(ref[0]) == np.shape(bre) == np.shape(bim), (got.shape, np.shape(ref[0]), np.shape(bre))
        err = np.concatenate([np.abs(got.real.astype(LD) - ref[0]).ravel(), np.abs(got.imag.astype(LD) - ref[1]).ravel()])
        b = np.concatenate([np.asarray(bre, LD).ravel(), np.asarray(bim, LD).ravel()])
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, LD(0), err / b)
    worst = float(r.max()) if r.size else 0.0
    print("  %-44s max |err| %.3g, max err / bound %.3f" % (tag, float(err.max()) if err.size else 0.0, worst))
    return worst


def _assert_f32(tag, got, ref, bound):
    lo, hi = R.f32_interval(ref, bound)
    got = np.asarray(got, np.float32)
    ok = (got >= lo) & (got <= hi)
    print("  %-44s %d of %d float32 results may be either neighbour; %d wrong" % (tag, int((lo != hi).sum()), got.size, int((~ok).sum())))
    assert ok.all(), (tag, got[~ok][:4], lo[~ok][:4], hi[~ok][:4])


def rand_tables(rng, shape):
    """complex128, both parts of mixed sign and of magnitudes from 1e-3 to 1e3: nothing a twiddle table has, so that a swap of re and im or a
    tile offset cannot cancel"""
    def part():
        return rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-3, 3, shape)
    return part() + 1j * part()


def _parts(z):
    return z.real.astype(LD), z.imag.astype(LD)


# =======================================================================================================================================
# row stage and forward transform

def run_forward(pkg, iw, mu, Ex, Ey, win, per_frame, ph, pw, spare_rows=3, spare=5):
    """-> (T [B * h + spare_rows][pw], patch [B][ph * pw + spare]) complex128, sentinels wherever the launcher does not write"""
    B, h, w = iw.shape
    d = [_dev(x) if x is not None else None for x in (iw, mu, Ex, Ey, win)]
    T = _full((B * h + spare_rows, pw), torch.complex128)
    patch = _full((B, ph * pw + spare), torch.complex128)
    rc = pkg._lib.load().vistaf_ftp_test_dft_forward(_ptr(d[0]), _ptr(d[1]), _ptr(d[2]), _ptr(d[3]), w * pw if per_frame else 0, ph * h if per_frame else 0,
                                                     _ptr(d[4]), ph * pw if per_frame else 0, _ptr(T), _ptr(patch), ph * pw + spare, B, h, w, ph, pw, None)
    pkg._lib.check(rc)
    return T.cpu().numpy(), patch.cpu().numpy()


def check_forward(pkg, rng, B, h, w, ph, pw, per_frame, mu):
    iw = rng.standard_normal((B, h, w)).astype(np.float32) * np.float32(3.0)
    tb = (B,) if per_frame else ()
    Ex, Ey = rand_tables(rng, tb + (w, pw)), rand_tables(rng, tb + (ph, h))
    win = (rng.uniform(-1, 1, tb + (ph, pw))).astype(np.float32)
    T, patch = run_forward(pkg, iw, mu, Ex, Ey, win, per_frame, ph, pw)
    a = R.fsub32(iw, mu)
    exr, exi = _parts(Ex)
    tr, ti, btr, bti = R.cprod((a if per_frame else a.reshape(B * h, w), None), (exr, exi))
    tag = "B=%d h=%d w=%d ph=%d pw=%d %s" % (B, h, w, ph, pw, "per-frame" if per_frame else "shared")
    print(tag)
    assert (T[B * h:] == SC).all(), "rows past the last segment were written"
    r1 = _ratio("row stage T", T[:B * h].reshape(tr.shape), (tr, ti), btr, bti)
    sh = (B, h, pw)
    pr, pi, bpr, bpi = R.cprod(_parts(Ey), (tr.reshape(sh), ti.reshape(sh)), bB=(btr.reshape(sh), bti.reshape(sh)))
    wl = win.astype(LD)
    assert (patch[:, ph * pw:] == SC).all(), "the padding behind a patch was written"
    r2 = _ratio("patch", patch[:, :ph * pw].reshape(B, ph, pw), (pr * wl, pi * wl), bpr * np.abs(wl), bpi * np.abs(wl))
    assert r1 <= 1.0 and r2 <= 1.0, (tag, r1, r2)
    return iw, Ex, Ey, win, T, patch


@pytest.mark.parametrize("ph,pw", [(5, 7), (5, 8), (5, 9), (33, 33)])
def test_forward_shared_table(pkg, ph, pw):
    """27 rows (two strips, the second of 11 rows), w % 4 = 2, h % 8 = 1; 14, 16, 18 real columns (one tile short, one full, one into the
    second) and 66 (five tiles: two passes over x); 33 x 33 bins take the second trip of k_dft_fwd2's loop"""
    check_forward(pkg, np.random.default_rng(100 + pw), 3, 9, 10, ph, pw, False, np.array([0.25, -1.5, 0.0], np.float32))


@pytest.mark.parametrize("h", [24, 9])
def test_forward_per_frame_tables_and_windows(pkg, h):
    """one segment per frame (strips restart at each frame's first row; h = 24 and 9 leave 8 and 9 rows in the last strip); the three mu are
    distinct: a negative zero, a small one, and one large enough that iw - mu rounds in float32"""
    mu = np.array([-0.0, 0.37, 30000.0], np.float32)
    assert np.signbit(mu[0]) and np.isfinite(mu).all()
    check_forward(pkg, np.random.default_rng(200 + h), 3, h, 10, 5, 7, True, mu)
    check_forward(pkg, np.random.default_rng(300 + h), 3, h, 10, 5, 7, True, None)


@pytest.mark.parametrize("per_frame", [False, True])
def test_a_row_does_not_depend_on_its_batch_position(pkg, per_frame):
    """the same frame (and tables) at position 0 of a batch of one and at position 2 of a batch of three: equal bits.  With h = 9 the frame
    starts at row 18 of the shared segment, inside a strip"""
    rng = np.random.default_rng(9)
    B, h, w, ph, pw = 3, 9, 10, 5, 9
    iw = rng.standard_normal((B, h, w)).astype(np.float32)
    mu = np.array([0.1, 0.2, 0.3], np.float32)
    tb = (B,) if per_frame else ()
    Ex, Ey, win = rand_tables(rng, tb + (w, pw)), rand_tables(rng, tb + (ph, h)), rng.uniform(-1, 1, tb + (ph, pw)).astype(np.float32)
    T3, p3 = run_forward(pkg, iw, mu, Ex, Ey, win, per_frame, ph, pw)
    one = (lambda x: x[2:3]) if per_frame else (lambda x: x)
    T1, p1 = run_forward(pkg, iw[2:3], mu[2:3], one(Ex), one(Ey), one(win), per_frame, ph, pw)
    assert np.array_equal(T3[2 * h:3 * h].view(np.uint64), T1[:h].view(np.uint64))
    assert np.array_equal(p3[2, :ph * pw].view(np.uint64), p1[0, :ph * pw].view(np.uint64))


def run_full_mag(pkg, planes, Exh, Eyf, Hf, Wf, spare_rows=2):
    B, h, w = planes.shape
    Wh = Wf // 2 + 1
    T = _full((B * h + spare_rows, Wh), torch.complex128)
    mag = torch.full((B, Hf, Wf), -1.0, dtype=torch.float64, device="cuda")
    d = [_dev(planes), _dev(Exh), _dev(Eyf)]
    rc = pkg._lib.load().vistaf_ftp_test_dft_full_mag(_ptr(d[0]), _ptr(d[1]), _ptr(d[2]), _ptr(T), _ptr(mag), B, h, w, Hf, Wf, None)
    pkg._lib.check(rc)
    torch.cuda.synchronize()
    return T.cpu().numpy(), mag.cpu().numpy()


@pytest.mark.parametrize("Wf", [128, 256])
def test_row_launcher_at_65_and_129_columns(pkg, Wf):
    """launch_dft_rows (the row transform of the full spectrum and of the pressure read-out) with nc = Wf / 2 + 1 = 65 and 129 columns: 9 and 17
    column tiles, the last one of a single column, in 3 and 5 passes"""
    rng = np.random.default_rng(Wf)
    B, h, pad = 2, 24, 4
    w, Hf, Wh = Wf - 2 * pad, h + 2 * pad, Wf // 2 + 1
    planes = rng.standard_normal((B, h, w)).astype(np.float32)
    Exh, Eyf = rand_tables(rng, (w, Wh)), rand_tables(rng, (Hf, h))
    T, _ = run_full_mag(pkg, planes, Exh, Eyf, Hf, Wf)
    tr, ti, btr, bti = R.cprod((planes.reshape(B * h, w).astype(LD), None), _parts(Exh))
    print("rows nc=%d" % Wh)
    assert (T[B * h:] == SC).all()
    assert _ratio("row stage T", T[:B * h], (tr, ti), btr, bti) <= 1.0


# =======================================================================================================================================
# inverse transform

def run_inverse(pkg, patch, Gx, Gy, per_frame, B, h, w, ph, pw, want_field=True, cref=None, amp_ref=None, ref_stride=0, gi=None, spare=3):
    """-> dict of Q [B][ph][w], field (or None), amp, prod, wrapped; patch [B][ph * pw + spare]"""
    d = [_dev(x) if x is not None else None for x in (patch, Gx, Gy, cref, amp_ref)]
    Q = _full((B, ph, w), torch.complex128)
    field = _full((B, h, w), torch.complex128) if want_field else None
    amp, prod, wrapped = (_full((B, h, w), torch.float32) for _ in range(3))
    gi_arr = np.ascontiguousarray(gi, np.int32) if gi is not None else None
    rc = pkg._lib.load().vistaf_ftp_test_dft_inverse(_ptr(d[0]), patch.shape[1], _ptr(d[1]), _ptr(d[2]), pw * w if per_frame else 0, h * ph if per_frame else 0,
                                                     _ptr(Q), _ptr(field), _ptr(amp), _ptr(d[3]), _ptr(d[4]), ref_stride, _ptr(prod), _ptr(wrapped),
                                                     gi_arr.ctypes.data_as(ctypes.c_void_p) if gi_arr is not None else None, B, h, w, ph, pw, None)
    pkg._lib.check(rc)
    return {"Q": Q.cpu().numpy(), "field": field.cpu().numpy() if want_field else None, "amp": amp.cpu().numpy(), "prod": prod.cpu().numpy(),
            "wrapped": wrapped.cpu().numpy()}


def inverse_ref(patch, Gx, Gy, ext=None):
    """patch [B][ph][pw], Gx [(B,) pw][w], Gy [(B,) h][ph] complex128; ext: per frame (ph_b, pw_b) limiting the sums.  -> (Q, field) as
    (re, im, bre, bim), Q rows beyond a frame's ph_b zero"""
    B, ph, pw = patch.shape
    qs, fs = [], []
    for b in range(B):
        gx, gy = (Gx[b] if Gx.ndim == 3 else Gx), (Gy[b] if Gy.ndim == 3 else Gy)
        a, c = ext[b] if ext is not None else (ph, pw)
        q = R.cprod(_parts(patch[b, :a, :c]), _parts(gx[:c]))
        f = R.cprod(_parts(gy[:, :a]), q[:2], bB=q[2:])
        qs.append(q)
        fs.append(f)
    return qs, fs


amp_bound = R.amp_bound


def check_inverse_outputs(tag, out, qs, fs, B, ext=None, want_field=True):
    worst = 0.0
    for b in range(B):
        a = ext[b][0] if ext is not None else out["Q"].shape[1]
        worst = max(worst, _ratio("%s Q[%d]" % (tag, b), out["Q"][b, :a], qs[b][:2], qs[b][2], qs[b][3]))
        assert (out["Q"][b, a:] == SC).all(), "rows of Q beyond the frame's own ph were written"
        fr, fi, bre, bim = fs[b]
        if want_field:
            worst = max(worst, _ratio("%s field[%d]" % (tag, b), out["field"][b], (fr, fi), bre, bim))
        _assert_f32("%s amp[%d]" % (tag, b), out["amp"][b], *amp_bound(fr, fi, bre, bim))
    assert worst <= 1.0, (tag, worst)


@pytest.mark.parametrize("h,w,ph,pw", [(16, 8, 1, 1), (17, 63, 2, 7), (70, 65, 7, 7), (16, 257, 8, 7), (17, 257, 7, 1), (70, 8, 8, 1), (17, 65, 1, 7)])
@pytest.mark.parametrize("per_frame", [False, True])
def test_inverse(pkg, h, w, ph, pw, per_frame):
    """h = 16, 17, 70 (one full strip, one row into the second, a second workgroup row); w = 8, 63, 65, 257 (inside one column tile, one short of
    a wave's 64, one past it, five blocks); K = 2 ph = 2, 4, 14, 16 real k-steps (the k guard of the MFMA loop active and idle); pw 1 and 7.
    With and without the float64 field: the same amplitude bits, and prod / wrapped untouched without a reference field"""
    rng = np.random.default_rng(h * 1000 + w + ph)
    B = 2
    tb = (B,) if per_frame else ()
    patch = np.full((B, ph * pw + 3), SC, np.complex128)
    pt = rand_tables(rng, (B, ph, pw))
    patch[:, :ph * pw] = pt.reshape(B, -1)
    Gx, Gy = rand_tables(rng, tb + (pw, w)), rand_tables(rng, tb + (h, ph))
    qs, fs = inverse_ref(pt, Gx, Gy)
    tag = "h=%d w=%d ph=%d pw=%d %s" % (h, w, ph, pw, "per-frame" if per_frame else "shared")
    print(tag)
    out = run_inverse(pkg, patch, Gx, Gy, per_frame, B, h, w, ph, pw, want_field=True)
    check_inverse_outputs(tag, out, qs, fs, B)
    assert (out["prod"] == np.float32(S)).all() and (out["wrapped"] == np.float32(S)).all()
    out2 = run_inverse(pkg, patch, Gx, Gy, per_frame, B, h, w, ph, pw, want_field=False)
    assert np.array_equal(out2["amp"].view(np.uint32), out["amp"].view(np.uint32)) and np.array_equal(out2["Q"].view(np.uint64), out["Q"].view(np.uint64))
    assert (out2["prod"] == np.float32(S)).all() and (out2["wrapped"] == np.float32(S)).all()


def test_inverse_with_a_frame_limited_below_the_layout(pkg):
    """pair mode: an 8 x 7 layout, the second sample's own patch 5 x 4: its sums stop there whatever the tables and the patch hold beyond
    (deliberately not zeros here), rows 5..7 of its Q are not written"""
    rng = np.random.default_rng(41)
    B, h, w, ph, pw = 2, 17, 65, 8, 7
    pt = rand_tables(rng, (B, ph, pw))
    Gx, Gy = rand_tables(rng, (B, pw, w)), rand_tables(rng, (B, h, ph))
    ext = [(8, 7), (5, 4)]
    gi = np.zeros((B, 10), np.int32)
    gi[0, 2:4], gi[1, 2:4] = (8, 7), (5, 4)
    gi[0, 2] = 11                                       # beyond the layout: clamped to it
    qs, fs = inverse_ref(pt, Gx, Gy, ext)
    out = run_inverse(pkg, pt.reshape(B, -1), Gx, Gy, True, B, h, w, ph, pw, gi=gi)
    print("limited frame")
    check_inverse_outputs("limited", out, qs, fs, B, ext)


@pytest.mark.parametrize("ref_stride_frames", [0, 1])
def test_inverse_against_a_reference_field(pkg, ref_stride_frames):
    """wrapped = float32 angle(field * conj(cref)) on the circle and prod = amp_ref * amp, one reference for the batch or one per frame.  Frame 1
    has a zero patch: amp 0, and wrapped 0 wherever the reference's real part is positive (NumPy's own angle of (0 + 0j) * conj(cref) is pi
    where both parts of cref are negative: asserted to be the same).  Where cref = -field exactly, wrapped is float32(pi) or its negative."""
    rng = np.random.default_rng(50 + ref_stride_frames)
    B, h, w, ph, pw = 2, 17, 65, 7, 7
    P = h * w
    pt = rand_tables(rng, (B, ph, pw))
    pt[1] = 0
    Gx, Gy = rand_tables(rng, (pw, w)), rand_tables(rng, (h, ph))
    first = run_inverse(pkg, pt.reshape(B, -1), Gx, Gy, False, B, h, w, ph, pw)
    nref = B if ref_stride_frames else 1
    cref = rng.standard_normal((nref, h, w)) + 1j * rng.standard_normal((nref, h, w))
    cref[-1] = np.abs(cref[-1].real) + 1j * cref[-1].imag            # the reference of the zero frame (the shared one): positive real part ...
    neg = np.zeros((h, w), bool)
    neg[3, :9] = True
    cref[-1][neg] = -1.5 - 0.5j                                        # ... but for nine pixels with both parts negative
    opposite = np.zeros((h, w), bool)
    opposite[5:8, 10:50] = True
    opposite &= ~neg
    cref[0][opposite] = -first["field"][0][opposite]                  # exactly opposite to the field the kernel itself produced
    amp_ref = rng.uniform(0, 3, (nref, h, w)).astype(np.float32)
    out = run_inverse(pkg, pt.reshape(B, -1), Gx, Gy, False, B, h, w, ph, pw, want_field=True, cref=cref, amp_ref=amp_ref, ref_stride=P * ref_stride_frames)
    assert np.array_equal(out["field"].view(np.uint64), first["field"].view(np.uint64)) and np.array_equal(out["amp"].view(np.uint32), first["amp"].view(np.uint32))
    qs, fs = inverse_ref(pt, Gx, Gy)
    print("reference field, stride %d" % (P * ref_stride_frames))
    check_inverse_outputs("with cref", out, qs, fs, B)
    for b in range(B):
        c, ar = cref[b if ref_stride_frames else 0], amp_ref[b if ref_stride_frames else 0]
        fr, fi, bre, bim = fs[b]
        amp, bamp = amp_bound(fr, fi, bre, bim)
        lo, hi = R.f32_interval(amp, bamp)
        plo, phi = ar * lo, ar * hi                                    # float32 products; amp_ref >= 0
        assert ((out["prod"][b] >= plo) & (out["prod"][b] <= phi)).all(), "prod"
        assert np.array_equal(out["prod"][b].view(np.uint32), (ar * out["amp"][b]).view(np.uint32))
        if b == 1:
            assert (out["amp"][b] == 0).all()
            want = np.angle(np.zeros((h, w), np.complex128) * np.conj(c)).astype(np.float32)
            assert (want[c.real > 0] == 0).all() and (want[neg] == np.float32(np.pi)).all() and (c.real > 0).sum() > P // 2
            assert np.array_equal(out["wrapped"][b], want)
            continue
        # r = field * conj(cref) in longdouble, its parts within (brr, bri) in float64: the propagated field bound plus the three roundings of
        # each part; the angle then within |dr| / |r| + 4 * 2^-53 |angle| (atan2 to two ulp), and float32 of that on the circle
        cr, ci = c.real.astype(LD), c.imag.astype(LD)
        rr, ri = fr * cr + fi * ci, fi * cr - fr * ci
        brr = bre * np.abs(cr) + bim * np.abs(ci) + 3 * R.U53 * (np.abs(fr * cr) + np.abs(fi * ci))
        bri = bim * np.abs(cr) + bre * np.abs(ci) + 3 * R.U53 * (np.abs(fi * cr) + np.abs(fr * ci))
        ang = np.arctan2(ri, rr)
        bang = np.sqrt(brr * brr + bri * bri) / np.sqrt(rr * rr + ri * ri) + 4 * R.U53 * np.abs(ang)
        got = out["wrapped"][b]
        ok = np.zeros((h, w), bool)
        for turn in (-1, 0, 1):
            lo, hi = R.f32_interval(ang + turn * 2 * LD(np.pi), bang)
            ok |= (got >= lo) & (got <= hi)
        on = ~opposite
        print("  wrapped: %d pixels, largest angle bound %.3g, %d wrong" % (int(on.sum()), float(bang[on].max()), int((~ok & on).sum())))
        assert float(bang[on].max()) < 1e-9 and ok[on].all()
        assert (np.abs(got[opposite]) == np.float32(np.pi)).all() and opposite.sum() == 120


# =======================================================================================================================================
# full spectrum

@pytest.mark.parametrize("Hf,Wf", [(24, 24), (25, 27), (40, 128), (33, 130)])
@pytest.mark.parametrize("pad", [0, 4])
def test_full_spectrum_magnitude(pkg, Hf, Wf, pad):
    """tables from launch_build_full_tables, then launch_dft_full_mag: even and odd sizes (the mirror column of fx = Wf / 2 exists only for even
    Wf), Wh = 13, 14, 65, 66 computed columns; against |fftshift(fft2(pad_reflect(plane)))| of the longdouble DFT; every element written"""
    rng = np.random.default_rng(Hf * Wf + pad)
    B, h, w, Wh = 2, Hf - 2 * pad, Wf - 2 * pad, Wf // 2 + 1
    planes = rng.standard_normal((B, h, w)).astype(np.float32)
    Exf, Eyf = _full((w, Wh), torch.complex128), _full((Hf, h), torch.complex128)
    pkg._lib.check(pkg._lib.load().vistaf_ftp_test_build_full_tables(_ptr(Exf), _ptr(Eyf), h, w, pad, Hf, Wf, None))
    refs = [R.full_mag_ref(planes[b], pad) for b in range(B)]
    ex, ey = refs[0][2:]
    print("full spectrum %dx%d pad %d" % (Hf, Wf, pad))
    r = [_ratio("Exf", Exf.cpu().numpy(), ex[:2], ex[2], ex[2]), _ratio("Eyf", Eyf.cpu().numpy(), ey[:2], ey[2], ey[2])]
    T, mag = run_full_mag(pkg, planes, Exf.cpu().numpy(), Eyf.cpu().numpy(), Hf, Wf)
    assert (T[B * h:] == SC).all() and (mag >= 0).all(), "an element of mag kept its sentinel"
    for b in range(B):
        r.append(_ratio("mag[%d]" % b, mag[b], refs[b][0], refs[b][1]))
    assert max(r) <= 1.0, r


# =======================================================================================================================================
# tables

def table_geoms(Hf, Wf):
    """(x0, y0, ph, pw, dpx, dpy, keep_carrier): an interior patch with a sub-bin remainder, patches clipped at x0 = 0, x1 = Wf and y1 = Hf, zero
    and +-0.5 remainders, re-centred and in place"""
    return [(1, 0, min(7, Hf), min(7, Wf - 1), 0.3, -0.2, 0), (0, Hf - 5, 5, 5, 0.0, 0.0, 0), (Wf - 4, 1, 6, 4, 0.5, -0.5, 1), (2, 2, 3, 4, -0.5, 0.5, 0),
            (1, 0, min(7, Hf), min(7, Wf - 1), 0.0, 0.0, 1)]


@pytest.mark.parametrize("h,w,pad", [(8, 8, 0), (9, 12, 3), (8, 10, 20), (24, 31, 16)])
@pytest.mark.parametrize("pair", [0, 1])
def test_twiddle_tables(pkg, h, w, pad, pair):
    """pad 0, pad < w, pad > w (a source pixel is met five times), Hf != Wf; packed tables (entries of a frame's slot beyond its own extent
    untouched, `win` untouched) and the pair layout of pmax = 9 > ph, pw (exact zeros beyond, win = hann(ph) x hann(pw) bit for bit)"""
    Hf, Wf, pmax = h + 2 * pad, w + 2 * pad, 9
    geoms = table_geoms(Hf, Wf)
    B = len(geoms)
    gd, gi = np.zeros((B, 7)), np.zeros((B, 10), np.int32)
    for b, (x0, y0, ph, pw, dpx, dpy, keep) in enumerate(geoms):
        assert x0 + pw <= Wf and y0 + ph <= Hf and ph <= pmax and pw <= pmax
        gd[b, 4:6], gi[b, :4], gi[b, 9] = (dpx, dpy), (x0, y0, ph, pw), keep
    Ex, Gx = _full((B, w * pmax), torch.complex128), _full((B, w * pmax), torch.complex128)
    Ey, Gy = _full((B, h * pmax), torch.complex128), _full((B, h * pmax), torch.complex128)
    win = _full((B, pmax, pmax), torch.float32)
    rc = pkg._lib.load().vistaf_ftp_test_build_tables(gd.ctypes.data_as(ctypes.c_void_p), gi.ctypes.data_as(ctypes.c_void_p), 1, B, h, w, pad, Hf, Wf, pmax, pair,
                                                      _ptr(Ex), _ptr(Ey), _ptr(Gx), _ptr(Gy), _ptr(win), None)
    pkg._lib.check(rc)
    Ex, Ey, Gx, Gy, win = (t.cpu().numpy() for t in (Ex, Ey, Gx, Gy, win))
    print("tables h=%d w=%d pad=%d %s" % (h, w, pad, "pair layout" if pair else "packed"))
    worst = 0.0
    for b, (x0, y0, ph, pw, dpx, dpy, keep) in enumerate(geoms):
        lh, lw = (pmax, pmax) if pair else (ph, pw)
        exr, exi, bex = R.table_forward_ref(w, pad, x0, pw, layout=lw)
        eyr, eyi, bey = R.table_forward_ref(h, pad, y0, ph, layout=lh)
        gxr, gxi, bgx = R.table_inverse_ref(w, pad, x0, pw, dpx, keep, 1.0, layout=lw)
        gyr, gyi, bgy = R.table_inverse_ref(h, pad, y0, ph, dpy, keep, 1.0 / (float(Hf) * float(Wf)), layout=lh)
        for name, got, n, ref in (("Ex", Ex[b], w * lw, (exr, exi, bex)), ("Ey", Ey[b], lh * h, (eyr.T, eyi.T, bey.T)),
                                  ("Gx", Gx[b], lw * w, (gxr, gxi, bgx)), ("Gy", Gy[b], h * lh, (gyr.T, gyi.T, bgy.T))):
            assert (got[n:] == SC).all(), (name, "written beyond the frame's tables")
            g = got[:n].reshape(ref[0].shape)
            worst = max(worst, _ratio("%s[%d]" % (name, b), g, ref[:2], ref[2], ref[2]))
            if pair:                                    # beyond the sample's own bins: exact zeros
                beyond = np.ones(ref[0].shape, bool)
                {"Ex": beyond[:, :pw], "Ey": beyond[:ph, :], "Gx": beyond[:pw, :], "Gy": beyond[:, :ph]}[name][...] = False
                assert beyond.any() and (g[beyond] == 0).all(), name
        if pair:
            want = np.zeros((pmax, pmax), np.float32)
            want[:ph, :pw] = O.hann_patch_window(ph, pw)
            assert np.array_equal(win[b].view(np.uint32), want.view(np.uint32)), "win"
        else:
            assert (win[b] == np.float32(S)).all()
    assert worst <= 1.0, worst


# =======================================================================================================================================
# peak search

def run_top_peaks(pkg, mag, dc, npeaks):
    B, Hf, Wf = mag.shape
    out = torch.full((B, 192), S, dtype=torch.float64, device="cuda")
    d = _dev(mag)
    pkg._lib.check(pkg._lib.load().vistaf_ftp_test_top_peaks(_ptr(d), B, Hf, Wf, dc, npeaks, _ptr(out), None))
    return out.cpu().numpy()


@pytest.mark.parametrize("case", D.peak_cases(), ids=lambda c: c.name)
def test_top_peaks(pkg, case):
    """positions and values exactly, in the kernel's written order (descending, equal values by ascending linear index: where the values are
    distinct that is O.find_top_peaks, asserted on the CPU by tests/test_kernel_refs.py); nothing written behind the list"""
    out = run_top_peaks(pkg, case.mag, case.dc, case.npeaks)
    for b, mag in enumerate(case.mag):
        want = R.top_peaks_rule(mag, case.dc, case.npeaks)
        got = [(int(x), int(y), float(v)) for x, y, v in out[b, :3 * case.npeaks].reshape(-1, 3)]
        if case.distinct:
            assert want == O.find_top_peaks(mag, case.dc, case.npeaks)
        first = next((i for i in range(case.npeaks) if got[i] != want[i]), None)
        print("%s[%d]: %d peaks, first difference at %s" % (case.name, b, case.npeaks, first))
        assert got == want, (case.name, b, first, got[first], want[first])
        assert (out[b, 3 * case.npeaks:] == S).all()


# =======================================================================================================================================
# carrier choice

def run_carrier(pkg, peaks_lists, mags, bw, frac):
    """one frame per list (all of one length) -> (gd [B][7], gi [B][10])"""
    B, npk = len(peaks_lists), len(peaks_lists[0])
    pk = np.full((B, 192), S)
    for b, lst in enumerate(peaks_lists):
        assert len(lst) == npk
        pk[b, :3 * npk] = np.array(lst, np.float64).ravel()
    mag = np.stack(mags)
    gd, gi = np.full((B, 7), S), np.full((B, 10), int(S), np.int32)
    d = [_dev(pk), _dev(mag)]
    rc = pkg._lib.load().vistaf_ftp_test_carrier_choose(_ptr(d[0]), npk, _ptr(d[1]), mag.shape[1], mag.shape[2], bw, frac, gd.ctypes.data_as(ctypes.c_void_p),
                                                        gi.ctypes.data_as(ctypes.c_void_p), B, None)
    pkg._lib.check(rc)
    return gd, gi


def assert_geom(name, gd, gi, case):
    wd, wi, (bx, by) = R.carrier_ref(case.peaks, case.mag, case.bw, case.frac)
    assert gi.tolist() == wi.tolist(), (name, gi.tolist(), wi.tolist())
    if case.exact_half:
        bx = by = 0.0                                                  # log(1.0) is exact: so is the half
    # period = Wf / |kx|: the bound of kx through the derivative, and the division's own rounding
    bp = case.mag.shape[1] / wd[2] ** 2 * bx + 2 * 2.0 ** -53 * wd[6] if wd[6] else 0.0
    bounds = [bx, by, bx, by, bx if wd[4] or wd[5] else 0.0, by if wd[4] or wd[5] else 0.0, bp]
    err = np.abs(gd - wd)
    print("%-40s err %s bounds %s" % (name, ["%.2g" % e for e in err], ["%.2g" % b for b in bounds]))
    assert (err <= np.array(bounds)).all(), (name, err, bounds)
    return max((e / b for e, b in zip(err, bounds) if b > 0), default=0.0)


def test_carrier_choice(pkg):
    """every hand-built list of tests/dft_cases.py: integer fields and ok exact, the refined peak and what derives from it within the bound of
    kernel_refs.carrier_ref; the four one-peak border lists once more as one batch"""
    cases = D.carrier_cases()
    worst = 0.0
    for c in cases:
        gd, gi = run_carrier(pkg, [c.peaks], [c.mag], c.bw, c.frac)
        worst = max(worst, assert_geom(c.name, gd[0], gi[0], c))
    batch = [c for c in cases if len(c.peaks) == 1]
    assert len(batch) >= 10
    gd, gi = run_carrier(pkg, [c.peaks for c in batch], [c.mag for c in batch], 3, 0.12)
    for b, c in enumerate(batch):
        assert_geom("batch:" + c.name, gd[b], gi[b], c)
    print("carrier: largest err / bound %.3f" % worst)


# =======================================================================================================================================
# hooks refuse what they cannot run

def test_hooks_refuse_bad_arguments(pkg):
    lib = pkg._lib.load()
    z = torch.zeros(4096, dtype=torch.float64, device="cuda")
    p = _ptr(z)
    gd, gi = np.zeros((1, 7)), np.zeros((1, 10), np.int32)
    hd, hi = gd.ctypes.data_as(ctypes.c_void_p), gi.ctypes.data_as(ctypes.c_void_p)
    calls = [lib.vistaf_ftp_test_top_peaks(None, 1, 8, 8, 0, 4, p, None), lib.vistaf_ftp_test_top_peaks(p, 1, 8, 8, 0, 65, p, None),
             lib.vistaf_ftp_test_top_peaks(p, 1, 2, 2, 0, 5, p, None), lib.vistaf_ftp_test_top_peaks(p, 0, 8, 8, 0, 4, p, None),
             lib.vistaf_ftp_test_carrier_choose(p, 0, p, 8, 8, 3, 0.12, hd, hi, 1, None), lib.vistaf_ftp_test_carrier_choose(p, 1, p, 8, 8, 3, 0.12, None, hi, 1, None),
             lib.vistaf_ftp_test_build_tables(hd, hi, 2, 1, 8, 8, 0, 8, 8, 7, 0, p, p, p, p, None, None),
             lib.vistaf_ftp_test_build_tables(hd, hi, 1, 1, 8, 8, 1, 8, 8, 7, 0, p, p, p, p, None, None),
             lib.vistaf_ftp_test_build_tables(hd, hi, 1, 1, 8, 8, 0, 8, 8, 7, 1, p, p, p, p, None, None),
             lib.vistaf_ftp_test_build_full_tables(p, p, 8, 8, 2, 12, 11, None),
             lib.vistaf_ftp_test_dft_forward(p, None, p, p, 0, 8, p, 0, p, p, 4, 1, 4, 4, 2, 2, None),
             lib.vistaf_ftp_test_dft_forward(p, None, p, p, 0, 0, p, 0, p, p, 3, 1, 4, 4, 2, 2, None),
             lib.vistaf_ftp_test_dft_inverse(p, 4, p, p, 0, 0, p, None, None, None, None, 0, None, None, None, 1, 4, 4, 2, 2, None),
             lib.vistaf_ftp_test_dft_inverse(p, 4, p, p, 0, 0, p, None, p, p, None, 0, p, p, None, 1, 4, 4, 2, 2, None),
             lib.vistaf_ftp_test_dft_inverse(p, 4, p, p, 0, 0, p, None, p, p, p, 3, p, p, None, 1, 4, 4, 2, 2, None)]
    assert calls == [-1] * len(calls), calls
    pk = torch.zeros(192, dtype=torch.float64, device="cuda")
    pk[0] = 8.0                                                         # x = Wf: outside the plane
    assert lib.vistaf_ftp_test_carrier_choose(_ptr(pk), 1, p, 8, 8, 3, 0.12, hd, hi, 1, None) == -1
    assert (z == 0).all()


# =======================================================================================================================================
# end to end in kernels: tables -> forward -> inverse, the carrier from the peak search and the choice

def _two_carriers(h, w):
    yy, xx = np.indices((h, w))
    return np.clip(128 + 50 * np.cos(2 * np.pi * (xx / 4.7 + yy / 31.0)) + 50 * np.cos(2 * np.pi * (xx / 7.9 - yy / 3.1)), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("h,w,pad,bw", [(24, 31, 16, 3), (40, 40, 0, 16)])
@pytest.mark.parametrize("image", ["white_noise", "two_carriers"])
def test_demodulation_end_to_end_in_kernels(pkg, h, w, pad, bw, image):
    """full tables -> magnitude -> peaks -> carrier -> tables -> forward -> inverse on the float32 plane the oracle itself transforms
    (O.ftp_complex_demod in complex128): the geometry exact, the refined peak within its bound, the field within the composed bound of the
    longdouble chain of reference tables, and within 1e-12 of the oracle's (what the references themselves agree to)"""
    rng = np.random.default_rng(h + pad)
    img = rng.integers(0, 256, (h, w)).astype(np.uint8) if image == "white_noise" else _two_carriers(h, w)
    cfg = O.OracleConfig(bad_pixel_enable=False, illum_sigma_px=3.0, pre_blur_sigma_px=0.0, fft_pad_px=pad, patch_half_width_bins=bw, dc_exclusion=2, n_fft_peaks=12)
    o = O.ftp_complex_demod(img, np.ones((h, w), np.float32), cfg)
    iw = np.ascontiguousarray(o["inter"]["iw"], np.float32)[None]
    Hf, Wf = o["fft_shape"]
    lib = pkg._lib.load()
    Wh = Wf // 2 + 1
    Exf, Eyf = _full((w, Wh), torch.complex128), _full((Hf, h), torch.complex128)
    pkg._lib.check(lib.vistaf_ftp_test_build_full_tables(_ptr(Exf), _ptr(Eyf), h, w, pad, Hf, Wf, None))
    _, mag = run_full_mag(pkg, iw, Exf.cpu().numpy(), Eyf.cpu().numpy(), Hf, Wf)
    peaks = run_top_peaks(pkg, mag, cfg.dc_exclusion, cfg.n_fft_peaks)
    padded = cvlite.pad_reflect(iw[0], pad) if pad else iw[0]
    omag = np.abs(np.fft.fftshift(np.fft.fft2(padded.astype(np.float64))))
    opeaks = O.find_top_peaks(omag, cfg.dc_exclusion, cfg.n_fft_peaks)
    got_pk = [(int(x), int(y)) for x, y, _ in peaks[0, :36].reshape(-1, 3)]
    # the oracle's list is only an order where its values are further apart than the two spectra differ
    vals = np.array([v for _, _, v in opeaks])
    if (np.abs(np.diff(vals)) > 1e-9 * vals.max()).all():
        assert got_pk == [(x, y) for x, y, _ in opeaks]
    wd, wi, (bx, by) = R.carrier_ref(opeaks, omag, bw, cfg.peak_max_dy_from_center)
    assert wd[:2].tolist() == list(o["peak_refined"])
    lmag, bmag, _, _ = R.full_mag_ref(iw[0], pad)
    assert _ratio("mag", mag[0], lmag, bmag) <= 1.0
    # the kernel refines on its own magnitudes: their relative bound at the five points is a further error of the logarithms
    px, py = int(wi[6]), int(wi[7])
    pts = [(py, px), (py, max(px - 1, 0)), (py, min(px + 1, Wf - 1)), (max(py - 1, 0), px), (min(py + 1, Hf - 1), px)]
    log_err = max(float(bmag[p] / lmag[p]) for p in pts) * 1.01 + 2.0 ** -52
    _, _, (bx2, by2) = R.carrier_ref(opeaks, omag, bw, cfg.peak_max_dy_from_center, log_err=log_err)
    for v, b in ((wd[0], bx), (wd[1], by)):                            # the case is not within its bound of a rounding boundary
        assert abs(abs(v - np.floor(v)) - 0.5) > 1e-9 + 10 * b and abs(abs(v - np.round(v)) - 1e-6) > 1e-9 + 10 * b
    dm, dp = _dev(mag), _dev(peaks)
    gd, gi = np.full((1, 7), S), np.full((1, 10), int(S), np.int32)
    pkg._lib.check(lib.vistaf_ftp_test_carrier_choose(_ptr(dp), cfg.n_fft_peaks, _ptr(dm), Hf, Wf, bw, cfg.peak_max_dy_from_center,
                                                      gd.ctypes.data_as(ctypes.c_void_p), gi.ctypes.data_as(ctypes.c_void_p), 1, None))
    print("e2e %s h=%d w=%d pad=%d bw=%d: peak %s, patch %s" % (image, h, w, pad, bw, gd[0, :2], gi[0, :4]))
    assert gi[0].tolist() == wi.tolist(), (gi, wi)
    print("  refined peak: err (%.3g, %.3g), bound (%.3g, %.3g)" % (abs(gd[0, 0] - wd[0]), abs(gd[0, 1] - wd[1]), bx2, by2))
    assert abs(gd[0, 0] - wd[0]) <= bx2 and abs(gd[0, 1] - wd[1]) <= by2, (gd, wd, bx2, by2)
    # and on the kernel's own spectrum and list, the bound of the choice alone
    kd, ki, (kbx, kby) = R.carrier_ref([(int(x), int(y), float(v)) for x, y, v in peaks[0, :36].reshape(-1, 3)], mag[0], bw, cfg.peak_max_dy_from_center)
    assert ki.tolist() == gi[0].tolist() and abs(gd[0, 0] - kd[0]) <= kbx and abs(gd[0, 1] - kd[1]) <= kby
    x0, y0, ph, pw = (int(v) for v in gi[0, :4])
    pmax = 2 * bw + 1
    Ex, Gx = _full((w * pmax,), torch.complex128), _full((w * pmax,), torch.complex128)
    Ey, Gy = _full((h * pmax,), torch.complex128), _full((h * pmax,), torch.complex128)
    pkg._lib.check(lib.vistaf_ftp_test_build_tables(gd.ctypes.data_as(ctypes.c_void_p), gi.ctypes.data_as(ctypes.c_void_p), 0, 1, h, w, pad, Hf, Wf, pmax, 0,
                                                    _ptr(Ex), _ptr(Ey), _ptr(Gx), _ptr(Gy), None, None))
    win = O.hann_patch_window(ph, pw)
    Exn, Eyn = Ex.cpu().numpy()[:w * pw].reshape(w, pw), Ey.cpu().numpy()[:ph * h].reshape(ph, h)
    Gxn, Gyn = Gx.cpu().numpy()[:pw * w].reshape(pw, w), Gy.cpu().numpy()[:h * ph].reshape(h, ph)
    T, patch = run_forward(pkg, iw, None, Exn, Eyn, win, False, ph, pw)
    out = run_inverse(pkg, patch, Gxn, Gyn, False, 1, h, w, ph, pw)
    # the longdouble chain on reference tables built from the KERNEL's geometry (its dpx, dpy: the reference's within the bound above)
    ex = R.table_forward_ref(w, pad, x0, pw)
    ey = R.table_forward_ref(h, pad, y0, ph)
    gx = R.table_inverse_ref(w, pad, x0, pw, gd[0, 4], 0, 1.0)
    gy = R.table_inverse_ref(h, pad, y0, ph, gd[0, 5], 0, 1.0 / (float(Hf) * float(Wf)))
    ch = R.demod_chain(iw[0].astype(LD), ex, (ey[0].T, ey[1].T, ey[2].T), win, gx, (gy[0].T, gy[1].T, gy[2].T))
    r = [_ratio("T", T[:h], ch["T"][:2], *ch["T"][2:]), _ratio("patch", patch[0, :ph * pw].reshape(ph, pw), ch["patch"][:2], *ch["patch"][2:]),
         _ratio("Q", out["Q"][0], ch["Q"][:2], *ch["Q"][2:]), _ratio("field", out["field"][0], ch["field"][:2], *ch["field"][2:])]
    assert max(r) <= 1.0, r
    _assert_f32("amp", out["amp"][0], *amp_bound(*ch["field"]))
    rel = float(np.abs(out["field"][0] - o["field"]).max() / np.abs(o["field"]).max())
    print("  field vs O.ftp_complex_demod: %.3g of max |field|" % rel)
    assert rel <= 1e-12
