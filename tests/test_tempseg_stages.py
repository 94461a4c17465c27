"""The periodic-stripe segmentation (csrc/tempseg.hip, vistaf_tempseg_segment) checked stage by stage: every plane the session leaves behind is
read with vistaf_ftp_test_tempseg_plane (csrc/test_hooks.h) and held against the stage function of tests/tempseg_cases.py applied to the device's
OWN upstream plane, so that errors do not compound and most stages are held exactly.  A CPU test runs the same stage functions on the oracle's
planes and finds the oracle's masks and numbers again, which makes the staged reference the oracle itself.  Beyond the stages every case is
compared end to end with the oracle at "at most 8 pixels per mask": that allowance is where the float32 spectrum of the carrier search and the
last bit of the normalising mean (include/vistaf_temp.h) are absorbed, and nowhere else.

The one bound that is measured rather than derived: the magnitude plane of the carrier search comes from hipFFT's float32 transform, a library
the project does not control.  Against |fftshift(fft2(float64(inorm)))| of the device's own inorm, relative to the plane's maximum, the largest
deviation over all cases below on the MI355X is MAG_MEASURED = 1.42e-7 (272 x 1009, narrow dark stripes; the other cases 3.2e-8 .. 1.06e-7);
MAG_ALLOWED is four times that, 5.68e-7, the factor covering the dependence of a library transform on shape and content.  Every other bound
is computed by the test from the reference (tests/tempseg_cases.py derives the one on z) or is equality."""
import ctypes
import dataclasses

import numpy as np
import pytest

import kernel_refs as R
import tempseg_cases as TC
from oracle import temp_oracle as T

MAG_MEASURED = 1.42e-7          # c9_272x1009_narrow_dark; the other cases 3.2e-8 .. 1.06e-7
MAG_ALLOWED = 4 * MAG_MEASURED

E_INVALID, E_STATE, E_NOCARRIER = -1, -3, -4
NAMES = [c.name for c in TC.CASES]


# =======================================================================================================================================
# CPU: the staged reference is the oracle

@pytest.mark.parametrize("name", NAMES)
def test_staged_reference_reproduces_the_oracle(name):
    c = TC.BY_NAME[name]
    cfg = c.config(T.TempSegConfig)
    img, roi, dark, light, pack = TC.oracle_run(name)
    dbg = pack["dbg"]
    gray = TC.ref_gray(img)
    sat0, sat, roi_eff = TC.ref_sat(gray, roi, cfg)
    assert np.array_equal(sat, pack["sat"]) and np.array_equal(roi_eff, pack["roi_eff"]) and sat0.any()
    g = TC.ref_g(gray, roi, TC.ref_med(gray, roi_eff))
    blur, norm = TC.ref_norm(g, cfg.seg_illum_sigma)
    cands = TC.ref_inorm_candidates(norm, roi_eff)
    # the oracle's mu is NumPy's float32 pairwise mean: within log2(n) float32 roundings of the float64 mean the candidates are built around
    mu_o = np.float32(np.mean(norm[roi_eff]))
    assert abs(float(mu_o) - float(cands[0][0])) <= 32 * 2.0 ** -24 * float(mu_o)
    assert _bits_equal(pack["i_norm"], (norm / mu_o).astype(np.float32))
    inorm = pack["i_norm"]
    F = TC.ref_spectrum(inorm)
    assert np.array_equal(np.abs(F), pack["fft_mag"])
    peaks = TC.ref_peaks(pack["fft_mag"], cfg)
    px, py, angle, period = TC.ref_carrier(peaks, c.h, c.w, cfg)
    assert (px, py) == tuple(pack["peak"]) == (dbg["peak_x"], dbg["peak_y"]) and angle == dbg["carrier_angle_rad"]
    assert period == dbg["carrier_period_px"] or (np.isnan(period) and np.isnan(dbg["carrier_period_px"]))
    R_ = cfg.seg_band_radius
    assert R_ <= px < c.w - R_ and R_ <= py < c.h - R_, "the band leaves the spectrum"
    z = TC.ref_bandpass(F, (px, py), R_)
    assert np.array_equal(z, pack["z"])
    phi0, cc, _ = TC.ref_phi0(z, inorm, roi_eff)
    assert phi0 == dbg["phi0_rad"]
    mask_a = TC.ref_mask_a(z, phi0, roi_eff)
    assert np.array_equal(TC.ref_signal(z, phi0).astype(np.float32), pack["signal"])
    (sa, na), (sb, nb), mean_a, mean_b, a_dark = TC.ref_sides(gray, mask_a, roi_eff)
    # the oracle's means are float32 quotients of the same exact sums (np.mean of a float32 array); the order of the two is the same
    assert sa < 2 ** 24 and sb < 2 ** 24
    for mean, s, n, key in ((mean_a, sa, na, "mean_gray_A"), (mean_b, sb, nb, "mean_gray_B")):
        assert dbg[key] == (float(np.float32(s) / np.float32(n)) if n else 1e9) and (n == 0 or abs(dbg[key] - mean) <= 2.0 ** -24 * mean)
    assert ("A_is_dark" if a_dark else "B_is_dark") == dbg["chosen"] == c.chosen
    raw, d, l = TC.ref_final(mask_a, a_dark, roi_eff, cfg)
    assert np.array_equal(raw, pack["raw_dark"]) and np.array_equal(d, dark) and np.array_equal(l, light)
    assert (int(roi.sum()), int(roi_eff.sum()), int(sat.sum()), int(d.sum()), int(l.sum())) == tuple(
        dbg[k] for k in ("roi_pixels", "roi_eff_pixels", "sat_pixels", "dark_pixels", "light_pixels"))
    # the reference alone leaves no pixel out of the sign comparison
    bz = TC.bound_z(inorm, F, (px, py), R_)
    assert int((np.abs(TC.ref_signal(z, phi0))[roi_eff] <= 2 * bz).sum()) == 0
    if name == "c8_tie":
        assert cc == 0 and phi0 == 0.0 and mean_a == mean_b == 100.0 and na > 0 and nb > 0
    if name == "c8_tie_dc6_empty_b":
        assert nb == 0 and mean_b == 1e9
    if name == "c1_even_sizes":
        o = TC.oracle_run("c1_64x64_bits")
        assert np.array_equal(dark, o[2]) and np.array_equal(light, o[3])
    if name == "c6_80x3329_one_peak":
        assert len(peaks) == 1 and np.array_equal(raw, d)


# =======================================================================================================================================
# GPU

PLANES = {"gray": np.float32, "g": np.float32, "blur": np.float32, "norm": np.float32, "inorm": np.float32, "sat0": np.uint8, "mask_a": np.uint8,
          "mag": np.float64, "z": np.complex128}


def read_plane(pkg, seg, name):
    import torch
    if name in PLANES:
        t = torch.zeros((seg.H, seg.W), dtype=getattr(torch, np.dtype(PLANES[name]).name), device="cuda")
    elif name == "peaks":
        t = torch.zeros(192, dtype=torch.float64, device="cuda")
    elif name == "med":
        t = torch.zeros(1, dtype=torch.float32, device="cuda")
    else:
        t = torch.zeros(96, dtype=torch.uint8, device="cuda")
    pkg._lib.check(pkg._lib.load().vistaf_ftp_test_tempseg_plane(seg._h, name.encode(), ctypes.c_void_p(t.data_ptr()), t.numel() * t.element_size(), None))
    a = t.cpu().numpy()
    if name == "geom":
        return a[:56].view(np.float64).copy(), a[56:].view(np.int32).copy()
    return a


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


_MAG_SEEN = {}


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_every_stage_from_the_device_own_upstream_plane(pkg, name):
    c = TC.BY_NAME[name]
    cfg = c.config(T.TempSegConfig)
    img, roi = c.image()
    h, w, R_ = c.h, c.w, cfg.seg_band_radius
    seg = pkg.TempSegmenter(h, w, c.config(pkg.tempseg.TempSegConfig))
    dark, light, pack = seg.segment(img, roi)
    dbg = pack["dbg"]
    P = {k: read_plane(pkg, seg, k) for k in list(PLANES) + ["peaks", "med"] if not (k == "blur" and cfg.seg_illum_sigma <= 0)}
    gd, gi = read_plane(pkg, seg, "geom")
    seg.close()
    # ---- gray, saturation, effective ROI, median: exact
    gray = TC.ref_gray(img)
    sat0, sat, roi_eff = TC.ref_sat(gray, roi, cfg)
    assert np.array_equal(P["gray"], gray.astype(np.float32)) and np.array_equal(P["sat0"], sat0.astype(np.uint8))
    assert np.array_equal(pack["sat"], sat) and np.array_equal(pack["roi_eff"], roi_eff)
    med = TC.ref_med(gray, roi_eff)
    assert P["med"][0] == med
    # ---- fill, blur, normalisation: bit for bit from the device's own planes
    assert _bits_equal(P["g"], TC.ref_g(gray, roi, med))
    blur, norm = TC.ref_norm(P["g"], cfg.seg_illum_sigma)
    if blur is not None:
        assert _bits_equal(P["blur"], blur)
        assert _bits_equal(P["norm"], (P["g"] / np.where(P["blur"] < 1e-6, np.float32(1.0), P["blur"])).astype(np.float32))
    else:
        assert _bits_equal(P["norm"], P["g"])
    hits = [float(m) for m, v in TC.ref_inorm_candidates(P["norm"], roi_eff) if _bits_equal(P["inorm"], v)]
    print("%s: inorm is norm / mu for mu in %s" % (name, hits))
    assert hits, "inorm is norm / mu for none of the three candidates"
    # which of the three: the device forms the mean in float64 and rounds it once, so mu is the float32 rounding of the exact mean, a neighbour
    # only where the exact mean lies within the float64 summation error (n 2^-53 mean|norm|, any order) of a float32 rounding boundary
    sel = P["norm"][roi_eff].astype(R.LD)
    mean = sel.sum() / sel.size
    lo, hi = R.f32_interval(mean, sel.size * R.U53 * np.abs(sel).sum() / sel.size + 2 * R.U53 * abs(mean))
    assert any(lo <= np.float32(m) <= hi for m in hits), (hits, float(lo), float(hi))
    # ---- spectrum: the float32 transform against float64, the peak list exactly from the device's own magnitudes
    F = TC.ref_spectrum(P["inorm"])
    ref_mag = np.abs(F)
    dev = float(np.abs(P["mag"] - ref_mag).max() / ref_mag.max())
    _MAG_SEEN[name] = dev
    print("%s: float32 spectrum deviates by %.3g of the plane's maximum (largest so far %.3g, allowed %.3g)" % (name, dev, max(_MAG_SEEN.values()), MAG_ALLOWED))
    assert dev <= MAG_ALLOWED
    n = cfg.n_peaks
    got_peaks = [(int(x), int(y), float(v)) for x, y, v in P["peaks"][:3 * n].reshape(-1, 3)]
    # find_top_peaks with its order among equal values stated (a real frame's magnitudes come in equal Hermitian pairs, and NumPy leaves the
    # order inside a pair open): the same multiset as the oracle's list, in the kernel's documented order
    assert got_peaks == R.top_peaks_rule(P["mag"], int(cfg.seg_dc_exclusion), n)
    assert sorted(v for _, _, v in got_peaks) == sorted(v for _, _, v in TC.ref_peaks(P["mag"], cfg))
    # ---- carrier: the oracle's choice on the device's list, the oracle's formulas on that peak
    px, py, angle, period = TC.ref_carrier(got_peaks, h, w, cfg)
    assert (int(gi[6]), int(gi[7])) == (px, py) == (dbg["peak_x"], dbg["peak_y"]) == tuple(pack["peak"]) and gi[8] == 1
    assert (gi[0], gi[1], gi[2], gi[3], gi[9]) == (px - R_, py - R_, 2 * R_ + 1, 2 * R_ + 1, 1) and gd[4] == 0.0 and gd[5] == 0.0
    assert dbg["carrier_angle_rad"] == angle and dbg["carrier_period_px"] == period
    if name == "c6_80x3329_one_peak":
        assert px <= w // 2, "the single peak was meant to lie outside the right half-plane"
    # ---- band-pass: float64 against float64, within the composed bound
    z_ref = TC.ref_bandpass(F, (px, py), R_)
    bz = TC.bound_z(P["inorm"], F, (px, py), R_)
    ez = max(float(np.abs(P["z"].real - z_ref.real).max()), float(np.abs(P["z"].imag - z_ref.imag).max()))
    print("%s: z within %.3g of the reference, bound %.3g, max |z| %.3g" % (name, ez, bz, float(np.abs(z_ref).max())))
    assert ez <= bz
    # ---- rotation angle
    phi0_ref, cc, sabs = TC.ref_phi0(P["z"], P["inorm"], roi_eff)
    if cc == 0:
        assert dbg["phi0_rad"] == 0.0 and not np.signbit(dbg["phi0_rad"])
    else:
        bphi = h * w * TC.U * sabs / abs(cc)
        print("%s: phi0 %.17g, reference %.17g, bound %.3g" % (name, dbg["phi0_rad"], phi0_ref, bphi))
        assert abs(dbg["phi0_rad"] - phi0_ref) <= bphi
    # ---- sign mask: exact outside the pixels whose |Re| is within twice the bound on z
    s = TC.ref_signal(P["z"], dbg["phi0_rad"])
    near = (np.abs(s) <= 2 * bz) & roi_eff
    assert int((np.abs(TC.ref_signal(z_ref, phi0_ref)) <= 2 * bz)[roi_eff].sum()) == 0, "the reference itself leaves pixels out"
    assert int(near.sum()) <= 0.001 * int(roi_eff.sum())
    want_a = (s.astype(np.float32) >= 0) & roi_eff
    mask_a = P["mask_a"] != 0
    assert set(np.unique(P["mask_a"])) <= {0, 1} and not (mask_a & ~roi_eff).any()
    assert np.array_equal(mask_a[~near], want_a[~near]), int((mask_a != want_a)[~near].sum())
    # ---- side means and the choice: integer sums, so bit for bit from the device's own mask
    (sa, na), (sb, nb), mean_a, mean_b, a_dark = TC.ref_sides(gray, mask_a, roi_eff)
    assert dbg["mean_gray_A"] == mean_a and dbg["mean_gray_B"] == mean_b and (dbg["chosen"] == "A_is_dark") == a_dark
    print("%s: %s, means %r / %r, sides of %d / %d pixels" % (name, dbg["chosen"], mean_a, mean_b, na, nb))
    assert dbg["chosen"] == c.chosen
    if name.startswith("c8_tie"):
        assert mean_a == 100.0 and (mean_b == 1e9 and nb == 0 if name.endswith("empty_b") else mean_b == 100.0 and nb > 0)
    # ---- close / open and the counts: exactly the oracle's morphology on the device's own raw mask
    raw, d_ref, l_ref = TC.ref_final(mask_a, a_dark, roi_eff, cfg)
    assert np.array_equal(dark, d_ref) and np.array_equal(light, l_ref)
    assert (dbg["roi_pixels"], dbg["roi_eff_pixels"], dbg["sat_pixels"], dbg["dark_pixels"], dbg["light_pixels"]) == (
        int(roi.sum()), int(roi_eff.sum()), int(sat.sum()), int(d_ref.sum()), int(l_ref.sum()))
    # ---- end to end against the oracle
    _, _, dark_o, light_o, pack_o = TC.oracle_run(name)
    nd, nl = int((dark != dark_o).sum()), int((light != light_o).sum())
    print("%s: %d dark and %d light pixels differ from the oracle's" % (name, nd, nl))
    assert nd <= 8 and nl <= 8
    assert dbg["chosen"] == pack_o["dbg"]["chosen"]
    mirror = (2 * (w // 2) - pack_o["peak"][0], 2 * (h // 2) - pack_o["peak"][1])          # the other bin of the Hermitian pair: the same masks
    assert (px, py) == tuple(pack_o["peak"]) or (cfg.n_peaks == 1 and (px, py) == mirror)


# =======================================================================================================================================
# the sign split on planes of the caller: zeros, negative zeros and values that only become zero as float32

def test_sign_reference_counts_float32_zeros_as_a():
    """CPU: what the reference's float32 cast does to the sign: -0.0 and every |value| below half the smallest float32 denormal are >= 0"""
    s = np.array([0.0, -0.0, -1e-50, 1e-50, -7e-46, -8e-46, -1.0, 1.0])
    assert ((s.astype(np.float32) >= 0) == np.array([1, 1, 1, 1, 1, 0, 0, 1], bool)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("phi0", [0.0, 0.3, -2.0, float(np.pi)])
def test_sign_split_direct(pkg, phi0):
    """k_ts_sign through vistaf_ftp_test_tempseg_sign: more pixels than the grid has threads (and no multiple of the block), a field with exact
    zeros, negative zeros, values that round to a float32 zero, and whole rows off the ROI; mask and the four sums exactly"""
    import torch
    n = 1024 * 256 + 77
    rng = np.random.default_rng(int(abs(phi0) * 100) + 3)
    z = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    special = np.array([0.0, -0.0, 1e-50, -1e-50, -7e-46, -8e-46, 7e-46, 1e-300, -1e-300])
    k = rng.integers(0, n, 4000)
    z.real[k] = special[rng.integers(0, special.size, k.size)]
    z.imag[k[:2000]] = special[rng.integers(0, special.size, 2000)]
    roi = (rng.random(n) < 0.8).astype(np.uint8) * np.array([1, 2, 255], np.uint8)[rng.integers(0, 3, n)]
    roi[1000:3000] = 0
    gray = rng.integers(0, 256, n).astype(np.float32)
    # the real part as complex128 multiplication by exp(-i phi0) = (c, -s) forms it: re c - im (-s), each operation rounded on its own
    c0, s0 = np.cos(phi0), np.sin(phi0)
    sig = z.real * c0 - z.imag * (-s0)
    want = (roi != 0) & (sig.astype(np.float32) >= 0)
    zero32 = (sig.astype(np.float32) == 0) & (roi != 0)
    assert int(zero32.sum()) >= (100 if phi0 == 0.0 else 10), "the case holds too few float32 zeros to say anything"
    d = [torch.from_numpy(a).cuda() for a in (z, roi, gray)]
    out = torch.full((n + 64,), 7, dtype=torch.uint8, device="cuda")
    sums = (ctypes.c_double * 4)(-1, -1, -1, -1)
    pkg._lib.check(pkg._lib.load().vistaf_ftp_test_tempseg_sign(ctypes.c_void_p(d[0].data_ptr()), phi0, ctypes.c_void_p(d[1].data_ptr()),
                                                                ctypes.c_void_p(d[2].data_ptr()), ctypes.c_void_p(out.data_ptr()), sums, n, None))
    got = out.cpu().numpy()
    assert (got[n:] == 7).all() and set(np.unique(got[:n])) <= {0, 1}
    bad = np.flatnonzero((got[:n] != 0) != want)
    assert bad.size == 0, (bad.size, bad[:5], sig[bad[:5]], int(zero32[bad].sum()))
    b = (roi != 0) & ~want
    assert list(sums) == [float(gray[want].astype(np.float64).sum()), float(want.sum()), float(gray[b].astype(np.float64).sum()), float(b.sum())]


@pytest.mark.gpu
def test_sign_hook_refusals(pkg):
    import torch
    lib = pkg._lib.load()
    t = torch.zeros(64, dtype=torch.float64, device="cuda")
    p, sums = ctypes.c_void_p(t.data_ptr()), (ctypes.c_double * 4)()
    for args in ((None, 0.0, p, p, p, sums, 4), (p, 0.0, None, p, p, sums, 4), (p, 0.0, p, None, p, sums, 4), (p, 0.0, p, p, None, sums, 4),
                 (p, 0.0, p, p, p, None, 4), (p, 0.0, p, p, p, sums, 0), (p, float("nan"), p, p, p, sums, 4), (p, float("inf"), p, p, p, sums, 4)):
        assert lib.vistaf_ftp_test_tempseg_sign(*args, None) == E_INVALID, args[1:]


def _good():
    c = TC.BY_NAME["c1_64x64_bits"]
    img, roi = c.image()
    return c, img, roi


def _segment_bits(seg, img, roi):
    dark, light, pack = seg.segment(img, roi)
    return dark, light, pack["roi_eff"], pack["sat"], tuple(sorted(pack["dbg"].items()))


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4] == b[4]


@pytest.mark.gpu
def test_errors_leave_the_session_usable(pkg):
    """the three refusals of a frame, each followed by a good frame on the same session: the bits of a fresh session.  A session whose only call
    failed hands out no plane."""
    import torch
    lib = pkg._lib.load()
    c, img, roi = _good()
    gcfg = c.config(pkg.tempseg.TempSegConfig)
    fresh = pkg.TempSegmenter(64, 64, gcfg)
    want = _segment_bits(fresh, img, roi)
    fresh.close()
    _, xx = np.mgrid[0:64, 0:64]
    sat_all = np.full((64, 64, 3), 250, np.uint8)
    flat = np.full((64, 64, 3), 100, np.uint8)
    fine = np.clip(np.rint(120.0 + 60.0 * np.cos(2 * np.pi * xx / 2.5)), 0, 255).astype(np.uint8)
    fine = np.repeat(fine[..., None], 3, axis=2)
    ones = np.ones((64, 64), bool)
    wide = dataclasses.replace(gcfg, seg_band_radius=8)
    buf = torch.zeros((64, 64), dtype=torch.float32, device="cuda")

    def plane_rc(seg):
        return lib.vistaf_ftp_test_tempseg_plane(seg._h, b"gray", ctypes.c_void_p(buf.data_ptr()), 64 * 64 * 4, None)

    for what, frame, cfg_g, text in (("saturated", sat_all, gcfg, "ROI became empty"), ("flat", flat, gcfg, "Could not find FFT peaks"),
                                     ("fine", fine, wide, "carrier band leaves the spectrum")):
        if cfg_g is not gcfg:
            fresh = pkg.TempSegmenter(64, 64, cfg_g)
            want = _segment_bits(fresh, img, roi)
            fresh.close()
            o = T.segment_dark_light_gratings_periodic_fft(img, roi, dataclasses.replace(c.config(T.TempSegConfig), seg_band_radius=8))
            assert int((want[0] != o[0]).sum()) <= 8 and int((want[1] != o[1]).sum()) <= 8
        seg = pkg.TempSegmenter(64, 64, cfg_g)
        with pytest.raises(RuntimeError, match=text):
            seg.segment(frame, ones)
        assert plane_rc(seg) == E_STATE, what                  # the only call of this session failed: no plane to read
        assert _same(_segment_bits(seg, img, roi), want), what
        assert plane_rc(seg) == 0
        with pytest.raises(RuntimeError, match=text):
            seg.segment(frame, ones)
        assert plane_rc(seg) == E_STATE, what                  # nor after a failure that follows a good frame
        assert _same(_segment_bits(seg, img, roi), want), what
        seg.close()
    with pytest.raises(RuntimeError, match="ROI became empty"):                 # the oracle refuses the saturated ROI the same way
        T.segment_dark_light_gratings_periodic_fft(sat_all, ones, c.config(T.TempSegConfig))


@pytest.mark.gpu
def test_plane_hook_refusals(pkg):
    import torch
    lib = pkg._lib.load()
    c, img, roi = _good()
    seg = pkg.TempSegmenter(64, 64, c.config(pkg.tempseg.TempSegConfig))
    buf = torch.full((64 * 64 * 16 + 64,), 7, dtype=torch.uint8, device="cuda")
    p = ctypes.c_void_p(buf.data_ptr())
    assert lib.vistaf_ftp_test_tempseg_plane(seg._h, b"gray", p, 64 * 64 * 4, None) == E_STATE          # has not segmented yet
    seg.segment(img, roi)
    for args in ((None, b"gray", p, 64 * 64 * 4), (seg._h, None, p, 64 * 64 * 4), (seg._h, b"gray", None, 64 * 64 * 4), (seg._h, b"grey", p, 64 * 64 * 4),
                 (seg._h, b"", p, 0), (seg._h, b"gray", p, 64 * 64 * 4 - 1), (seg._h, b"gray", p, 64 * 64), (seg._h, b"mag", p, 64 * 64 * 4),
                 (seg._h, b"z", p, 64 * 64 * 8), (seg._h, b"peaks", p, 192 * 4), (seg._h, b"med", p, 8), (seg._h, b"geom", p, 104), (seg._h, b"sat0", p, 64 * 64 * 4)):
        assert lib.vistaf_ftp_test_tempseg_plane(*args, None) == E_INVALID, args[1:]
    assert bool((buf == 7).all())
    sizes = {"gray": 4, "g": 4, "blur": 4, "norm": 4, "inorm": 4, "sat0": 1, "mask_a": 1, "mag": 8, "z": 16}
    for k, b in sizes.items():
        buf.fill_(7)
        assert lib.vistaf_ftp_test_tempseg_plane(seg._h, k.encode(), p, 64 * 64 * b, None) == 0, k
        assert bool((buf[64 * 64 * b:] == 7).all()), k
    seg.close()
