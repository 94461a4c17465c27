"""CPU checks of the references in tests/kernel_refs.py: each is compared with an independent statement of the same operation, so that a
kernel test that fails points at the kernel."""
import numpy as np
import pytest

import dft_cases as D
import kernel_refs as R
from oracle import cvlite
from oracle import ftp_oracle as O


def test_keys_are_order_preserving_and_invertible():
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.standard_normal(1000).astype(np.float32) * np.float32(1e20), np.array([0.0, -0.0, 1e-45, -1e-45, 3e38, -3e38], np.float32)])
    k = R.f2key(x)
    assert (R.bits(R.key2f(k)) == R.bits(x)).all()
    order = np.argsort(k, kind="stable")
    assert (np.diff(x[order].astype(np.float64)) >= 0).all()
    assert R.f2key(np.float32(-0.0)) + 1 == R.f2key(np.float32(0.0))


@pytest.mark.parametrize("n", [1, 2, 3, 10, 1001, 4096])
def test_selection_reference_is_the_interpolated_order_statistic(n):
    """np.percentile's float32 result against the textbook definition in float64 on the sorted values"""
    rng = np.random.default_rng(n)
    v = rng.standard_normal(n).astype(np.float32)
    reqs = [0.0, 8.0, 25.0, 50.0, 92.0, 99.7, 99.9, 100.0, R.MEDIAN]
    out, cnt, nbrs = R.select_ref(v, np.ones(n, np.uint8), reqs)
    assert cnt == n
    s = np.sort(v.astype(np.float64))
    for j, q in enumerate(reqs):
        exact = np.median(s) if q is R.MEDIAN else np.percentile(s, q)
        k = nbrs[j][0]
        # NumPy forms the fractional rank n * q in float32: it is off by up to n * 2^-23 of a rank, times the local spacing of the values
        gap = s[min(k + 2, n - 1)] - s[max(k - 1, 0)]
        assert abs(float(out[j]) - exact) <= 4 * 2.0 ** -23 * max(1.0, np.abs(s).max()) + n * 2.0 ** -22 * gap, (n, q)
        assert s[k] <= exact + 1e-12 and (k + 1 >= n or exact <= s[k + 1] + 1e-12)


def test_the_kernels_index_and_interpolation_model_is_numpys_float32_percentile_bit_for_bit():
    """select.hpp's arithmetic, restated (kernel_refs.percentile_model), against np.percentile: equal bits at every size and request.  (The
    general Hyndman-Fan index n*q + (1 - q) - 1 in float32 is NOT: it differs from NumPy's (n - 1)*q in a third of these cases.)"""
    rng = np.random.default_rng(0)
    f, general_differs = np.float32, 0
    for n in (2, 3, 7, 100, 1023, 5759, 50176, 262143, 300001):
        v = rng.standard_normal(n).astype(f)
        s = np.sort(v)
        for q in (0.0, 1.0, 8.0, 25.0, 33.3, 50.0, 92.0, 95.0, 98.0, 99.7, 99.9, 100.0):
            exp = f(np.percentile(v, q))
            assert R.bits(R.percentile_model(s, q))[0] == R.bits(exp)[0], (n, q)
            q32 = R.request_value(q)
            general_differs += f(f(f(f(n) * q32) + f(f(1) + f(q32 * f(-1)))) - f(1)) != f(f(n - 1) * q32)
    assert general_differs > 0


def test_selection_reference_drops_masked_and_non_finite_and_applies_abs_then_threshold():
    v = np.array([np.nan, -3.0, np.inf, 2.0, -np.inf, -1.0, 5.0], np.float32)
    m = np.array([1, 1, 1, 1, 1, 1, 0], np.uint8)
    assert sorted(R.select_compact(v, m)) == [-3.0, -1.0, 2.0]
    assert sorted(R.select_compact(v, m, use_abs=True, le_thr=2.0)) == [1.0, 2.0]
    out, cnt, _ = R.select_ref(v, np.zeros(7, np.uint8), [50.0, R.MEDIAN])
    assert cnt == 0 and (R.bits(out) == R.QNAN_BITS).all()
    assert R.same_result(np.float32(np.nan), -np.float32(np.nan)) and R.same_result(np.float32(0.0), np.float32(-0.0))
    assert not R.same_result(np.float32(1.0), np.float32(np.nan)) and not R.same_result(np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0)))


@pytest.mark.parametrize("order", [1, 2])
def test_fit_references_agree_and_recover_the_surface(order):
    h, w = 90, 130
    rng = np.random.default_rng(order)
    yy, xx = np.indices((h, w))
    xn, yn = (xx - (w - 1) / 2) / ((w - 1) / 2), (yy - (h - 1) / 2) / ((h - 1) / 2)
    true = np.array([0.7, -0.4, 1.5, 0.3, -0.2, 0.25]) * ([1, 1, 1, 1, 1, 1] if order == 2 else [1, 1, 1, 0, 0, 0])
    z = true[0] * xn + true[1] * yn + true[2] + true[3] * xn * xn + true[4] * xn * yn + true[5] * yn * yn + 0.01 * rng.standard_normal((h, w))
    out = rng.random((h, w)) < 0.05
    z[out] += 5.0
    z = z.astype(np.float32)
    mask = ((xx - 60) ** 2 + (yy - 45) ** 2 <= 44 ** 2).astype(np.uint8)
    c32, r32 = R.polyfit_ref32(z, mask, order, 6, 4.685)
    c64, r64 = R.polyfit_ref64(z, mask, order, 6, 4.685)
    assert np.abs(c64 - true).max() < 5e-3                          # robust: the 5 % outliers of +5 do not pull the surface
    assert np.abs(c32 - c64).max() < 1e-4 and np.abs(r32 - r64).max() < 1e-4
    # too few pixels: zero coefficients, fit 0 (ftp_oracle.robust_polyfit2d)
    few = np.zeros((h, w), np.uint8)
    few[0, :150 % w] = 1
    c32, r32 = R.polyfit_ref32(z, few, order, 6, 4.685)
    c64, r64 = R.polyfit_ref64(z, few, order, 6, 4.685)
    assert not c32.any() and not c64.any() and (R.bits(r32) == R.bits(z)).all() and (r64 == z).all()


@pytest.mark.parametrize("sigma,taps", [(0.25, 3), (0.5, 5), (0.75, 7), (1.0, 9), (1.25, 11), (1.5, 13), (1.75, 15), (2.0, 17), (2.5, 21), (6.0, 49), (9.0, 73)])
def test_blur_reference_is_within_its_rounding_bound_of_the_float64_convolution(sigma, taps):
    """also on frames shorter than the radius: cvlite reflects repeatedly (len <= r is handled), as np.pad's reflect does"""
    assert cvlite.gaussian_ksize(sigma) == taps
    rng = np.random.default_rng(taps)
    for h, w in ((8, 8), (9, 65), (33, 129), (31, 7), (2, 3)):
        src = rng.standard_normal((h, w)).astype(np.float32)
        a, b = R.blur_ref32(src, sigma), R.blur_ref64(src, sigma)
        err, bound = float(np.abs(a - b).max()), R.blur_ref32_bound(src, sigma)
        assert err <= bound, (h, w, err, bound)
        assert err <= 8 * 2.0 ** -23 * np.abs(src).max()          # in practice a few float32 ulps of max|src|


# ---- the demodulation references ---------------------------------------------------------------------------------------------------------
def _c128(re, im):
    return np.asarray(re, np.float64) + 1j * np.asarray(im, np.float64)


def _demod_cfg(pad, bw):
    return O.OracleConfig(bad_pixel_enable=False, illum_sigma_px=3.0, pre_blur_sigma_px=0.0, fft_pad_px=pad, patch_half_width_bins=bw, dc_exclusion=2,
                          n_fft_peaks=12)


@pytest.mark.parametrize("h,w,pad,bw,peak", [(24, 31, 16, 3, None), (20, 26, 0, 4, (24.3, 1.2)), (24, 31, 5, 3, (39.6, 17.5))])
def test_reference_tables_composed_reproduce_fft2_of_the_padded_plane_and_the_oracles_field(h, w, pad, bw, peak):
    """Ey . x . Ex against np.fft.fft2(pad_reflect(x)) on the patch, and Gy . (win * patch) . Gx against the field of ftp_complex_demod, both to
    1e-12 of the largest value: a searched carrier, a locked one whose patch the spectrum border clips (pad 0), and a locked one with an exact
    half offset."""
    rng = np.random.default_rng(h * w + pad)
    img = rng.integers(0, 256, (h, w)).astype(np.uint8)
    cfg = _demod_cfg(pad, bw)
    o = O.ftp_complex_demod(img, np.ones((h, w), np.float32), cfg, locked_peak_refined=peak)
    x = o["inter"]["iw"]
    assert x.dtype == np.float32
    hf, wf = o["fft_shape"]
    pxf, pyf = o["peak_refined"]
    px_i, py_i = int(np.round(pxf)), int(np.round(pyf))
    x0, x1, y0, y1 = max(0, px_i - bw), min(wf, px_i + bw + 1), max(0, py_i - bw), min(hf, py_i + bw + 1)
    ph, pw = y1 - y0, x1 - x0
    if peak == (24.3, 1.2):
        assert ph < 2 * bw + 1 and pw < 2 * bw + 1                     # clipped on two sides
    exr, exi, _ = R.table_forward_ref(w, pad, x0, pw)
    eyr, eyi, _ = R.table_forward_ref(h, pad, y0, ph)
    tr, ti, _, _ = R.cprod((x.astype(R.LD), None), (exr, exi))
    pr, pi, _, _ = R.cprod((eyr.T, eyi.T), (tr, ti))
    padded = cvlite.pad_reflect(x, pad) if pad > 0 else x
    want = np.fft.fftshift(np.fft.fft2(padded.astype(np.float64)))[y0:y1, x0:x1]
    err = np.abs(_c128(pr, pi) - want).max() / np.abs(want).max()
    print("forward tables vs fft2: %.3g" % err)
    assert err <= 1e-12
    dpx, dpy = pxf - px_i, pyf - py_i
    if not (abs(dpx) > 1e-6 or abs(dpy) > 1e-6):
        dpx = dpy = 0.0
    win = O.hann_patch_window(ph, pw).astype(R.LD)
    gxr, gxi, _ = R.table_inverse_ref(w, pad, x0, pw, dpx, 0, 1.0)
    gyr, gyi, _ = R.table_inverse_ref(h, pad, y0, ph, dpy, 0, 1.0 / (hf * wf))
    qr, qi, _, _ = R.cprod((pr * win, pi * win), (gxr, gxi))
    fr, fi, _, _ = R.cprod((gyr.T, gyi.T), (qr, qi))
    err = np.abs(_c128(fr, fi) - o["field"]).max() / np.abs(o["field"]).max()
    print("inverse tables vs the oracle's field: %.3g" % err)
    assert err <= 1e-12
    # in place (keep_carrier): the same patch left where it is -- the field times the carrier exp(2 pi i (kx X / Wf + ky Y / Hf)) of the integer peak
    kxr, kxi, _ = R.table_inverse_ref(w, pad, x0, pw, dpx, 1, 1.0)
    kyr, kyi, _ = R.table_inverse_ref(h, pad, y0, ph, dpy, 1, 1.0 / (hf * wf))
    qr, qi, _, _ = R.cprod((pr * win, pi * win), (kxr, kxi))
    kr, ki, _, _ = R.cprod((kyr.T, kyi.T), (qr, qi))
    X, Y = np.arange(w) + pad, np.arange(h) + pad
    shift = np.exp(2j * np.pi * (((x0 + pw // 2 - wf // 2) * X[None, :] / wf) + ((y0 + ph // 2 - hf // 2) * Y[:, None] / hf)))
    assert np.abs(_c128(kr, ki) - o["field"] * shift).max() / np.abs(o["field"]).max() <= 1e-12


def test_longdouble_dft_is_numpys_fft2():
    rng = np.random.default_rng(3)
    p = rng.standard_normal((25, 27)).astype(np.float32)
    re, im = R.dft2_ld(p)
    want = np.fft.fft2(p.astype(np.float64))
    assert np.abs(_c128(re, im) - want).max() <= 1e-12 * np.abs(want).max()


def test_cprod_is_the_complex_product_and_its_bound_holds_for_float64():
    rng = np.random.default_rng(4)
    a, b = rng.standard_normal((3, 5, 7)) + 1j * rng.standard_normal((3, 5, 7)), rng.standard_normal((7, 4)) + 1j * rng.standard_normal((7, 4))
    re, im, bre, bim = R.cprod((a.real, a.imag), (b.real, b.imag))
    got = a @ b
    assert (np.abs(got.real - re) <= bre).all() and (np.abs(got.imag - im) <= bim).all()
    assert float((bre / np.abs(re)).min()) < 1e-14                  # and the bound is of the size of float64 rounding, not a loose bar
    lo, hi = R.f32_interval(np.array([1.0, 1.0 + 2.0 ** -24]), np.array([1e-12, 1e-12]))
    assert lo[0] == hi[0] == np.float32(1.0) and lo[1] == np.float32(1.0) and hi[1] == np.nextafter(np.float32(1.0), np.float32(2.0))


def test_peak_cases_are_what_their_names_say():
    cases = {c.name: c for c in D.peak_cases()}
    assert cases["plane_of_64_all_listed"].mag[0].size == 64 and cases["batch_of_3"].mag.shape[0] == 3
    for c in cases.values():
        for mag in c.mag:
            rule = R.top_peaks_rule(mag, c.dc, c.npeaks)
            assert D.overflows(mag, c.dc, c.npeaks) == c.overflow, c.name
            if c.distinct:                                          # an order is asserted: the values are pairwise distinct, and the oracle agrees
                assert len(np.unique(mag)) == mag.size, c.name
                assert rule == O.find_top_peaks(mag, c.dc, c.npeaks), c.name
            else:                                                   # NumPy leaves the order of equal values open: the values still agree
                assert [v for _, _, v in rule] == [v for _, _, v in O.find_top_peaks(mag, c.dc, c.npeaks)], c.name
    c = cases["dc_box_is_the_plane"]
    assert c.dc > max(c.mag.shape[1:]) // 2 and all(v == 0 for _, _, v in R.top_peaks_rule(c.mag[0], c.dc, c.npeaks))
    for name, stride, count in (("crowded_128x64", 5, 8), ("crowded_128x96_twelve_in_one_stride", 5, 12)):
        c = cases[name]
        idx = [y * c.mag.shape[2] + x for x, y, _ in R.top_peaks_rule(c.mag[0], c.dc, c.npeaks)]
        assert sum(i % 1024 == stride for i in idx) == count and len(idx) == 12, name
    c = cases["plateau_of_6"]
    rule = R.top_peaks_rule(c.mag[0], c.dc, c.npeaks)
    idx = [y * 64 + x for x, y, _ in rule[:6]]
    assert [v for _, _, v in rule[:6]] == [3.0] * 6 and rule[6][2] < 3.0 and idx == sorted(idx) and sum(i % 1024 == 7 for i in idx) == 5
    c = cases["sparse_8_positive"]
    rule = R.top_peaks_rule(c.mag[0], c.dc, c.npeaks)
    assert [v for _, _, v in rule] == [8.0, 7.0, 6.0, 5.0, 4.0, 3.0, 2.0, 1.0, 0.0, 0.0, 0.0, 0.0] and np.count_nonzero(c.mag) == 8
    assert all((y * 64 + x) % 1024 == 0 for x, y, v in rule if v > 0)
    assert [(x, y) for x, y, _ in R.top_peaks_rule(cases["all_zero"].mag[0], 4, 12)] == [(i, 0) for i in range(12)]


def test_carrier_cases_are_what_their_names_say():
    assert D.HALF + 1e-12 == 1.0 and np.log(D.HALF + 1e-12) == 0.0
    cases = {c.name: c for c in D.carrier_cases()}
    cy, cx = D.HF // 2, D.WF // 2
    for c in cases.values():
        gd, gi, (bx, by) = R.carrier_ref(c.peaks, c.mag, c.bw, c.frac)
        assert len({(x, y) for x, y, _ in c.peaks}) == len(c.peaks), c.name
        if c.exact_half:
            assert gd[0] - gi[6] == 0.5 and gd[1] - gi[7] == 0.5, c.name
        else:                       # further from a rounding boundary (x.5 for the integer peak, 1e-6 for the zeroed remainders) than the bound
            for v, b in ((gd[0], bx), (gd[1], by)):
                assert abs(abs(v - np.floor(v)) - 0.5) > 10 * b + 1e-9, c.name
                assert abs(abs(v - np.round(v)) - 1e-6) > 10 * b + 1e-9, c.name
    max_dy = int(0.12 * D.HF)
    assert max_dy == 4 and 0.12 * D.HF > 4.5
    right = lambda c: [p for p in c.peaks if p[0] > cx]
    near = lambda ps: [p for p in ps if abs(p[1] - cy) <= max_dy]
    assert not right(cases["no_peak_right_of_centre"])
    c = cases["no_peak_near_the_centre_row"]
    assert right(c) and not near(right(c))
    for name in ("both_filters_strongest_left_next_far", "both_filters_strongest_right_but_far"):
        c = cases[name]
        best = max(c.peaks, key=lambda p: p[2])
        chosen = tuple(R.carrier_ref(c.peaks, c.mag, c.bw, c.frac)[1][6:8])
        assert chosen != best[:2] and near(right(c)) and (best not in near(right(c))), name
    c = cases["both_filters_strongest_left_next_far"]
    srt = sorted(c.peaks, key=lambda p: -p[2])
    assert srt[0] not in right(c) and srt[1] in right(c) and srt[1] not in near(right(c))
    assert max(cases["both_filters_strongest_right_but_far"].peaks, key=lambda p: p[2]) in right(cases["both_filters_strongest_right_but_far"])
    c = cases["equal_values_first_listed_wins"]
    assert tuple(R.carrier_ref(c.peaks, c.mag, c.bw, c.frac)[1][6:8]) == (33, 21) and [p[2] for p in c.peaks[1:]] == [7.0] * 3
    assert len(cases["one_peak"].peaks) == 1 and len(cases["64_peaks"].peaks) == 64
    c = cases["max_dy_truncates"]
    assert abs(c.peaks[0][1] - cy) == 5 and c.peaks[0][2] > c.peaks[1][2] and tuple(R.carrier_ref(c.peaks, c.mag, c.bw, c.frac)[1][6:8]) == c.peaks[1][:2]
    for name in ("border_left", "border_right", "border_top", "border_bottom"):
        gd, gi, _ = R.carrier_ref(cases[name].peaks, cases[name].mag, 3, 0.12)
        assert gd[0] == gi[6] and gd[1] == gi[7] and (gi[6] in (0, D.WF - 1) or gi[7] in (0, D.HF - 1)), name
    gd, gi, _ = R.carrier_ref(*cases["three_equal_neighbours_in_x"][1:5])
    assert gd[0] == gi[6] and gd[1] != gi[7]
    c = cases["zero_magnitude_neighbour"]
    assert c.mag[21, 30] == 0.0 and np.isfinite(R.carrier_ref(*c[1:5])[0]).all()
    gd, gi, _ = R.carrier_ref(*cases["offsets_below_1e-6_both_zeroed"][1:5])
    assert 0 < abs(gd[0] - gi[6]) < 1e-6 and 0 < abs(gd[1] - gi[7]) < 1e-6 and gd[4] == 0.0 and gd[5] == 0.0
    gd, gi, _ = R.carrier_ref(*cases["offset_below_1e-6_in_x_only_both_kept"][1:5])
    assert 0 < abs(gd[4]) < 1e-6 and abs(gd[5]) > 1e-6
    assert [R.carrier_ref(*cases["exact_half_px_%d" % p][1:5])[1][4] for p in (20, 21)] == [20, 22]
    assert R.carrier_ref(*cases["chosen_value_zero"][1:5])[1][8] == 0
    for name, field, full in (("clipped_left", 3, False), ("clipped_right", 3, False), ("clipped_top", 2, False), ("clipped_bottom", 2, False), ("one_peak", 3, True)):
        gi = R.carrier_ref(*cases[name][1:5])[1]
        assert (gi[field] == 7) == full and gi[8] == 1, name
