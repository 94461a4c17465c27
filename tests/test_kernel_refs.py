"""CPU checks of the references in tests/kernel_refs.py: each is compared with an independent statement of the same operation, so that a
kernel test that fails points at the kernel."""
import numpy as np
import pytest

import kernel_refs as R
from oracle import cvlite


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
