"""Plain references for the kernels that tests/test_kernels_direct.py launches directly: exact selection, the IRLS surface fit and the
separable Gaussian.  NumPy only (plus the oracle's own functions); nothing here touches the GPU.  tests/test_kernel_refs.py checks the
references against each other on the CPU."""
import numpy as np

from oracle import cvlite
from oracle import ftp_oracle as O

QNAN_BITS = 0x7FC00000          # what the selection kernels return when no element is valid
MEDIAN = None                   # a request: np.median instead of np.percentile


# ---------------------------------------------------------------------------------------------------------------------------------------
# order-preserving float32 <-> uint32 keys (common.hpp: f2key / key2f); -0.0 sorts just below +0.0

def f2key(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def key2f(k):
    k = np.ascontiguousarray(k, np.uint32)
    u = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)
    return u.view(np.float32)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def request_value(q):
    """what the kernel is handed for a request: float32(q) / float32(100) (np.percentile's own division), negative for the median"""
    return np.float32(-1.0) if q is MEDIAN else np.float32(q) / np.float32(100.0)


# ---------------------------------------------------------------------------------------------------------------------------------------
# selection

def select_compact(vals, mask, use_abs=False, le_thr=None):
    vals = np.asarray(vals, np.float32).ravel()
    v = vals[(np.asarray(mask).ravel() != 0) & np.isfinite(vals)]
    if use_abs:
        v = np.abs(v)
    if le_thr is not None:
        v = v[v <= np.float32(le_thr)]
    return v.astype(np.float32)


def select_ref(vals, mask, reqs, use_abs=False, le_thr=None):
    """(results float32[len(reqs)], count, neighbours): NumPy's float32 percentile / median of the compacted values; neighbours[j] is
    (rank k, s[k - 1], s[k], s[k + 1]) around the request's lower rank in the sorted values (None outside the array), for diagnostics."""
    v = select_compact(vals, mask, use_abs, le_thr)
    n = int(v.size)
    out = np.empty(len(reqs), np.float32)
    nbrs = []
    s = key2f(np.sort(f2key(v)))
    for j, q in enumerate(reqs):
        if n == 0:
            out[j] = np.array([QNAN_BITS], np.uint32).view(np.float32)[0]
            nbrs.append(None)
            continue
        with np.errstate(all="ignore"):
            out[j] = np.median(v) if q is MEDIAN else np.percentile(v, float(q))
        k = (n - 1) // 2 if q is MEDIAN else min(n - 1, int(np.floor((n - 1) * float(q) / 100.0)))
        nbrs.append((k, float(s[k - 1]) if k > 0 else None, float(s[k]), float(s[k + 1]) if k + 1 < n else None))
    return out, n, nbrs


def percentile_model(sorted_vals, q):
    """what select.hpp (np_percentile_index, np_lerp) computes from the two neighbouring order statistics, restated in float32 NumPy scalars:
    vi = (n - 1) * q32, k = floor(vi), gamma = vi - k, a + (b - a) * gamma, or b - (b - a) * (1 - gamma) from gamma = 0.5 on"""
    f = np.float32
    s = np.asarray(sorted_vals, f)
    n = s.size
    vi = f(f(n - 1) * request_value(q))
    if vi >= f(n - 1):
        return s[n - 1]
    k = int(np.floor(vi))
    g, d = f(vi - f(k)), f(s[k + 1] - s[k])
    return f(s[k + 1] - f(d * f(f(1) - g))) if g >= f(0.5) else f(s[k] + f(d * g))


def same_result(got, exp):
    """Bit equality of two float32 results, with two exceptions where NumPy's own bits are not a function of the values selected.
    A NaN (the interpolation's inf * 0 when the neighbours are 6e38 apart) carries the sign of the host's default NaN: any NaN equals
    any NaN.  The sign of a ZERO result depends on NumPy's code path and element order, not on the data (np.median of [-0.0] is +0.0,
    np.percentile of the same array at 50 is -0.0, at 100 of [-0.0, -0.0] it is +0.0; with both zeros present the partition decides):
    a zero equals a zero of either sign.  Nothing downstream of a threshold distinguishes the two."""
    g, e = np.float32(got), np.float32(exp)
    if np.isnan(g) or np.isnan(e):
        return bool(np.isnan(g) and np.isnan(e))
    if g == 0 and e == 0:
        return True
    return int(bits(g).ravel()[0]) == int(bits(e).ravel()[0])


# ---------------------------------------------------------------------------------------------------------------------------------------
# IRLS fit

def _pad6(coef):
    c = np.zeros(6, np.asarray(coef).dtype)
    c[:len(coef)] = coef
    return c


def polyfit_ref32(z, mask, order, iters, c):
    """the oracle (float32 LAPACK): (coef[6] float32, residual plane z - fit in float32, NaN where z is)"""
    z = np.asarray(z, np.float32)
    with np.errstate(all="ignore"):
        coef, fit = O.robust_polyfit2d(z, np.asarray(mask) != 0, order=order, iters=iters, c=c)
        return _pad6(coef), (z - fit).astype(np.float32)


def polyfit_ref64(z, mask, order, iters, c, min_count=200):
    """the same IRLS in float64 throughout (coordinates, design, lstsq, medians, weights, evaluation): (coef[6] float64, z - fit float64)"""
    z = np.asarray(z, np.float32).astype(np.float64)
    h, w = z.shape
    m = (np.asarray(mask) != 0) & np.isfinite(z)
    if np.count_nonzero(m) < min_count:
        return np.zeros(6), z.copy()
    yy, xx = np.indices((h, w))
    xnf = (xx - (w - 1) / 2.0) / ((w - 1) / 2.0)
    ynf = (yy - (h - 1) / 2.0) / ((h - 1) / 2.0)
    xn, yn, zz = xnf[m], ynf[m], z[m]
    a = O._design(xn, yn, order)
    wts = np.ones_like(zz)
    for _ in range(iters):
        coef = np.linalg.lstsq(a * wts[:, None], zz * wts, rcond=None)[0]
        r = zz - a @ coef
        med = np.median(r)
        sigma = 1.4826 * (np.median(np.abs(r - med)) + 1e-6)
        u = r / (c * sigma)
        wts = 1.0 / (1.0 + u * u)
    with np.errstate(invalid="ignore"):
        return _pad6(coef), z - O._eval_poly(xnf, ynf, coef, order)


# ---------------------------------------------------------------------------------------------------------------------------------------
# Gaussian

def blur_ref32(src, sigma):
    """cv::GaussianBlur's row pass and symmetric column pass in float32 with fused multiply-adds, as the kernels execute them"""
    return cvlite.gaussian_blur(np.asarray(src, np.float32), float(sigma))


def blur_ref64(src, sigma):
    """the same float32 taps, separable convolution with BORDER_REFLECT_101 in float64"""
    src = np.asarray(src, np.float32).astype(np.float64)
    n = cvlite.gaussian_ksize(sigma)
    k = cvlite.gaussian_kernel(n, sigma).astype(np.float64)
    r = n // 2
    p = np.pad(src, ((0, 0), (r, r)), mode="reflect")
    t = sum(k[j] * p[:, j:j + src.shape[1]] for j in range(n))
    p = np.pad(t, ((r, r), (0, 0)), mode="reflect")
    return sum(k[j] * p[j:j + src.shape[0], :] for j in range(n))


def blur_ref32_bound(src, sigma):
    """worst-case distance of the float32 sequence from the exact convolution: every one of the n roundings of a pass is at most half an
    ulp of a partial sum, and the partial sums of positive taps adding up to one never exceed max|src|; two passes, plus the rounding of
    the intermediate plane and of the float64 reference's own taps"""
    n = cvlite.gaussian_ksize(sigma)
    return (2 * n + 2) * 2.0 ** -24 * float(np.max(np.abs(np.asarray(src, np.float64))))
