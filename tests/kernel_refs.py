"""Plain references for the kernels that tests/test_kernels_direct.py and tests/test_dft_direct.py launch directly: exact selection, the IRLS
surface fit, the separable Gaussian, and the demodulation family (float64 GEMM stages, twiddle tables, peak search, carrier choice) in
np.longdouble with mpmath's unit roots.  NumPy only (plus the oracle's own functions); nothing here touches the GPU.
tests/test_kernel_refs.py checks the references against each other on the CPU."""
import functools

import mpmath
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


# ---------------------------------------------------------------------------------------------------------------------------------------
# demodulation (k_dft.hip, k_dft_tables.hip, cgemm_mfma.hpp): everything in np.longdouble (64-bit mantissa), unit roots from mpmath

LD = np.longdouble
U53 = LD(2.0) ** -53            # unit roundoff of float64


def _mp_to_ld(x):
    hi = float(x)
    return LD(hi) + LD(float(x - hi))


def cis_turns(num, den):
    """(cos, sin)(2 pi num / den) as longdoubles; num an int, a float (taken exactly) or an mpf"""
    with mpmath.workdps(40):
        t = mpmath.mpf(num) / den
        t -= mpmath.floor(t)
        a = 2 * mpmath.pi * t
        return _mp_to_ld(mpmath.cos(a)), _mp_to_ld(mpmath.sin(a))


@functools.lru_cache(maxsize=None)
def unit_roots(n):
    """(cos, sin)(2 pi m / n), m = 0..n-1"""
    cs = [cis_turns(m, n) for m in range(n)]
    return np.array([c for c, _ in cs], LD), np.array([x for _, x in cs], LD)


def reflect_map(n, pad):
    """padded position -> source position of cv2.copyMakeBorder(BORDER_REFLECT), read off the oracle's pad_reflect on an index ramp"""
    if pad == 0:
        return np.arange(n)
    ramp = np.arange(n, dtype=np.float32)[None, :]
    return cvlite.pad_reflect(ramp, pad)[0].astype(np.int64)


def table_forward_ref(n, pad, f0, cnt, zero_from=None, layout=None):
    """E[s][c] = sum over the padded positions X that the reflect padding maps to s of exp(-2 pi i f_c X / N), N = n + 2 pad, f_c = f0 + c - N // 2
    (f0: the patch origin in the fftshift-ed spectrum).  Returns (re, im, bound) [n][layout or cnt]; columns from zero_from (default cnt) on are
    zero.  bound: each unit root of the kernel is good to 4 * 2^-53 per component (argument 2 m / N rounded once: pi * 2^-53, sincospi itself
    one ulp), so the sum of t of them to t * 4 * 2^-53."""
    N = n + 2 * pad
    cs, sn = unit_roots(N)
    src = reflect_map(n, pad)
    lay = layout if layout is not None else cnt
    re, im = np.zeros((n, lay), LD), np.zeros((n, lay), LD)
    X = np.arange(N)
    for c in range(cnt if zero_from is None else min(cnt, zero_from)):
        m = ((f0 + c - N // 2) * X) % N
        np.add.at(re[:, c], src, cs[m])
        np.add.at(im[:, c], src, -sn[m])
    terms = np.bincount(src, minlength=n).astype(LD)
    bound = np.repeat((terms * 4 * U53)[:, None], lay, axis=1)
    return re, im, bound


def table_inverse_ref(n, pad, p0, cnt, d, keep, scale, layout=None):
    """G[c][x]: what a unit value in bin c of the patch contributes to pixel x of the crop, literally: the patch is written into an empty
    fftshift-ed spectrum of N = n + 2 pad bins at N // 2 - cnt // 2 (re-centred at DC) or at p0 (keep: in place), np.fft.ifftshift moves it, the
    inverse DFT sums exp(+2 pi i k X / N) (its 1 / N is part of `scale`), the sub-bin ramp multiplies by exp(-2 pi i d X / N), the crop keeps
    X = x + pad.  Returns (re, im, bound) [layout or cnt][n].
    bound = 2 pi * 4 * 2^-53 * (1 + |arg|) * scale: the kernel hands sincospi the argument arg = 2 m / N - 2 d (X / N), formed with four roundings
    (two quotients, the product, the difference) of at most 2^-53 relative to quantities no larger than 1 + |arg|; d/d(arg) exp(i pi arg) is
    pi, and the bound is doubled for sincospi's own ulp and the rounding of the product with scale."""
    N = n + 2 * pad
    came_from = np.fft.ifftshift(np.arange(N))            # came_from[k]: the shifted position whose value lands on frequency index k
    lay = layout if layout is not None else cnt
    re, im, bound = np.zeros((lay, n), LD), np.zeros((lay, n), LD), np.zeros((lay, n), LD)
    sc = LD(scale)
    for c in range(cnt):
        j = p0 + c if keep else N // 2 - cnt // 2 + c
        k = int(np.nonzero(came_from == j)[0][0])
        for x in range(n):
            X = x + pad
            with mpmath.workdps(40):
                co, si = cis_turns(mpmath.mpf(k * X) - mpmath.mpf(float(d)) * X, N)
            re[c, x], im[c, x] = co * sc, si * sc
            arg = 2.0 * ((k * X) % N) / N + 2.0 * abs(float(d)) * X / N
            bound[c, x] = 2 * LD(np.pi) * 4 * U53 * (1 + arg) * sc
    return re, im, bound


def cprod(A, B, bA=None, bB=None, ksteps=None):
    """The product A [.., m, k] . B [.., k, n] of two complex operands given as (re, im) pairs of longdouble arrays (im None: real), by einsum.
    Returns (re, im, bound_re, bound_im): the componentwise bound (K + 3) 2^-53 (|A| . |B|) of a float64 evaluation with K real k-steps per
    component (2 k for two complex operands, k with a real one; `ksteps` overrides k), the 3 for the operand conversion and a final window or
    scale, plus what the operands' own bounds bA, bB (pairs like the operands) propagate through the absolute values."""
    e = functools.partial(np.einsum, "...ik,...kj->...ij")
    z = lambda x, like: np.zeros_like(like) if x is None else np.asarray(x, LD)
    Ar, Br = np.asarray(A[0], LD), np.asarray(B[0], LD)
    Ai, Bi = z(A[1], Ar), z(B[1], Br)
    re, im = e(Ar, Br) - e(Ai, Bi), e(Ar, Bi) + e(Ai, Br)
    aAr, aAi, aBr, aBi = np.abs(Ar), np.abs(Ai), np.abs(Br), np.abs(Bi)
    k = Ar.shape[-1] if ksteps is None else ksteps
    K = k * (1 if (A[1] is None or B[1] is None) else 2)
    bre, bim = (K + 3) * U53 * (e(aAr, aBr) + e(aAi, aBi)), (K + 3) * U53 * (e(aAr, aBi) + e(aAi, aBr))
    if bA is not None:
        bAr, bAi = z(bA[0], Ar), z(bA[1], Ar)
        bre, bim = bre + e(bAr, aBr) + e(bAi, aBi), bim + e(bAr, aBi) + e(bAi, aBr)
        aAr, aAi = aAr + bAr, aAi + bAi
    if bB is not None:
        bBr, bBi = z(bB[0], Br), z(bB[1], Br)
        bre, bim = bre + e(aAr, bBr) + e(aAi, bBi), bim + e(aAr, bBi) + e(aAi, bBr)
    return re, im, bre, bim


def demod_chain(a, Ex, Ey, win, Gx, Gy):
    """the four stages on one frame's operand a [h][w] (longdouble): every table is (re, im, bound) in the kernels' layout (Ex [w][pw],
    Ey [ph][h], Gx [pw][w], Gy [h][ph]), win [ph][pw].  Returns a dict of (re, im, bound_re, bound_im) for T, patch, Q and field, each bound
    carrying the ones before it."""
    w = np.asarray(win).astype(LD)
    T = cprod((a, None), Ex[:2], bB=(Ex[2], Ex[2]))
    P = cprod(Ey[:2], T[:2], bA=(Ey[2], Ey[2]), bB=T[2:])
    P = (P[0] * w, P[1] * w, P[2] * np.abs(w), P[3] * np.abs(w))
    Q = cprod(P[:2], Gx[:2], bA=P[2:], bB=(Gx[2], Gx[2]))
    F = cprod(Gy[:2], Q[:2], bA=(Gy[2], Gy[2]), bB=Q[2:])
    return {"T": T, "patch": P, "Q": Q, "field": F}


def fsub32(iw, mu):
    """float32(iw) - float32(mu[b]) rounded to float32 (the kernel's __fsub_rn), as longdouble; iw [B, h, w]"""
    iw = np.asarray(iw, np.float32)
    if mu is None:
        return iw.astype(LD)
    return (iw - np.asarray(mu, np.float32)[:, None, None]).astype(np.float32).astype(LD)


def f32_interval(ref, bound):
    """the float32 results a correctly rounded float64 computation within `bound` of `ref` can give: [float32(ref - bound), float32(ref + bound)].
    The two ends are equal, the float32 rounding of ref, unless ref lies within the bound of a rounding boundary."""
    ref, bound = np.asarray(ref, LD), np.asarray(bound, LD)
    return (ref - bound).astype(np.float32), (ref + bound).astype(np.float32)


def dft2_ld(plane):
    """the unshifted 2-D DFT of a real plane, in longdouble: (re, im)"""
    p = np.asarray(plane).astype(LD)
    H, W = p.shape
    cy, sy = unit_roots(H)
    cx, sx = unit_roots(W)
    my, mx = np.outer(np.arange(H), np.arange(H)) % H, np.outer(np.arange(W), np.arange(W)) % W
    tr, ti, _, _ = cprod((p, None), (cx[mx], -sx[mx]))
    re, im, _, _ = cprod((cy[my], -sy[my]), (tr, ti))
    return re, im


def amp_bound(fr, fi, bre, bim):
    """|z| in float64 from parts within (bre, bim) of (fr, fi): the hypot of the bounds, plus the three roundings of sqrt(fma(re, re, im * im)).
    Returns (|z|, bound)"""
    amp = np.sqrt(fr * fr + fi * fi)
    return amp, np.sqrt(bre * bre + bim * bim) + 3 * U53 * amp


def full_mag_ref(plane, pad):
    """|fftshift(fft2(pad_reflect(plane)))| [Hf][Wf] in longdouble and the bound of launch_dft_full_mag on tables within their own bound: the
    stages' composed bound on the computed half fx <= Wf / 2, carried to the mirror positions as the values are.  Also returns the reference
    tables (Exf, Eyf) as (re, im, bound) in the kernels' layout."""
    plane = np.asarray(plane, np.float32)
    h, w = plane.shape
    Hf, Wf, Wh = h + 2 * pad, w + 2 * pad, (w + 2 * pad) // 2 + 1
    ex = table_forward_ref(w, pad, Wf // 2, Wh)
    ey = table_forward_ref(h, pad, Hf // 2, Hf)
    ey = (ey[0].T, ey[1].T, ey[2].T)
    t = cprod((plane.astype(LD), None), ex[:2], bB=(ex[2], ex[2]))
    f = cprod(ey[:2], t[:2], bA=(ey[2], ey[2]), bB=t[2:])
    dr, di = dft2_ld(cvlite.pad_reflect(plane, pad) if pad else plane)
    assert max(float(np.abs(dr[:, :Wh] - f[0]).max()), float(np.abs(di[:, :Wh] - f[1]).max())) <= 1e-15 * float(np.abs(dr).max())   # the two statements agree
    _, bamp = amp_bound(f[0], f[1], f[2], f[3])
    bound = np.zeros((Hf, Wf), LD)
    fy, fx = np.indices((Hf, Wh))
    bound[fy, fx] = bamp
    np.maximum.at(bound, ((Hf - fy) % Hf, (Wf - fx) % Wf), bamp)
    return np.fft.fftshift(np.sqrt(dr * dr + di * di)), np.fft.fftshift(bound), ex, ey


def top_peaks_rule(mag, dc, n):
    """the kernel's written rule: the n largest values outside the DC box (counted as zero inside), descending, equal values by ascending
    linear index.  [(x, y, value)]"""
    mag = np.asarray(mag, np.float64)
    h, w = mag.shape
    cy, cx = h // 2, w // 2
    work = mag.copy()
    work[max(0, cy - dc):min(h, cy + dc), max(0, cx - dc):min(w, cx + dc)] = 0
    flat = work.ravel()
    order = np.lexsort((np.arange(flat.size), -flat))[:n]
    return [(int(i % w), int(i // w), float(flat[i])) for i in order]


def parabola_offset_and_sensitivity(fm1, f0, fp1):
    """(offset, |d/dfm1| + |d/df0| + |d/dfp1|) of the log-parabola vertex 0.5 (fm1 - fp1) / (fm1 - 2 f0 + fp1); (0, 0) where the reference
    returns 0 for a flat denominator"""
    den = fm1 - 2.0 * f0 + fp1
    if abs(den) < 1e-12:
        return 0.0, 0.0
    num = fm1 - fp1
    return 0.5 * num / den, abs(0.5 / den - 0.5 * num / den ** 2) + abs(num / den ** 2) + abs(-0.5 / den - 0.5 * num / den ** 2)


def carrier_ref(peaks, mag, bw, max_dy_frac, log_err=0.0):
    """CarrierGeom of k_carrier_choose from the oracle's own functions: choose_carrier_peak, refine_peak_parabolic_log and the geometry lines of
    ftp_complex_demod.  Returns (gd[7], gi[10], bound): bound = (bx, by), the distance within which a float64 evaluation whose logarithms are
    good to e = 2 ulp of the largest |log| involved stays of the reference's refined peak: (sum of |partial derivatives|) * e + 4 * 2^-53 |x|.
    log_err: added to e, for magnitudes that themselves carry a relative error (a spectrum computed by the kernels)."""
    mag = np.asarray(mag, np.float64)
    hf, wf = mag.shape
    cy, cx = hf // 2, wf // 2
    px, py = O.choose_carrier_peak(peaks, hf, wf, max_dy_frac)
    value = next(p[2] for p in peaks if (p[0], p[1]) == (px, py))
    pxf, pyf = O.refine_peak_parabolic_log(mag, px, py)
    bx = by = 0.0
    if 0 < px < wf - 1 and 0 < py < hf - 1:
        lm = np.log(mag[py - 1:py + 2, px - 1:px + 2] + 1e-12)
        e = 2.0 * float(np.spacing(np.abs([lm[1, 0], lm[1, 1], lm[1, 2], lm[0, 1], lm[2, 1]]).max())) + log_err
        bx = parabola_offset_and_sensitivity(lm[1, 0], lm[1, 1], lm[1, 2])[1] * e + 4 * 2.0 ** -53 * abs(pxf)
        by = parabola_offset_and_sensitivity(lm[0, 1], lm[1, 1], lm[2, 1])[1] * e + 4 * 2.0 ** -53 * abs(pyf)
    kx, ky = pxf - cx, pyf - cy
    px_i, py_i = int(np.round(pxf)), int(np.round(pyf))
    x0, x1 = max(0, px_i - bw), min(wf, px_i + bw + 1)
    y0, y1 = max(0, py_i - bw), min(hf, py_i + bw + 1)
    ph, pw = y1 - y0, x1 - x0
    dpx, dpy = float(pxf - px_i), float(pyf - py_i)
    if not (abs(dpx) > 1e-6 or abs(dpy) > 1e-6):
        dpx = dpy = 0.0
    ok = int(value > 0 and ph >= 1 and pw >= 1 and np.isfinite(pxf) and np.isfinite(pyf))
    period = wf / abs(kx) if abs(kx) > 1e-9 else 0.0
    return (np.array([pxf, pyf, kx, ky, dpx, dpy, period]), np.array([x0, y0, ph, pw, px_i, py_i, px, py, ok, 0], np.int32), (bx, by))
