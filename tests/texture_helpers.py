"""The surface texture read-out's definition (include_ext/vistaf_texture.h) written out in NumPy and Python float64, the checks that hold
the device to it stage by stage, and hand-made scenes for tests/test_textures.py.

`numpy_textures` follows the header step by step on the box of every row, with `math.fsum` for every sum; its form fit is `np.linalg.lstsq`
with the verdict from the singular values, `numpy_textures_ne` forms the normal equations as the device does.  The device is not held to the
restatement by one invented tolerance but stage by stage (`hold_device`):
  S1  the form, as the shape read-out's fit is held: largest |P_dev - P_ref| over the evaluation pixels relative to the peak, against 4 times
      the same distance between the two restatements (floor 64 ulp);
  S2  the residual plane, bit-equal to step 3 evaluated from the device's own coefficients;
  S3  the sums, from the device's own residual plane: integers exact, a sum of n terms within 1.01 * n * 2^-53 * sum|term| of fsum (the
      order-independent summation bound; the terms are single IEEE operations, identical on both sides), a field built from sums within that
      bound pushed through its expression (the corners of the sums' intervals) plus 8 ulp for its own roundings;
  S4  the decisions (lobe, ring, profile, pitch), bit-equal to steps 7 and 8 run on the device's own window and direction;
and end to end (`hold_end_to_end`) on cases whose `decision_margin` shows that no comparison sits on its edge.
"""
import itertools
import math

import numpy as np

from shapes_helpers import C_PEAK, C_X0, C_X1, C_Y0, FLOOR, ULP, H, W, Scene, disc, pack, quadric, rect, table_box

NTEXTURE = 40
FIELDS = ("eval_pixels", "form_status", "form_c0", "form_c1", "form_c2", "form_c3", "form_c4", "form_c5", "sa_mm", "sq_mm", "ssk", "sku", "sp_mm",
          "sv_mm", "sz_mm", "sp_pixel", "sv_pixel", "grad_pixels", "sdq", "sdr", "grad_dir_x", "grad_dir_y", "coherence", "acf_valid_lags",
          "lobe_lags", "lobe_status", "sal_mm", "sal_lag_x", "sal_lag_y", "rmax_mm", "str", "pitch_mm", "pitch_acf", "profile_samples")
T = {name: i for i, name in enumerate(FIELDS)}
INT_FIELDS = ("eval_pixels", "form_status", "sp_pixel", "sv_pixel", "grad_pixels", "acf_valid_lags", "lobe_lags", "lobe_status", "sal_lag_x",
              "sal_lag_y", "profile_samples")
DECISIONS = ("acf_valid_lags", "lobe_lags", "lobe_status", "sal_mm", "sal_lag_x", "sal_lag_y", "rmax_mm", "str", "pitch_mm", "pitch_acf",
             "profile_samples")
OK, NONE, FLAT = 0, 1, 2
NTERMS = {0: 1, 1: 3, 2: 6}
NAN = float("nan")
F = np.float64


def same(a, b):
    """equal values, NaN equal to NaN (not a comparison of NaN payloads or of the sign of zero)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)]))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------------------------- steps 0 to 3
def eval_box(depth_b, index_b, row, k, eps, frac, h, w):
    """steps 0 and 1 for one row: (own box, clipped box or None, evaluation mask and float32 depths of the clipped box)"""
    own, clipped = table_box(row, h, w)
    if clipped is None:
        return own, None, None, None
    x0, y0, x1, y1 = clipped
    d = np.asarray(depth_b[y0:y1 + 1, x0:x1 + 1], dtype=np.float32)
    d = np.where(np.isnan(d), np.float32(0.0), d)
    em = (np.asarray(index_b[y0:y1 + 1, x0:x1 + 1]) == k) & (d > np.float32(eps))
    if frac != 0.0:
        with np.errstate(invalid="ignore"):
            em &= d >= np.float32(frac * row[C_PEAK])
    return own, clipped, em, d


def coords(em, own, clipped):
    bx0, by0, bx1, by1 = own
    ys, xs = np.nonzero(em)
    xc, yc = (float(bx0) + float(bx1)) / 2.0, (float(by0) + float(by1)) / 2.0
    hx, hy = max((float(bx1) - float(bx0)) / 2.0, 1.0), max((float(by1) - float(by0)) / 2.0, 1.0)
    return ((xs + clipped[0]).astype(np.float64) - xc) / hx, ((ys + clipped[1]).astype(np.float64) - yc) / hy


def poly(c, u, v):
    return c[0] + c[1] * u + c[2] * v + c[3] * (u * u) + c[4] * (u * v) + c[5] * (v * v)


def fit_lstsq(X, d):
    norm = np.sqrt((X * X).sum(axis=0))
    if not (norm > 0).all() or not np.linalg.svd(X / norm, compute_uv=False).min() > np.sqrt(FLOOR):
        return None
    return np.linalg.lstsq(X, d, rcond=None)[0]


def fit_normal_equations(X, d):
    A, rhs = X.T @ X, X.T @ d
    try:
        np.linalg.cholesky(A - FLOOR * np.diag(np.diag(A)))
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return None
    return np.linalg.solve(L.T, np.linalg.solve(L, rhs))


def form(em, d, own, clipped, degree, fit):
    """step 2: the six coefficients (zeros above the degree), or None for FORM_STATUS = 1"""
    n = NTERMS[degree]
    if int(em.sum()) < max(n, 6):
        return None
    dd = d[em].astype(np.float64)
    if not np.isfinite(dd).all():
        return None
    u, v = coords(em, own, clipped)
    X = np.stack([np.ones(len(u)), u, v, u * u, u * v, v * v], axis=1)[:, :n]
    c = fit(X, dd)
    if c is None or not np.isfinite(c).all():
        return None
    return np.concatenate([c, np.zeros(6 - n)])


def residual_box(c, em, d, own, clipped):
    """step 3 on the clipped box: float32, NaN off the evaluation pixels (and everywhere for c None)"""
    r = np.full(em.shape, np.nan, np.float32)
    if c is not None:
        u, v = coords(em, own, clipped)
        r[em] = (d[em].astype(np.float64) - poly(c, u, v)).astype(np.float32)
    return r


# ---------------------------------------------------------------------------------------------------------------- steps 4 to 6: sums
class Sum:
    """an fsum with what bounds another order of the same terms: n terms, sum of their magnitudes"""

    def __init__(self, terms):
        t = np.asarray(terms, dtype=np.float64).ravel()
        self.n = int(t.size)
        if np.isfinite(t).all():
            self.value, self.mag = math.fsum(t.tolist()), math.fsum(np.abs(t).tolist())
        else:
            self.value, self.mag = float(t.sum()), float("inf")

    def slack(self):
        return 1.01 * self.n * 2.0 ** -53 * self.mag

    def ends(self, extra=0.0):
        """the interval another order of summation stays in; extra: a relative error of every term on top of that"""
        half = self.slack() + extra * self.mag
        return (self.value - half, self.value + half) if math.isfinite(self.mag) else (self.value, self.value)


def _sqrt(x):
    with np.errstate(invalid="ignore"):
        return np.sqrt(F(x))


def f_sa(s1, m):
    return F(s1) / F(m)


def f_sq(s2, m):
    return _sqrt(F(s2) / F(m))


def f_ssk(s3, s2, m):
    sq = f_sq(s2, m)
    return (F(s3) / F(m)) / (sq * sq * sq)


def f_sku(s4, s2, m):
    sq = f_sq(s2, m)
    return (F(s4) / F(m)) / ((sq * sq) * (sq * sq))


def f_sdq(jxx, jyy, g):
    return _sqrt((F(jxx) + F(jyy)) / F(g))


def f_direction(jxx, jyy, jxy):
    """step 5: (GRAD_DIR_X, GRAD_DIR_Y, COHERENCE)"""
    jxx, jyy, jxy = F(jxx), F(jyy), F(jxy)
    with np.errstate(all="ignore"):
        hd = (jxx - jyy) / F(2.0)
        rad = _sqrt(hd * hd + jxy * jxy)
        ex, ey = (hd + rad, jxy) if hd >= 0.0 else (jxy, rad - hd)
        gx, gy = F(1.0), F(0.0)
        if not (ex == 0.0 and ey == 0.0):
            n = _sqrt(ex * ex + ey * ey)
            gx, gy = ex / n, ey / n
            if gx < 0.0 or (gx == 0.0 and gy < 0.0):
                gx, gy = -gx, -gy
        return gx, gy, rad / ((jxx + jyy) / F(2.0))


def f_acf(c, n, c0, m):
    with np.errstate(all="ignore"):
        return (F(c) / F(n)) / (F(c0) / F(m))


def height_slope_sums(r, em, clipped, w, s):
    """steps 4 and 5 from a float32 residual box r (read only at em): the integers, the extremes and every raw sum as a Sum"""
    x0, y0 = clipped[0], clipped[1]
    rd = r.astype(np.float64)
    v = rd[em]
    ys, xs = np.nonzero(em)
    flat = (ys + y0).astype(np.int64) * w + (xs + x0)
    r2 = v * v
    out = {"m": int(em.sum()), "s1": Sum(np.abs(v)), "s2": Sum(r2), "s3": Sum(r2 * v), "s4": Sum(r2 * r2)}
    out["sp"], out["sv"] = float(v.max()), float(-v.min())
    out["sp_pixel"], out["sv_pixel"] = int(flat[int(np.argmax(v))]), int(flat[int(np.argmin(v))])
    pad = np.pad(em, 1)
    inner = em & pad[1:-1, :-2] & pad[1:-1, 2:] & pad[:-2, 1:-1] & pad[2:, 1:-1]
    rp = np.pad(rd, 1, constant_values=np.nan)
    s2 = 2.0 * float(s)
    with np.errstate(all="ignore"):
        rx = ((rp[1:-1, 2:] - rp[1:-1, :-2]) / s2)[inner]
        ry = ((rp[2:, 1:-1] - rp[:-2, 1:-1]) / s2)[inner]
        out.update(g=int(inner.sum()), jxx=Sum(rx * rx), jyy=Sum(ry * ry), jxy=Sum(rx * ry), sdr=Sum(np.sqrt((1.0 + rx * rx) + ry * ry) - 1.0))
    return out


def acf_sums(r, em, L):
    """step 6 from a float32 residual box: N [2L+1, 2L+1] and the Sums C of the half plane, {(dx, dy): Sum}"""
    rd = np.where(em, r.astype(np.float64), 0.0)
    bh, bw = em.shape
    N = np.zeros((2 * L + 1, 2 * L + 1), np.int64)
    C = {}
    for dy in range(0, L + 1):
        for dx in range(0 if dy == 0 else -L, L + 1):
            if dy >= bh or abs(dx) >= bw:
                C[(dx, dy)] = Sum([])
                continue
            xa0, xa1 = max(0, -dx), bw - max(0, dx)
            ea, eb = em[0:bh - dy, xa0:xa1], em[dy:bh, xa0 + dx:xa1 + dx]
            both = ea & eb
            C[(dx, dy)] = Sum((rd[0:bh - dy, xa0:xa1] * rd[dy:bh, xa0 + dx:xa1 + dx])[both])
            N[dy + L, dx + L] = N[L - dy, L - dx] = int(both.sum())
    return N, C


def half(dx, dy):
    return (dx, dy) if dy > 0 or (dy == 0 and dx >= 0) else (-dx, -dy)


def acf_window(N, C, m, L):
    need = max(16, m // 8)
    A = np.full((2 * L + 1, 2 * L + 1), np.nan)
    c0 = C[(0, 0)].value
    for dy in range(-L, L + 1):
        for dx in range(-L, L + 1):
            n = int(N[dy + L, dx + L])
            if n >= need:
                A[dy + L, dx + L] = f_acf(C[half(dx, dy)].value, n, c0, m)
    return A


# ---------------------------------------------------------------------------------------------------------------- steps 7 and 8: decisions
def decisions(A, gx, gy, s, L, thr, peak_min):
    """steps 7 and 8 on a window A [2L+1, 2L+1] (NaN = invalid lag) and a direction: the DECISIONS fields, and what they were decided on"""
    D = 2 * L + 1
    A = np.asarray(A, dtype=np.float64)
    valid = ~np.isnan(A)
    out = {name: NAN for name in DECISIONS}
    out["acf_valid_lags"] = float(valid.sum())
    aux = {"profile": [], "lags": [], "lobe": np.zeros((D, D), bool)}
    if not valid[L, L]:
        return out, aux
    with np.errstate(invalid="ignore"):
        above = valid & (A > thr)
    lobe = np.zeros((D, D), bool)
    stack = [(L, L)] if above[L, L] else []
    while stack:
        y, x = stack.pop()
        if lobe[y, x]:
            continue
        lobe[y, x] = True
        for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
            if 0 <= yy < D and 0 <= xx < D and above[yy, xx] and not lobe[yy, xx]:
                stack.append((yy, xx))
    pad = np.pad(lobe, 1)
    dil = (pad[1:-1, :-2] | pad[1:-1, 2:] | pad[:-2, 1:-1] | pad[2:, 1:-1]) & ~lobe
    ring = dil & valid
    is_open = bool((dil & ~valid).any() or lobe[0].any() or lobe[-1].any() or lobe[:, 0].any() or lobe[:, -1].any())
    out["lobe_lags"], out["lobe_status"] = float(lobe.sum()), 1.0 if is_open else 0.0
    aux["lobe"] = lobe
    if ring.any():
        ys, xs = np.nonzero(ring)
        keys = [(int((x - L) ** 2 + (y - L) ** 2), int(y - L), int(x - L)) for y, x in zip(ys, xs)]
        d2, dy, dx = min(key for key in keys if key[1] > 0 or (key[1] == 0 and key[2] >= 0))
        sal, rmax = F(s) * np.sqrt(F(d2)), F(s) * np.sqrt(F(max(key[0] for key in keys)))
        out.update(sal_mm=float(sal), sal_lag_x=float(dx), sal_lag_y=float(dy), rmax_mm=float(rmax), str=float(sal / rmax))
    prof, lags = [F(1.0)], [(0, 0)]
    if math.isfinite(gx) and math.isfinite(gy):
        for j in range(1, L + 1):
            ix, iy = int(math.floor(F(j) * F(gx) + F(0.5))), int(math.floor(F(j) * F(gy) + F(0.5)))
            if abs(ix) > L or abs(iy) > L or not valid[iy + L, ix + L]:
                break
            prof.append(F(A[iy + L, ix + L]))
            lags.append((ix, iy))
    out["profile_samples"] = float(len(prof))
    aux["profile"], aux["lags"] = prof, lags
    below = False
    for j in range(2, L):
        if j + 1 >= len(prof):
            break
        am, a0, ap = prof[j - 1], prof[j], prof[j + 1]
        below = below or bool(am <= thr)
        if am < a0 and a0 >= ap and a0 >= peak_min and below:
            out["pitch_mm"] = float(F(s) * (F(j) + (F(0.5) * (am - ap)) / (am - F(2.0) * a0 + ap)))
            out["pitch_acf"] = float(a0)
            aux["peak"] = j
            break
    return out, aux


# ---------------------------------------------------------------------------------------------------------------- the restatement
def _params(c):
    return c["frac"], c.get("degree", 2), c.get("L", 8), c.get("thr", 0.2), c.get("peak_min", 0.3)


def _row(c, b, k):
    """steps 0 and 1 of row k of frame b of a case"""
    B, h, w = c["index"].shape
    return eval_box(c["depth"][b], c["index"][b], c["tab"][b, k], k, c["eps"], c["frac"], h, w)


def _textures(c, fit, forms_only=False):
    frac, degree, L, thr, peak_min = _params(c)
    B, h, w = c["index"].shape
    K = c["tab"].shape[1]
    tex = np.full((B, K, NTEXTURE), np.nan)
    res = np.full((B, h, w), np.nan, np.float32)
    acf = np.full((B, K, 2 * L + 1, 2 * L + 1), np.nan)
    aux = {}
    for b in range(B):
        s = float(c["mpp"][b])
        for k in range(min(max(int(c["count"][b]), 0), K)):
            o = tex[b, k]
            own, clipped, em, d = _row(c, b, k)
            m = 0 if clipped is None else int(em.sum())
            o[T["eval_pixels"]], o[T["form_status"]] = m, NONE
            coef = None if clipped is None else form(em, d, own, clipped, degree, fit)
            if coef is None:
                continue
            x0, y0, x1, y1 = clipped
            r = residual_box(coef, em, d, own, clipped)
            res[b, y0:y1 + 1, x0:x1 + 1][em] = r[em]
            o[T["form_status"]] = OK
            o[T["form_c0"]:T["form_c0"] + 6] = coef
            if forms_only:
                continue
            hs = height_slope_sums(r, em, clipped, w, s)
            o[T["sp_pixel"]], o[T["sv_pixel"]] = hs["sp_pixel"], hs["sv_pixel"]
            if hs["s2"].value == 0.0:
                o[T["form_status"]] = FLAT
                for name in ("sa_mm", "sq_mm", "sp_mm", "sv_mm", "sz_mm"):
                    o[T[name]] = 0.0
                continue
            o[T["sa_mm"]], o[T["sq_mm"]] = f_sa(hs["s1"].value, m), f_sq(hs["s2"].value, m)
            o[T["ssk"]], o[T["sku"]] = f_ssk(hs["s3"].value, hs["s2"].value, m), f_sku(hs["s4"].value, hs["s2"].value, m)
            o[T["sp_mm"]], o[T["sv_mm"]], o[T["sz_mm"]] = hs["sp"], hs["sv"], F(hs["sp"]) + F(hs["sv"])
            o[T["grad_pixels"]] = hs["g"]
            if hs["g"]:
                o[T["sdq"]], o[T["sdr"]] = f_sdq(hs["jxx"].value, hs["jyy"].value, hs["g"]), F(hs["sdr"].value) / F(hs["g"])
                o[T["grad_dir_x"]], o[T["grad_dir_y"]], o[T["coherence"]] = f_direction(hs["jxx"].value, hs["jyy"].value, hs["jxy"].value)
            N, C = acf_sums(r, em, L)
            A = acf_window(N, C, m, L)
            acf[b, k] = A
            dec, daux = decisions(A, o[T["grad_dir_x"]], o[T["grad_dir_y"]], s, L, thr, peak_min)
            for name, val in dec.items():
                o[T[name]] = val
            aux[(b, k)] = {"N": N, "A": A, "m": m, "decisions": daux}
    return {"textures": tex, "residual": res, "acf": acf, "aux": aux}


def numpy_textures(case):
    """a case (`tcase`) -> {"textures" [B,K,40] f64, "residual" [B,h,w] f32, "acf" [B,K,2L+1,2L+1] f64, "aux"}"""
    return _textures(case, fit_lstsq)


def numpy_textures_ne(case, forms_only=False):
    """the same with the form from the normal equations; forms_only: steps 0 to 3 only (what S1 needs of it)"""
    return _textures(case, fit_normal_equations, forms_only)


def form_distance(case, ta, tb):
    """S1: the largest |P_a - P_b| over the evaluation pixels of any row with a form in tb, relative to the row's peak"""
    worst = 0.0
    for b, k in np.ndindex(tb.shape[:2]):
        if not tb[b, k, T["form_status"]] in (OK, FLAT):
            continue
        own, clipped, em, d = _row(case, b, k)
        u, v = coords(em, own, clipped)
        ca, cb = (t[b, k, T["form_c0"]:T["form_c0"] + 6] for t in (ta, tb))
        worst = max(worst, float(np.abs(poly(ca, u, v) - poly(cb, u, v)).max() / abs(case["tab"][b, k, C_PEAK])))
    return worst


def decision_margin(case, ref=None):
    """The smallest relative distance of any comparison of the case's decisions (steps 6 to 8 of the pure restatement) from flipping: A
    against the two thresholds, the profile's neighbours against each other, j*G + 0.5 against the next integer, N against the validity
    count.  inf for a case that decides nothing."""
    frac, degree, L, thr, peak_min = _params(case)
    ref = ref or numpy_textures(case)
    worst = float("inf")
    for (b, k), a in ref["aux"].items():
        A, N, m = a["A"], a["N"], a["m"]
        need = max(16, m // 8)
        worst = min(worst, float(np.abs(N - (need - 0.5)).min() / need))
        v = A[~np.isnan(A)]
        if v.size:
            worst = min(worst, float(np.abs(v - thr).min() / thr))
        prof, lags = [float(p) for p in a["decisions"]["profile"]], a["decisions"]["lags"]
        for j in range(1, len(prof)):
            worst = min(worst, abs(prof[j] - peak_min) / peak_min)
            if lags[j] != lags[j - 1]:                                     # two samples of one lag are equal on every side
                worst = min(worst, abs(prof[j] - prof[j - 1]) / max(abs(prof[j]), abs(prof[j - 1])))
        gx, gy = ref["textures"][b, k, T["grad_dir_x"]], ref["textures"][b, k, T["grad_dir_y"]]
        if math.isfinite(gx) and math.isfinite(gy):
            for j in range(1, L + 1):
                for g in (gx, gy):
                    t = j * g + 0.5
                    worst = min(worst, abs(t - round(t)) if abs(t - round(t)) > 0 else 1.0)
    return worst


# ---------------------------------------------------------------------------------------------------------------- holding the device
def _within(got, fn, sums, what, extra=0.0):
    """S3 for a field built from sums: fn at the corners of the sums' intervals, 8 ulp for its own roundings"""
    vals = [fn(*corner) for corner in itertools.product(*[s.ends(extra) for s in sums])] + [fn(*[s.value for s in sums])]
    vals = [float(v) for v in vals]
    if any(math.isnan(v) for v in vals):
        assert all(math.isnan(v) for v in vals) and math.isnan(got), (what, got, vals)
        return
    lo, hi = min(vals), max(vals)
    slack = 8.0 * ULP * max(abs(lo), abs(hi))
    assert lo - slack <= got <= hi + slack, (what, got, lo, hi, slack)


def hold_device(case, got, ref=None, ne=None):
    """S1 to S4 for what the device returned for a case: got = {"textures", "residual", "acf"} as NumPy arrays.  ref, ne: the two
    restatements when they are at hand (S1 needs them; without them S1 is left to the caller)."""
    frac, degree, L, thr, peak_min = _params(case)
    tex, res, acf = got["textures"], got["residual"], got["acf"]
    B, h, w = case["index"].shape
    K = case["tab"].shape[1]
    assert tex.shape == (B, K, NTEXTURE) and tex.dtype == np.float64 and res.shape == (B, h, w) and res.dtype == np.float32
    assert acf.shape == (B, K, 2 * L + 1, 2 * L + 1) and acf.dtype == np.float64
    assert np.isnan(tex[..., len(FIELDS):]).all()
    want_res = np.full((B, h, w), np.nan, np.float32)
    for b in range(B):
        s = float(case["mpp"][b])
        kk = min(max(int(case["count"][b]), 0), K)
        assert np.isnan(tex[b, kk:]).all() and np.isnan(acf[b, kk:]).all(), b
        for k in range(kk):
            o, where = tex[b, k], (b, k)
            own, clipped, em, d = _row(case, b, k)
            m = 0 if clipped is None else int(em.sum())
            assert o[T["eval_pixels"]] == m, where
            status = int(o[T["form_status"]])
            if ref is not None:
                assert status == ref["textures"][b, k, T["form_status"]], where
            if status == NONE:
                assert clipped is None or form(em, d, own, clipped, degree, fit_lstsq) is None, where
                assert np.isnan(np.delete(o, [T["eval_pixels"], T["form_status"]])).all() and np.isnan(acf[b, k]).all(), where
                continue
            x0, y0, x1, y1 = clipped
            coef = o[T["form_c0"]:T["form_c0"] + 6]
            assert np.isfinite(coef).all() and (coef[NTERMS[degree]:] == 0.0).all(), where
            # S2
            rbox = residual_box(coef, em, d, own, clipped)
            want_res[b, y0:y1 + 1, x0:x1 + 1][em] = rbox[em]
            r = res[b, y0:y1 + 1, x0:x1 + 1]
            assert same_bits(r[em], rbox[em]), (where, "residual")
            # S3 from the device's own plane
            hs = height_slope_sums(r, em, clipped, w, s)
            assert o[T["sp_pixel"]] == hs["sp_pixel"] and o[T["sv_pixel"]] == hs["sv_pixel"], where
            if hs["s2"].value == 0.0:
                assert status == FLAT and all(o[T[n]] == 0.0 for n in ("sa_mm", "sq_mm", "sp_mm", "sv_mm", "sz_mm")), where
                assert np.isnan(o[[T["ssk"], T["sku"]]]).all() and np.isnan(o[T["grad_pixels"]:]).all() and np.isnan(acf[b, k]).all(), where
                continue
            assert status == OK, where
            assert o[T["sp_mm"]] == hs["sp"] and o[T["sv_mm"]] == hs["sv"] and o[T["sz_mm"]] == F(hs["sp"]) + F(hs["sv"]), where
            _within(o[T["sa_mm"]], lambda a: f_sa(a, m), [hs["s1"]], (where, "sa"))
            _within(o[T["sq_mm"]], lambda a: f_sq(a, m), [hs["s2"]], (where, "sq"))
            _within(o[T["ssk"]], lambda a, q: f_ssk(a, q, m), [hs["s3"], hs["s2"]], (where, "ssk"))
            _within(o[T["sku"]], lambda a, q: f_sku(a, q, m), [hs["s4"], hs["s2"]], (where, "sku"))
            g = hs["g"]
            assert o[T["grad_pixels"]] == g, where
            if g == 0:
                assert np.isnan(o[T["sdq"]:T["coherence"] + 1]).all(), where
            else:
                js = [hs["jxx"], hs["jyy"], hs["jxy"]]
                _within(o[T["sdq"]], lambda a, q: f_sdq(a, q, g), js[:2], (where, "sdq"))
                _within(o[T["sdr"]], lambda a: F(a) / F(g), [hs["sdr"]], (where, "sdr"))
                _within(o[T["coherence"]], lambda a, q, p: f_direction(a, q, p)[2], js, (where, "coherence"))
                gx, gy = o[T["grad_dir_x"]], o[T["grad_dir_y"]]
                assert gx > 0.0 or (gx == 0.0 and gy > 0.0), where                  # the sign rule; the value is held up to that sign

                def turned(i):
                    def f(a, q, p):
                        v = f_direction(a, q, p)
                        return v[i] if v[0] * gx + v[1] * gy >= 0.0 else -v[i]
                    return f
                _within(gx, turned(0), js, (where, "grad_dir_x"))
                _within(gy, turned(1), js, (where, "grad_dir_y"))
            N, C = acf_sums(r, em, L)
            need = max(16, m // 8)
            A = acf[b, k]
            assert np.array_equal(~np.isnan(A), N >= need), (where, "valid lags")
            assert same_bits(A, A[::-1, ::-1].copy()), (where, "mirror")
            assert o[T["acf_valid_lags"]] == int((N >= need).sum()), where
            for dy in range(0, L + 1):
                for dx in range(0 if dy == 0 else -L, L + 1):
                    n = int(N[dy + L, dx + L])
                    if n >= need:
                        _within(A[dy + L, dx + L], lambda a, q: f_acf(a, n, q, m), [C[(dx, dy)], C[(0, 0)]], (where, "acf", dx, dy))
            if N[L, L] >= need:
                assert A[L, L] == 1.0, where
            # S4 on the device's own window and direction
            dec, _ = decisions(A, o[T["grad_dir_x"]], o[T["grad_dir_y"]], s, L, thr, peak_min)
            for name in DECISIONS:
                assert same(o[T[name]], dec[name]), (where, name, o[T[name]], dec[name])
    # the NaN pattern of the plane, and every bit of it
    assert np.array_equal(np.isnan(res), np.isnan(want_res)) and same_bits(res[~np.isnan(res)], want_res[~np.isnan(want_res)])
    # S1
    if ref is not None:
        e_ne = form_distance(case, ne["textures"], ref["textures"])
        bar = max(4.0 * e_ne, 64.0 * ULP)
        e = form_distance(case, tex, ref["textures"])
        print("S1 form distance", e, "bar", bar, "e_ne", e_ne)
        assert e <= bar, (e, bar)


def hold_end_to_end(case, got, ref):
    """S5: the decision fields against the pure restatement, for a case whose `decision_margin` is at least 1e-9.  What is decided on
    integers (counts, the lobe, lags, and SAL, RMAX, STR, which are functions of lags and s) is equal.  PITCH_ACF is a sample of A and
    PITCH_MM the vertex of the parabola through three of them: they are held as S3 holds A, with the sums' intervals widened by what the two
    sides' residuals may differ in -- where the two forms round d - P to different float32 neighbours a residual moves by one step, 2^-23 of
    itself at most, so a product of two by 2^-22 of itself (the forms themselves differ by S1's bar, far below a float32 step)."""
    frac, degree, L, thr, peak_min = _params(case)
    tex, want = got["textures"], ref["textures"]
    for name in DECISIONS:
        if name not in ("pitch_mm", "pitch_acf"):
            assert same(tex[..., T[name]], want[..., T[name]]), (name, tex[..., T[name]], want[..., T[name]])
    assert np.array_equal(np.isnan(tex[..., T["pitch_mm"]]), np.isnan(want[..., T["pitch_mm"]]))
    for (b, k), a in ref["aux"].items():
        if "peak" not in a["decisions"]:
            continue
        own, clipped, em, d = _row(case, b, k)
        x0, y0, x1, y1 = clipped
        N, C = acf_sums(ref["residual"][b, y0:y1 + 1, x0:x1 + 1], em, L)
        j, lags, m, s = a["decisions"]["peak"], a["decisions"]["lags"], a["m"], F(case["mpp"][b])
        three = [lags[j - 1], lags[j], lags[j + 1]]
        ns = [int(N[t[1] + L, t[0] + L]) for t in three]

        def pitch(cm, cc, cp, cz):
            am, ac, ap = (f_acf(c, n, cz, m) for c, n in zip((cm, cc, cp), ns))
            return s * (F(j) + (F(0.5) * (am - ap)) / (am - F(2.0) * ac + ap))
        print("S5 pitch", (b, k), tex[b, k, T["pitch_mm"]], want[b, k, T["pitch_mm"]], "acf", tex[b, k, T["pitch_acf"]], want[b, k, T["pitch_acf"]])
        _within(tex[b, k, T["pitch_mm"]], pitch, [C[half(*t)] for t in three] + [C[(0, 0)]], ((b, k), "pitch_mm"), extra=2.0 ** -22)
        _within(tex[b, k, T["pitch_acf"]], lambda cc, cz: f_acf(cc, ns[1], cz, m), [C[half(*three[1])], C[(0, 0)]], ((b, k), "pitch_acf"), extra=2.0 ** -22)


# ---------------------------------------------------------------------------------------------------------------- scenes
def tcase(scenes, K, s, frac=0.5, degree=2, L=8, thr=0.2, peak_min=0.3, count=None):
    c = pack(scenes, K, s, frac, count=count)
    c.update(degree=degree, L=L, thr=thr, peak_min=peak_min)
    return c


def args(c):
    """the arguments of contact_textures for a case"""
    return (c["depth"], c["index"], c["tab"], c["count"], c["mpp"], c["eps"]), dict(eval_min_fraction=c["frac"], form_degree=c["degree"], max_lag=c["L"],
                                                                                    acf_threshold=c["thr"], peak_min=c["peak_min"])


RIDGE_PHIS = (0.0, 30.0, -75.0, 90.0)
CAP = dict(xa=26.37, ya=18.21, d0=1.25, r1=18.0, r2=41.0, s=0.23)


def ridges(phi_deg, h=H, w=W, amp=0.02, pitch=6.0, radius=14.0):
    """the analytic cap of the shape tests plus amp * sin(2 pi ((x-xa) cos phi + (y-ya) sin phi) / pitch) on a disc"""
    phi = np.deg2rad(phi_deg)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    d = quadric(h, w, CAP["xa"], CAP["ya"], CAP["d0"], CAP["r1"], CAP["r2"], 0.0, CAP["s"])
    d = d + amp * np.sin(2.0 * np.pi * ((xx - CAP["xa"]) * np.cos(phi) + (yy - CAP["ya"]) * np.sin(phi)) / pitch)
    return Scene(h, w, 0.0).paint(0, disc(h, w, 26, 18, radius), d)


def _textured(h, w, seed, base=0.6, amp=0.03, pitch=5.0, phi=0.6, noise=0.004):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    return base + amp * np.sin(2.0 * np.pi * (xx * np.cos(phi) + yy * np.sin(phi)) / pitch) + rng.normal(0.0, noise, (h, w))


def cases():
    """every direct case by name"""
    h, w = H, W
    c = {}
    for phi in RIDGE_PHIS:
        c["ridges_%g" % phi] = tcase([ridges(phi)], 4, CAP["s"])
    c["ridges_30_lag_4"] = tcase([ridges(30.0)], 4, CAP["s"], L=4)
    rng = np.random.default_rng(7)
    c["white_noise"] = tcase([Scene(h, w, 0.0).paint(0, disc(h, w, 26, 18, 14.0), 0.5 + rng.normal(0.0, 0.01, (h, w)))], 4, 0.2)
    # a contact in the corner; the table's box reaches beyond the frame, so it is clipped and lags leave the frame
    edge = tcase([Scene(h, w, 0.0).paint(0, disc(h, w, 3, 2, 11.0), _textured(h, w, 11))], 4, 0.2)
    edge["tab"][0, 0, [C_X0, C_Y0]] -= 6.0
    c["frame_edge"] = edge
    nb = Scene(h, w, 0.0).paint(0, rect(h, w, 5, 4, 20, 22), _textured(h, w, 12)).paint(1, rect(h, w, 21, 4, 34, 22), _textured(h, w, 13, base=0.5))
    nb.paint(2, disc(h, w, 43, 24, 9.0, 4.0), _textured(h, w, 14, base=0.4, pitch=4.0))
    c["neighbours_and_ring"] = tcase([nb], 4, 0.2, frac=0.0)
    sm = Scene(h, w, 0.0).paint(0, rect(h, w, 4, 3, 23, 5), _textured(h, w, 15)).paint(1, rect(h, w, 30, 10, 30, 10), 0.5)
    five = np.zeros((h, w), bool)
    five[[20, 19, 21, 20, 20], [10, 10, 10, 9, 11]] = True
    sm.paint(2, five, _textured(h, w, 16, base=0.45)).paint(3, rect(h, w, 28, 30, 49, 30), _textured(h, w, 17, base=0.4))
    c["small_degree_2"] = tcase([sm], 4, 0.2, frac=0.0)
    c["small_degree_0"] = tcase([sm], 4, 0.2, frac=0.0, degree=0)
    c["flat"] = tcase([Scene(h, w, 0.0).paint(0, rect(h, w, 10, 10, 17, 17), 0.5)], 4, 0.2, degree=0)
    # the table's edge cases: count 0, count > K, NaN and infinite depths, a box that is not finite, plane values nobody owns
    base = Scene(h, w, 0.0).paint(0, disc(h, w, 14, 12, 8.5), _textured(h, w, 18)).paint(1, disc(h, w, 36, 24, 7.5), _textured(h, w, 19, base=0.5))
    base.paint(2, rect(h, w, 30, 2, 40, 9), _textured(h, w, 20)).paint(5, rect(h, w, 45, 28, 50, 34), 0.9)
    holes = Scene(h, w, 0.0).paint(0, disc(h, w, 14, 12, 8.5), _textured(h, w, 18)).paint(1, disc(h, w, 36, 24, 7.5), _textured(h, w, 19, base=0.5))
    holes.depth[10:13, 12:15] = np.nan
    holes.depth[24, 36] = np.inf
    nobox = Scene(h, w, 0.0).paint(0, disc(h, w, 14, 12, 8.5), _textured(h, w, 18)).paint(1, disc(h, w, 36, 24, 7.5), _textured(h, w, 19, base=0.5))
    t = tcase([base, base, base, holes, nobox], 3, [0.2, 0.25, 0.3, 0.2, 0.22], frac=0.25, count=[2, 0, 7, 2, 2])
    t["tab"][4, 0, C_X1] = np.inf
    t["tab"][4, 1, C_Y0] = np.nan
    c["table_edges"] = t
    tex = Scene(h, w, 0.0).paint(0, disc(h, w, 26, 18, 15.0), quadric(h, w, 25.6, 18.3, 1.1, 25.0, 35.0, 0.3, 0.2) + _textured(h, w, 21, base=0.0))
    c["lag_2"] = tcase([tex], 4, 0.2, L=2)
    c["lag_31"] = tcase([tex], 4, 0.2, L=31)
    c["degree_0"] = tcase([tex], 4, 0.2, degree=0)
    c["degree_1"] = tcase([tex], 4, 0.2, degree=1)
    c["all_pixels"] = tcase([tex], 4, 0.2, frac=0.0)
    c["five_frames"] = tcase([ridges(30.0), nb, sm, tex, base], 4, [0.23, 0.2, 0.2, 0.2, 0.21], frac=0.25, count=[1, 3, 4, 1, 2])
    return c


CASE_NAMES = ("ridges_0", "ridges_30", "ridges_-75", "ridges_90", "ridges_30_lag_4", "white_noise", "frame_edge", "neighbours_and_ring",
              "small_degree_2", "small_degree_0", "flat", "table_edges", "lag_2", "lag_31", "degree_0", "degree_1", "all_pixels", "five_frames")


def native_case(n=1182, s=0.05):
    """one native-size frame: a 3 x 1100 strip (a box wider than a workgroup, the longest ACF rows) and a disc of radius 100; L = 16"""
    sc = Scene(n, n)
    yy, xx = np.mgrid[0:n, 0:n].astype(np.float64)
    rng = np.random.default_rng(31)
    wave = 0.03 * np.sin(2.0 * np.pi * (xx * np.cos(0.4) + yy * np.sin(0.4)) / 9.0) + rng.normal(0.0, 0.003, (n, n))
    sc.paint(0, disc(n, n, 640, 500, 100.0), quadric(n, n, 641.3, 498.6, 2.4, 60.0, 45.0, 0.8, s) + wave)
    sc.paint(1, rect(n, n, 40, 1100, 1139, 1102), 1.5 + wave)
    return tcase([sc], 4, s, L=16)
