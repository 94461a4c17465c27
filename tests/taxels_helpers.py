"""Inputs, the two restatements of the taxel read-out (include/vistaf_taxel.h) and the derived bar for tests/test_taxels.py.

`numpy_taxels` is the definition written out plainly, one Python loop per taxel, every sum through `math.fsum` (correctly rounded).
`numpy_taxels_vec` is a second, vectorised restatement (`np.add.at`, `np.maximum.at`) that shares no code with the first.

THE BAR on a float field is derived, not measured.  The terms of S, Sx and Sy are non-negative (the contact depths of the cases are
positive) and the products x*d, y*d are exact in float64, so a sum of N such terms formed in any order lies within (N - 1) * 2^-53 of the
true sum, relatively; the frame sums add taxel sums, and adding the +0 of a taxel without contact is exact, so they too are sums of the
frame's N contact-pixel terms in some order.  A quotient of two such sums and the handful of roundings of the closing arithmetic stay within
(2 N + 16) * 2^-53, N = the FRAME's number of contact pixels, of the correctly rounded reference -- relative to the field's own scale: the
reference value for areas, volumes, mean depths, forces and pressures; max(h, w) for centroids and the centre of pressure;
|F| * max(h, w) * s for the moments.  Pixel counts, MAX_DEPTH_MM, ARGMAX_INDEX, ACTIVE_TAXELS, PEAK_TAXEL and the NaN pattern are exact.
"""
import math

import numpy as np

FIELDS = ("contact_pixels", "contact_area_mm2", "volume_cm3", "mean_depth_mm", "max_depth_mm", "argmax_index", "centroid_x", "centroid_y",
          "force_N", "pressure_kPa")
FRAME_FIELDS = ("active_taxels", "volume_cm3", "force_N", "cop_x", "cop_y", "moment_x_Nmm", "moment_y_Nmm", "peak_taxel")
T_ = {n: i for i, n in enumerate(FIELDS)}
F_ = {n: i for i, n in enumerate(FRAME_FIELDS)}
NTAXEL, NFRAME, NONE = 12, 8, 0xFFFF
EXACT, FRAME_EXACT = ("contact_pixels", "max_depth_mm", "argmax_index"), ("active_taxels", "peak_taxel")
OWN_SCALE, FRAME_OWN_SCALE = ("contact_area_mm2", "volume_cm3", "mean_depth_mm", "force_N", "pressure_kPa"), ("volume_cm3", "force_N")
U = 2.0 ** -53
H, W = 37, 53                   # base shape: P = 1961 is odd, every frame of a batch starts at another misalignment
EPS = 0.01


def _div(a, b):
    """IEEE a / b for Python floats (0/0 and x/0 included)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


# ---------------------------------------------------------------------------------------------------------------- the definition
def numpy_taxels(depth, tmap, n_taxels, origin, mpp, eps, force=None, status=None):
    """(taxels [B,T,12], frame [B,8]) float64 by the header's definition."""
    depth = np.asarray(depth, dtype=np.float32)
    B, h, w = depth.shape
    T = int(n_taxels)
    flat = np.asarray(tmap).ravel()
    order = np.argsort(flat, kind="stable")                    # the pixels of a taxel in row-major order
    bounds = np.searchsorted(flat[order], np.arange(T + 1))
    lists = [order[bounds[t]:bounds[t + 1]] for t in range(T)]
    e32 = np.float32(eps)
    tax, frm = np.full((B, T, NTAXEL), np.nan), np.full((B, NFRAME), np.nan)
    for b in range(B):
        if status is not None and int(status[b]) != 0:
            continue
        d = depth[b].ravel().copy()
        d[np.isnan(d)] = np.float32(0.0)
        s = float(mpp[b])
        px = s * s
        Fb = float(force[b]) if force is not None else math.nan
        S_t, Sx_t, Sy_t = [], [], []
        for t in range(T):
            idx = lists[t]
            dv = d[idx]
            c = dv > e32
            ci, dc = idx[c], dv[c].astype(np.float64)
            n, L = int(c.sum()), int(idx.size)
            S = math.fsum(dc.tolist())
            Sx = math.fsum(((ci % w).astype(np.float64) * dc).tolist())
            Sy = math.fsum(((ci // w).astype(np.float64) * dc).tolist())
            S_t.append(S), Sx_t.append(Sx), Sy_t.append(Sy)
            row = tax[b, t]
            row[T_["contact_pixels"]] = n
            row[T_["contact_area_mm2"]] = n * px
            row[T_["volume_cm3"]] = S * px / 1000.0
            row[T_["mean_depth_mm"]] = S / L if L else math.nan
            row[T_["max_depth_mm"]] = float(dc.max()) if n else 0.0
            if n:
                row[T_["argmax_index"]] = int(ci[int(np.argmax(dc))])          # first occurrence
                row[T_["centroid_x"]], row[T_["centroid_y"]] = _div(Sx, S), _div(Sy, S)
        Sf, Sxf, Syf = math.fsum(S_t), math.fsum(Sx_t), math.fsum(Sy_t)
        for t in range(T):
            L = int(lists[t].size)
            share = math.nan if force is None else (0.0 if Sf == 0.0 else Fb * (S_t[t] / Sf))
            tax[b, t, T_["force_N"]] = share
            tax[b, t, T_["pressure_kPa"]] = 1000.0 * share / (L * px) if L else math.nan
        active = [t for t in range(T) if tax[b, t, 0] > 0]
        cx, cy = (_div(Sxf, Sf), _div(Syf, Sf)) if Sf != 0.0 else (math.nan, math.nan)
        frm[b, F_["active_taxels"]] = len(active)
        frm[b, F_["volume_cm3"]] = Sf * px / 1000.0
        frm[b, F_["force_N"]] = Fb
        frm[b, F_["cop_x"]], frm[b, F_["cop_y"]] = cx, cy
        frm[b, F_["moment_x_Nmm"]] = Fb * (cy - origin[1]) * s
        frm[b, F_["moment_y_Nmm"]] = -(Fb * (cx - origin[0]) * s)
        if active:
            frm[b, F_["peak_taxel"]] = max(active, key=lambda t: (tax[b, t, T_["max_depth_mm"]], -t))
    return tax, frm


def numpy_taxels_vec(depth, tmap, n_taxels, origin, mpp, eps, force=None, status=None):
    """The same definition, vectorised: scatter-adds over the frame instead of a loop over taxels."""
    depth = np.asarray(depth, dtype=np.float32)
    B, h, w = depth.shape
    T = int(n_taxels)
    lab = np.asarray(tmap).ravel().astype(np.int64)
    has = lab != NONE
    L = np.bincount(lab[has], minlength=T).astype(np.float64)
    yy, xx = np.divmod(np.arange(h * w), w)
    tax, frm = np.full((B, T, NTAXEL), np.nan), np.full((B, NFRAME), np.nan)
    with np.errstate(all="ignore"):
        for b in range(B):
            if status is not None and int(status[b]) != 0:
                continue
            d = np.nan_to_num(depth[b].ravel(), nan=0.0, posinf=np.inf, neginf=-np.inf)
            c = has & (d > np.float32(eps))
            lc, dc, pc = lab[c], d[c].astype(np.float64), np.flatnonzero(c)
            n = np.bincount(lc, minlength=T).astype(np.float64)
            S, Sx, Sy = np.zeros(T), np.zeros(T), np.zeros(T)
            np.add.at(S, lc, dc)
            np.add.at(Sx, lc, xx[c] * dc)
            np.add.at(Sy, lc, yy[c] * dc)
            mx = np.full(T, -np.inf)
            np.maximum.at(mx, lc, dc)
            first = np.full(T, h * w, dtype=np.int64)
            at = dc == mx[lc]
            np.minimum.at(first, lc[at], pc[at])
            s = float(mpp[b])
            px = s * s
            on = n > 0
            Sf, Sxf, Syf = S.sum(), Sx.sum(), Sy.sum()
            Fb = float(force[b]) if force is not None else np.nan
            r = tax[b]
            r[:, 0], r[:, 1], r[:, 2] = n, n * px, S * px / 1000.0
            r[:, 3] = np.where(L > 0, S / L, np.nan)
            r[:, 4] = np.where(on, mx, 0.0)
            r[:, 5] = np.where(on, first, np.nan)
            r[:, 6], r[:, 7] = np.where(on, Sx / S, np.nan), np.where(on, Sy / S, np.nan)
            r[:, 8] = np.nan if force is None else (0.0 if Sf == 0.0 else Fb * (S / Sf))
            r[:, 9] = np.where(L > 0, 1000.0 * r[:, 8] / (L * px), np.nan)
            cx, cy = (Sxf / Sf, Syf / Sf) if Sf != 0.0 else (np.nan, np.nan)
            peak = np.nan
            if on.any():
                best = np.where(on, mx, -np.inf)
                peak = int(np.flatnonzero(best == best.max())[0])
            frm[b] = [on.sum(), Sf * px / 1000.0, Fb, cx, cy, Fb * (cy - origin[1]) * s, -(Fb * (cx - origin[0]) * s), peak]
    return tax, frm


# ---------------------------------------------------------------------------------------------------------------- comparison
def frame_contact_pixels(want_tax):
    """N of every frame from the reference rows (0 for a NaN frame)"""
    return np.nan_to_num(want_tax[..., 0], nan=0.0).sum(axis=1)


def exact_equal(got, want):
    """pixel counts, maxima, arg-max indices, active taxels, peak taxel and the NaN pattern of (taxels, frame)"""
    (gt, gf), (wt, wf) = got, want
    if gt.shape != wt.shape or gf.shape != wf.shape or not np.array_equal(np.isnan(gt), np.isnan(wt)) or not np.array_equal(np.isnan(gf), np.isnan(wf)):
        return False
    return all(np.array_equal(gt[..., T_[k]], wt[..., T_[k]], equal_nan=True) for k in EXACT) and \
        all(np.array_equal(gf[..., F_[k]], wf[..., F_[k]], equal_nan=True) for k in FRAME_EXACT)


def worst_excess(got, want, mpp, shape):
    """Largest |got - want| / (bar * scale) over the float fields and frames (<= 1 passes), with the field it occurs in.  NaNs are compared by
    `exact_equal`; a field whose scale is 0 must be equal."""
    (gt, gf), (wt, wf) = got, want
    B = wt.shape[0]
    N = frame_contact_pixels(wt)
    span = float(max(shape))
    worst, where = 0.0, None

    def see(g, w_, scale, bar, name, b):
        nonlocal worst, where
        g, w_, scale = np.broadcast_arrays(np.asarray(g, float), np.asarray(w_, float), np.asarray(scale, float))
        ok = ~np.isnan(w_)
        if not ok.any():
            return
        err, sc = np.abs(g[ok] - w_[ok]), np.abs(scale[ok]) * bar
        with np.errstate(all="ignore"):
            ratio = np.where(err == 0.0, 0.0, np.where(sc > 0.0, err / sc, np.inf))
        if ratio.max() > worst:
            worst, where = float(ratio.max()), (name, b)

    for b in range(B):
        if np.isnan(wf[b, 0]):
            continue
        bar = (2.0 * N[b] + 16.0) * U
        s = float(mpp[b])
        for k in OWN_SCALE:
            see(gt[b, :, T_[k]], wt[b, :, T_[k]], wt[b, :, T_[k]], bar, k, b)
        for k in ("centroid_x", "centroid_y"):
            see(gt[b, :, T_[k]], wt[b, :, T_[k]], span, bar, k, b)
        for k in FRAME_OWN_SCALE:
            see(gf[b, F_[k]], wf[b, F_[k]], wf[b, F_[k]], bar, "frame " + k, b)
        for k in ("cop_x", "cop_y"):
            see(gf[b, F_[k]], wf[b, F_[k]], span, bar, "frame " + k, b)
        for k in ("moment_x_Nmm", "moment_y_Nmm"):
            see(gf[b, F_[k]], wf[b, F_[k]], abs(wf[b, F_["force_N"]]) * span * s, bar, "frame " + k, b)
    return worst, where


# ---------------------------------------------------------------------------------------------------------------- layouts (plain maps)
def grid_map(h, w, rows, cols):
    return np.array([[(y * rows // h) * cols + x * cols // w for x in range(w)] for y in range(h)], dtype=np.uint16)


def polar_map(h, w, circle, rings, sectors):
    """pixel by pixel, in Python floats"""
    cx, cy, r = circle
    m = np.full((h, w), NONE, dtype=np.uint16)
    for y in range(h):
        for x in range(w):
            dx, dy = x - cx, y - cy
            if dx * dx + dy * dy <= r * r:
                ring = min(int(math.floor(math.sqrt(dx * dx + dy * dy) * rings / r)), rings - 1)
                a = math.atan2(dy, dx)
                a = a + 2.0 * math.pi if a < 0 else a
                m[y, x] = ring * sectors + min(int(math.floor(a * sectors / (2.0 * math.pi))), sectors - 1)
    return m


CIRCLE = (26, 18, 17)


def layouts():
    """name -> (map, n_taxels, origin) at the base shape"""
    yy, xx = np.mgrid[0:H, 0:W]
    holes = np.full((H, W), NONE, dtype=np.uint16)              # ids 0, 2, 5, 7 of 9 used, the rest of the frame no taxel
    holes[2:20, 3:30] = 2
    holes[5:9, 8:14] = NONE
    holes[15:33, 25:50] = 7
    holes[0:2, :] = 0
    holes[30:37, 0:10] = 5
    holes[16:19, 26:29] = 0                                      # a disconnected part of taxel 0 inside 7
    return {
        "grid_4x5": (grid_map(H, W, 4, 5), 20, ((W - 1) / 2.0, (H - 1) / 2.0)),
        "polar_3x8": (polar_map(H, W, CIRCLE, 3, 8), 24, (float(CIRCLE[0]), float(CIRCLE[1]))),
        "whole_frame": (np.zeros((H, W), np.uint16), 1, (0.0, 0.0)),
        "per_pixel": (np.arange(H * W, dtype=np.uint16).reshape(H, W), H * W, (30.25, -4.5)),
        "checkerboard": (((yy + xx) % 2).astype(np.uint16), 2, ((W - 1) / 2.0, (H - 1) / 2.0)),
        "holes_unused": (holes, 9, (20.0, 20.0)),
    }


# ---------------------------------------------------------------------------------------------------------------- planes
def bump(h, w, x0, y0, amp, sig):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    return amp * np.exp(-((xx - x0) ** 2 + (yy - y0) ** 2) / (2.0 * sig * sig))


def base_planes():
    """The five frames of the base shape: (depth [5,H,W] float32, mm_per_px, force_N, status)."""
    e32 = np.float32(EPS)
    up = np.nextafter(e32, np.float32(np.inf), dtype=np.float32)
    rng = np.random.default_rng(20240611)
    d = np.zeros((5, H, W), np.float32)
    # 0: empty -- zeros, a NaN border, nothing above eps
    d[0, 0, :] = np.nan
    d[0, :, 0] = np.nan
    # 1: one bump, NaN patches inside and beside it, negative values elsewhere
    d[1] = bump(H, W, 30.3, 14.6, 0.8, 5.0).astype(np.float32)
    d[1, 12:15, 31:34] = np.nan
    d[1, 30:35, 2:9] = np.nan
    d[1, 25:30, 40:50] = -0.4
    # 2: several bumps, pixels exactly at eps and one float32 step above it, a plateau that ties the maximum across cells
    d[2] = (bump(H, W, 8.2, 9.1, 0.5, 3.0) + bump(H, W, 44.0, 28.5, 0.7, 4.0) + bump(H, W, 45.5, 5.0, 0.3, 2.0)).astype(np.float32)
    d[2, 15:23, 20:28] = np.float32(0.75)                         # the maximum: grid columns 1|2 and rows 1|2, several sectors, both colours
    d[2, 33, 5:25:2] = e32
    d[2, 33, 6:25:2] = up
    d[2, 35, 0:53:3] = up
    d[2, 36, 52] = e32
    # 3: status != 0 -- garbage, infinities included
    d[3] = (rng.standard_normal((H, W)) * 1e30).astype(np.float32)
    d[3, ::3, ::5] = np.inf
    d[3, 1::4, 2::7] = -np.inf
    d[3, 5, 5] = np.nan
    # 4: several bumps on a noisy floor below eps, negative pixels, a NaN row
    d[4] = (bump(H, W, 26.0, 18.0, 1.1, 6.0) + bump(H, W, 3.0, 33.0, 0.4, 2.5) + bump(H, W, 50.0, 2.0, 0.6, 1.5)).astype(np.float32)
    d[4] += (rng.uniform(-0.02, 0.009, (H, W))).astype(np.float32) * (d[4] < 0.001)
    d[4, 20, :] = np.nan
    return d, np.array([0.05, 0.0493, 0.0512, 0.05, 0.0478]), np.array([0.37, 1.25, 2.5, 7.0, 3.75]), np.array([0, 0, 0, 2, 0], np.int32)


def strip_planes():
    """3 x 1100, B = 2: a long ridge and scattered single pixels"""
    h, w = 3, 1100
    d = np.zeros((2, h, w), np.float32)
    d[0] = (0.3 + 0.2 * np.sin(np.arange(w) / 37.0))[None, :].astype(np.float32) * np.array([[1.0], [0.5], [0.02]], np.float32)
    d[1, 1, ::97] = 0.6
    d[1, 2, 1099] = 0.6
    d[1, 0, 5:9] = np.nan
    return d, np.array([0.05, 0.051]), np.array([1.5, 0.25]), np.array([0, 0], np.int32)


def big_planes():
    """1182 x 1182, B = 2: a few wide bumps, NaN outside a disc"""
    n = 1182
    yy, xx = np.mgrid[0:n, 0:n].astype(np.float32)
    out = (xx - 590.5) ** 2 + (yy - 590.5) ** 2 > 560.0 ** 2

    def g(x0, y0, amp, sig):
        return amp * np.exp(-((xx - np.float32(x0)) ** 2 + (yy - np.float32(y0)) ** 2) / np.float32(2.0 * sig * sig))
    d = np.stack([g(400.0, 500.0, 1.2, 60.0) + g(800.0, 700.0, 0.8, 40.0), g(591.0, 591.0, 2.0, 90.0) + g(300.0, 900.0, 0.5, 25.0)]).astype(np.float32)
    d[:, out] = np.nan
    return d, np.array([0.0196, 0.0201]), np.array([4.0, 9.5]), np.array([0, 0], np.int32)


def cases():
    """name -> dict(depth, map, T, origin, mpp, force, status, eps): the six layouts on the five base frames, the strip and the native size"""
    out = {}
    d, mpp, force, status = base_planes()
    for name, (m, T, origin) in layouts().items():
        out[name] = dict(depth=d, map=m, T=T, origin=origin, mpp=mpp, force=force, status=status, eps=EPS)
    d, mpp, force, status = strip_planes()
    out["strip_3x1100"] = dict(depth=d, map=np.zeros((3, 1100), np.uint16), T=1, origin=(549.5, 1.0), mpp=mpp, force=force, status=status, eps=EPS)
    d, mpp, force, status = big_planes()
    out["big_1182_grid_16x16"] = dict(depth=d, map=grid_map_fast(1182, 1182, 16, 16), T=256, origin=(590.5, 590.5), mpp=mpp, force=force,
                                      status=status, eps=EPS)
    return out


def grid_map_fast(h, w, rows, cols):
    return ((np.arange(h)[:, None] * rows // h) * cols + np.arange(w)[None, :] * cols // w).astype(np.uint16)


def args(c, force=True, status=True):
    return (c["depth"], c["map"], c["T"], c["origin"], c["mpp"], c["eps"], c["force"] if force else None, c["status"] if status else None)
