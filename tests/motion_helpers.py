"""The contact motion read-out's definition (include/vistaf_motion.h) written out in NumPy, and hand-made scenes for tests/test_motion.py.

`numpy_motion` follows the header step by step in float64: the per-pixel expressions are the header's, operation for operation (NumPy does
not fuse), `_chol_solve` is csrc/chol.hpp line for line.  What is left between it and the device is the order of the sums over the template
pixels and the device's sin / cos.  `order` chooses how the restatement adds: "forward" (np.add.reduce in pixel order), "reversed" (the same
on the reversed pixels) or "fsum" (math.fsum, the correctly rounded sum); the distance between these on a case is what summation order alone
costs there, and the device is held to 16 times that (tests/test_motion.py).
"""
import math

import numpy as np

import shapes_helpers as SH

NCONTACT, NTRACK, NMOTION, NFRAME = 16, 16, 24, 8
FIELDS = ("parent_row", "template_pixels", "status", "iterations", "tx_px", "ty_px", "theta_rad", "beta_mm", "tx_mm", "ty_mm", "centre_x", "centre_y",
          "rms_before_mm", "rms_after_mm", "last_step_px", "se_tx_px", "se_ty_px", "se_theta_rad", "tx_minus_dx", "ty_minus_dy")
FRAME_FIELDS = ("registered", "max_slide_mm", "max_slide_row", "max_twist_rad", "max_twist_row", "mean_tx_mm", "mean_ty_mm", "mean_rms_after_mm")
M = {name: i for i, name in enumerate(FIELDS)}
MF = {name: i for i, name in enumerate(FRAME_FIELDS)}
EXACT = ("parent_row", "template_pixels", "status", "iterations", "centre_x", "centre_y")      # integers, and quotients of exact integers
FRAME_EXACT = ("registered", "max_slide_row", "max_twist_row")
OK, NOT_CONVERGED, NO_PARENT, TOO_FEW, SINGULAR = 0, 1, 2, 3, 4
T_PARENT, T_DX, T_DY = 2, 5, 6                                   # VISTAF_TRACK_* indices the read-out reads
FLOOR = 2.0 ** -32


def _chol_solve(A, rhs, N=4):
    """csrc/chol.hpp: returns the solution, or None if A is not positive definite"""
    L = [[0.0] * N for _ in range(N)]
    inv = [0.0] * N
    for i in range(N):
        for j in range(i + 1):
            s = A[i][j]
            for k in range(j):
                s -= L[i][k] * L[j][k]
            if i == j:
                if not s > 0.0:
                    return None
                L[i][i] = math.sqrt(s)
                inv[i] = 1.0 / L[i][i]
            else:
                L[i][j] = s * inv[j]
    x = [float(v) for v in rhs]
    for i in range(N):
        s = x[i]
        for k in range(i):
            s -= L[i][k] * x[k]
        x[i] = s * inv[i]
    for i in range(N - 1, -1, -1):
        s = x[i]
        for k in range(i + 1, N):
            s -= L[k][i] * x[k]
        x[i] = s * inv[i]
    return x


def _sum(v, order):
    v = np.asarray(v, dtype=np.float64)
    if order == "fsum":
        return math.fsum(v.tolist())
    return float(np.add.reduce(v[::-1] if order == "reversed" else v)) if v.size else 0.0


def _plane(d32):
    d = np.asarray(d32, dtype=np.float32)
    return np.where(np.isfinite(d), d, np.float32(0.0))


def _at(d, x, y):
    """float64 values of the cleaned float32 plane at coordinates clamped to the frame"""
    h, w = d.shape
    return d[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)].astype(np.float64)


def _sample(d, wx, wy):
    h, w = d.shape
    mx, my = float(w - 1), float(h - 1)
    with np.errstate(invalid="ignore"):
        qx = np.where(wx >= 0.0, np.where(wx <= mx, wx, mx), 0.0)
        qy = np.where(wy >= 0.0, np.where(wy <= my, wy, my), 0.0)
    x0, y0 = qx.astype(np.int64), qy.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    fx, fy = qx - x0.astype(np.float64), qy - y0.astype(np.float64)
    top = (1.0 - fx) * d[y0, x0].astype(np.float64) + fx * d[y0, x1].astype(np.float64)
    bot = (1.0 - fx) * d[y1, x0].astype(np.float64) + fx * d[y1, x1].astype(np.float64)
    return (1.0 - fy) * top + fy * bot


def register(T32, I32, mask, box_wh, s, start=(0.0, 0.0), dxy=(np.nan, np.nan), iterations=8, tol_px=1e-3, min_pixels=16, order="forward", parent=0):
    """one pair: the row [24] of steps 1..5.  T32 / I32 the float32 planes of frame t-1 / t, mask the template pixels, box_wh the clipped box's
    width and height, start the initial (tx, ty), dxy the tracker's (DX, DY)"""
    row = np.full(NMOTION, np.nan)
    T, I = _plane(T32), _plane(I32)
    ys, xs = np.nonzero(mask)
    n = int(xs.size)
    row[M["parent_row"]], row[M["template_pixels"]], row[M["iterations"]] = parent, n, 0
    if n:
        cx, cy = float(int(xs.sum())) / float(n), float(int(ys.sum())) / float(n)
        row[M["centre_x"]], row[M["centre_y"]] = cx, cy
    if n < min_pixels:
        row[M["status"]] = TOO_FEW
        return row
    bw, bh = float(box_wh[0]), float(box_wh[1])
    R = 0.5 * math.sqrt(bw * bw + bh * bh)
    Tv = T[ys, xs].astype(np.float64)
    Tx = (_at(T, xs + 1, ys) - _at(T, xs - 1, ys)) / 2.0
    Ty = (_at(T, xs, ys + 1) - _at(T, xs, ys - 1)) / 2.0
    ux, uy = xs.astype(np.float64) - cx, ys.astype(np.float64) - cy
    g2 = ux * Ty - uy * Tx
    S = lambda v: _sum(v, order)
    h00, h01, h02, h03, h11, h12, h13, h22, h23 = (S(Tx * Tx), S(Tx * Ty), S(Tx * g2), S(Tx), S(Ty * Ty), S(Ty * g2), S(Ty), S(g2 * g2), S(g2))
    H = [[h00, h01, h02, h03], [h01, h11, h12, h13], [h02, h12, h22, h23], [h03, h13, h23, float(n)]]
    H2 = [[H[i][j] - FLOOR * H[i][j] if i == j else H[i][j] for j in range(4)] for i in range(4)]
    if _chol_solve(H2, [0.0] * 4) is None or _chol_solve(H, [0.0] * 4) is None:
        row[M["status"]] = SINGULAR
        return row
    tx, ty, theta, beta = float(start[0]), float(start[1]), 0.0, 0.0
    c, sn = math.cos(theta), math.sin(theta)
    last = 0.0

    def sweep():
        wx, wy = ((cx + c * ux) - sn * uy) + tx, ((cy + sn * ux) + c * uy) + ty
        r = (_sample(I, wx, wy) - beta) - Tv
        return [S(Tx * r), S(Ty * r), S(g2 * r), S(r)], S(r * r)
    for it in range(iterations):
        b, rss = sweep()
        if it == 0:
            rss_before = rss
        d = _chol_solve(H, b)
        theta = theta - d[2]
        c, sn = math.cos(theta), math.sin(theta)
        tx = tx - (c * d[0] - sn * d[1])
        ty = ty - (sn * d[0] + c * d[1])
        beta = beta + d[3]
        last = max(abs(d[0]), abs(d[1]), abs(d[2]) * R) if not any(math.isnan(v) for v in d[:3]) else math.nan
    _, rss_after = sweep()
    row[M["status"]] = OK if last <= tol_px else NOT_CONVERGED
    row[M["iterations"]] = iterations
    row[M["tx_px"]], row[M["ty_px"]], row[M["theta_rad"]], row[M["beta_mm"]] = tx, ty, theta, beta
    row[M["tx_mm"]], row[M["ty_mm"]] = tx * s, ty * s
    with np.errstate(invalid="ignore"):
        row[M["rms_before_mm"]], row[M["rms_after_mm"]] = np.sqrt(rss_before / float(n)), np.sqrt(rss_after / float(n))
        row[M["last_step_px"]] = last
        var = rss_after / (float(n - 4) if n > 5 else 1.0)
        for i, name in enumerate(("se_tx_px", "se_ty_px", "se_theta_rad")):
            e = [0.0] * 4
            e[i] = 1.0
            row[M[name]] = np.sqrt(_chol_solve(H, e)[i] * var)
    row[M["tx_minus_dx"]], row[M["ty_minus_dy"]] = tx - dxy[0], ty - dxy[1]
    return row


def numpy_motion(depth_mm, contact_index, contacts, count, tracks, mm_per_px, eps, iterations=8, tol_px=1e-3, min_pixels=16,
                 init_from_centroid=True, carry=None, order="forward"):
    """depth_mm [B,h,w] float32, contact_index [B,h,w] int8, contacts [B,K,16], count [B], tracks [B,K,16], mm_per_px [B].  Returns
    (motion [B,K,24], frame [B,8], carry); pass the carry of one call to the next to continue the sequence."""
    depth_mm, contact_index = np.asarray(depth_mm, dtype=np.float32), np.asarray(contact_index)
    contacts, tracks = np.asarray(contacts, dtype=np.float64), np.asarray(tracks, dtype=np.float64)
    B, h, w = contact_index.shape
    K = contacts.shape[1]
    motion, frame = np.full((B, K, NMOTION), np.nan), np.full((B, NFRAME), np.nan)
    prev = carry
    for t in range(B):
        kk = min(max(int(count[t]), 0), K)
        m = 0 if prev is None else min(max(int(prev["count"]), 0), K)
        for k in range(kk):
            pr, DX, DY = tracks[t, k, T_PARENT], tracks[t, k, T_DX], tracks[t, k, T_DY]
            if not np.isfinite(pr) or pr < 0 or pr >= m:
                motion[t, k, :4] = [pr if np.isfinite(pr) else -1.0, 0, NO_PARENT, 0]
                continue
            p = int(pr)
            clipped = SH.table_box(prev["table"][p], h, w)[1]
            bw, bh = (clipped[2] - clipped[0] + 1, clipped[3] - clipped[1] + 1) if clipped else (0, 0)
            mask = SH.box_mask(clipped, h, w) & (prev["index"] == p) & (_plane(prev["depth"]) > np.float32(eps))
            start = (DX, DY) if init_from_centroid and np.isfinite(DX) and np.isfinite(DY) else (0.0, 0.0)
            motion[t, k] = register(prev["depth"], depth_mm[t], mask, (bw, bh), float(mm_per_px[t]), start, (DX, DY), iterations, tol_px, min_pixels,
                                    order, p)
        if kk:
            ok = [k for k in range(kk) if motion[t, k, M["status"]] == OK]
            frame[t, MF["registered"]] = len(ok)
            if ok:
                r = motion[t]
                slide = [math.sqrt(r[k, M["tx_mm"]] * r[k, M["tx_mm"]] + r[k, M["ty_mm"]] * r[k, M["ty_mm"]]) for k in ok]
                twist = [abs(r[k, M["theta_rad"]]) for k in ok]
                js, jt = int(np.argmax(slide)), int(np.argmax(twist))                      # argmax: the first maximum
                wn = wx = wy = wr = 0.0
                for k in ok:
                    nk = r[k, M["template_pixels"]]
                    wn, wx, wy, wr = wn + nk, wx + nk * r[k, M["tx_mm"]], wy + nk * r[k, M["ty_mm"]], wr + nk * r[k, M["rms_after_mm"]]
                frame[t, 1:] = [slide[js], ok[js], twist[jt], ok[jt], wx / wn, wy / wn, wr / wn]
        prev = {"depth": depth_mm[t].copy(), "index": contact_index[t].copy(), "table": contacts[t].copy(), "count": int(count[t])}
    return motion, frame, prev


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return bool(a.shape == b.shape and a.dtype == b.dtype == np.float64 and np.array_equal(a.view(np.int64), b.view(np.int64)))


def exact_equal(a, b, fields=EXACT, names=M):
    """the exact fields equal and NaN in the same places of the whole table"""
    a, b = np.asarray(a), np.asarray(b)
    cols = [names[f] for f in fields]
    na, nb = np.isnan(a[..., cols]), np.isnan(b[..., cols])
    return bool(a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(na, nb) and
                np.array_equal(a[..., cols][~na], b[..., cols][~nb]))


def field_distances(a, b):
    """{field: largest |a - b|} over the float fields of two motion tables (NaN in both does not count) -- absolute: pixels, radians, mm"""
    a, b = np.asarray(a), np.asarray(b)
    out = {}
    for name in FIELDS:
        if name in EXACT:
            continue
        d = np.abs(a[..., M[name]] - b[..., M[name]])
        out[name] = float(np.nanmax(d)) if np.isfinite(d).any() else 0.0
    return out


def frame_distances(a, b):
    a, b = np.asarray(a), np.asarray(b)
    out = {}
    for name in FRAME_FIELDS:
        if name in FRAME_EXACT:
            continue
        d = np.abs(a[..., MF[name]] - b[..., MF[name]])
        out[name] = float(np.nanmax(d)) if np.isfinite(d).any() else 0.0
    return out


# ---------------------------------------------------------------------------------------------------------------- surfaces and scenes
def two_bump(xm, ym):
    """an anisotropic ellipsoidal cap (a paraboloid cut at 0, radii 3.3 and 1.25 mm along axes turned by 0.45 rad, 1.1 mm deep) plus a second,
    off-centre Gaussian bump; xm, ym in mm about the contact's own origin"""
    a = 0.45
    up, vp = np.cos(a) * xm + np.sin(a) * ym, -np.sin(a) * xm + np.cos(a) * ym
    cap = np.maximum(1.1 - (up * up / (2.0 * 3.3) + vp * vp / (2.0 * 1.25)), 0.0)
    return cap + 0.35 * np.exp(-((xm - 0.9) ** 2 + (ym + 0.5) ** 2) / (2.0 * 0.45 * 0.45))


def ball(radius_mm, depth_mm):
    """the cap a ball of that radius leaves when pressed `depth_mm` deep: rotationally symmetric, not a paraboloid"""
    def f(xm, ym):
        return np.maximum(np.sqrt(np.maximum(radius_mm * radius_mm - (xm * xm + ym * ym), 0.0)) - (radius_mm - depth_mm), 0.0)
    return f


def rigid(x, y, centre, motion):
    """W^-1 of the header's warp: the coordinates in frame t-1 of the points (x, y) of frame t, for motion = (tx, ty, theta)"""
    tx, ty, th = motion
    qx, qy = x - centre[0] - tx, y - centre[1] - ty
    return centre[0] + np.cos(th) * qx + np.sin(th) * qy, centre[1] - np.sin(th) * qx + np.cos(th) * qy


def footprint_centre(mask):
    ys, xs = np.nonzero(mask)
    return float(int(xs.sum())) / xs.size, float(int(ys.sum())) / xs.size


class Contact:
    """a surface function f(xm, ym) in mm placed at `origin` (pixels) in a frame of s mm per pixel; `moved` composes a rigid motion about
    a centre and a depth change on top of it, as the object it stands for would move"""

    def __init__(self, f, origin, s, level=0.05, floor=0.02):
        self.f, self.origin, self.s, self.level, self.floor, self.chain, self.beta = f, origin, s, level, floor, [], 0.0

    def depth(self, h, w):
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        for centre, motion in reversed(self.chain):
            xx, yy = rigid(xx, yy, centre, motion)
        d = self.f((xx - self.origin[0]) * self.s, (yy - self.origin[1]) * self.s)
        return np.where(d > self.floor, d + self.beta, 0.0)

    def moved(self, centre, motion, beta):
        c = Contact(self.f, self.origin, self.s, self.level, self.floor)
        c.chain, c.beta = self.chain + [(centre, motion)], self.beta + beta
        return c


def paint(scene, k, contact):
    """paint the contact into a shapes_helpers.Scene as row k: its pixels deeper than `level` are labelled, the depth is written wherever
    the surface is above its floor (so the plane continues under the label's edge); returns the labelled mask"""
    h, w = scene.depth.shape
    d = contact.depth(h, w)
    lab = d > contact.level
    scene.depth[d > 0.0] = d[d > 0.0].astype(np.float32)
    scene.index[lab] = k
    return lab


def tracks_rows(B, K):
    return np.full((B, K, NTRACK), np.nan)


def link(tracks, t, k, parent, masks=None):
    """hand-made tracker row: PARENT_ROW, and DX / DY from the footprint centres of masks = (parent's, own) when given"""
    tracks[t, k, :5] = [10 * t + k, 1 if parent >= 0 else 0, parent, 0 if parent >= 0 else 1, 0]
    if parent >= 0 and masks is not None:
        (px, py), (qx, qy) = footprint_centre(masks[0]), footprint_centre(masks[1])
        tracks[t, k, T_DX], tracks[t, k, T_DY] = qx - px, qy - py


EPS, K, S_MM = 0.01, 4, 0.3
MOVE_A = (1.3, -0.7, 0.05, 0.02)


def pack(scenes, tracks, count, params=None, s=S_MM):
    depth, index = np.stack([sc.depth for sc in scenes]), np.stack([sc.index for sc in scenes])
    tab, cnt = SH.table_from_planes(depth, index, K, EPS, count)
    return {"depth": depth, "index": index, "tab": tab, "count": cnt, "tracks": tracks, "mpp": np.full(len(scenes), s), "eps": EPS,
            "params": dict(params or {})}


def main_batch(h, w, background=0.0):
    """three frames, four rows: frame 1 holds (row 0) the two-bump contact moved by MOVE_A, (1) a contact cut by the right border and moved
    further into it, (2) a ball's round cap, (3) a ridge across the whole frame whose parent is a 15-pixel contact (TOO_FEW); frame 2 holds
    (0) the two-bump contact moved again, with NaNs in both depth planes, (1) a born row, (2) a row whose parent row is beyond the table,
    (3) the ridge again (SINGULAR: its depth does not change along x)"""
    s = S_MM
    sc = [SH.Scene(h, w, background) for _ in range(3)]
    tr = tracks_rows(3, K)
    a0 = Contact(two_bump, (14.3, 12.6), s)
    b0 = Contact(ball(2.5, 0.9), (w - 4.4, 24.3), s)
    c0 = Contact(ball(2.0, 0.8), (33.7, 9.8), s)
    m0 = [paint(sc[0], 0, a0), paint(sc[0], 1, b0), paint(sc[0], 2, c0)]
    small = SH.rect(h, w, 3, 27, 7, 29)
    sc[0].paint(3, small, 0.4 + 0.02 * np.arange(w)[None, :])
    for k in range(4):
        link(tr, 0, k, -1)
    a1 = a0.moved(footprint_centre(m0[0]), MOVE_A[:3], MOVE_A[3])
    b1 = b0.moved(footprint_centre(m0[1]), (0.8, 0.6, -0.03), -0.01)
    c1 = c0.moved(footprint_centre(m0[2]), (0.5, -0.4, 0.0), 0.01)
    m1 = [paint(sc[1], 0, a1), paint(sc[1], 1, b1), paint(sc[1], 2, c1)]
    ridge = SH.rect(h, w, 0, h - 4, w - 1, h - 2)
    prof = np.zeros((h, 1))
    prof[h - 4:h - 1, 0] = [0.3, 0.55, 0.35]
    sc[1].paint(3, ridge, np.broadcast_to(prof, (h, w)))
    for k in range(3):
        link(tr, 1, k, k, (m0[k], m1[k]))
    link(tr, 1, 3, 3, (small, ridge))
    a2 = a1.moved(footprint_centre(m1[0]), (-0.9, 1.1, -0.04), -0.015)
    m2 = paint(sc[2], 0, a2)
    paint(sc[2], 1, b1)
    paint(sc[2], 2, c1)
    sc[2].paint(3, ridge, np.broadcast_to(prof + 0.01, (h, w)))
    ys, xs = np.nonzero(m1[0])
    if np.isnan(background):                                         # frame 1 is sampled by pair 0 -> 1 and is the template of pair 1 -> 2
        sc[1].depth[ys[5], xs[5]] = np.nan                           # a template pixel lost, and neighbours of template pixels
        sc[1].depth[ys[len(ys) // 2], xs[len(ys) // 2]] = np.nan
    sc[2].depth[ys[len(ys) // 3], xs[len(ys) // 3] + 1] = np.nan    # taps of the sample
    sc[2].depth[ys[-4], xs[-4]] = np.inf
    link(tr, 2, 0, 0, (m1[0], m2))
    link(tr, 2, 1, -1)
    link(tr, 2, 2, 7)
    link(tr, 2, 3, 3, (ridge, ridge))
    return pack(sc, tr, [4, 4, 4])


def empty_frame_batch(h, w):
    """count = [1, 0, 1]: the frame without contacts has NaN rows and a NaN frame row, and what follows it has no parent"""
    sc = [SH.Scene(h, w, 0.0) for _ in range(3)]
    tr = tracks_rows(3, K)
    a0 = Contact(two_bump, (20.2, 15.4), S_MM)
    m0 = paint(sc[0], 0, a0)
    paint(sc[1], 0, a0)                                              # the plane is there, the count says 0
    a2 = a0.moved(footprint_centre(m0), (0.4, 0.3, 0.01), 0.0)
    m2 = paint(sc[2], 0, a2)
    link(tr, 0, 0, -1)
    link(tr, 2, 0, 0, (m0, m2))                                      # the tracker would not say so; the read-out must not follow it
    return pack(sc, tr, [1, 0, 1])


def jump_batch(h, w):
    """a 12 px jump with init_from_centroid off: eight steps from 0 do not get there"""
    sc = [SH.Scene(h, w, 0.0) for _ in range(3)]
    tr = tracks_rows(3, K)
    a0 = Contact(two_bump, (16.0, 14.0), S_MM)
    m0 = paint(sc[0], 0, a0)
    a1 = a0.moved(footprint_centre(m0), (12.0, 0.0, 0.0), 0.0)
    m1 = paint(sc[1], 0, a1)
    a2 = a1.moved(footprint_centre(m1), (0.0, 12.0, 0.0), 0.0)
    m2 = paint(sc[2], 0, a2)
    link(tr, 0, 0, -1)
    link(tr, 1, 0, 0, (m0, m1))
    link(tr, 2, 0, 0, (m1, m2))
    return pack(sc, tr, [1, 1, 1], {"init_from_centroid": False})


SIZES = ((40, 52), (37, 53))


def cases():
    c = {}
    for h, w in SIZES:
        c["main_%dx%d" % (h, w)] = main_batch(h, w)
        c["empty_frame_%dx%d" % (h, w)] = empty_frame_batch(h, w)
        c["jump_%dx%d" % (h, w)] = jump_batch(h, w)
    c["main_nan_background_37x53"] = main_batch(37, 53, np.nan)
    return c


def run(case, order="forward", carry=None, frames=slice(None)):
    f = frames
    return numpy_motion(case["depth"][f], case["index"][f], case["tab"][f], case["count"][f], case["tracks"][f], case["mpp"][f], case["eps"],
                        carry=carry, order=order, **case["params"])
