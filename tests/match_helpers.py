"""Plain NumPy / Python restatement of the indenter match read-out (include_ext/vistaf_match.h) and the analytic inputs of tests/test_matches.py.

`ref_bank` restates the host bank builder with plain Python floats, one IEEE operation at a time in the header's order, so the library's bank
must equal it bit for bit.  `numpy_matches` restates the measure: the patch with NumPy's element-wise float64 operations (each a single IEEE
operation, so the float32 patch must equal the device's bit for bit), the sums and dot products in np.longdouble, whose own rounding (2^-64
per operation) is negligible beside the float64 bounds below.

THE BOUNDS, none of them measured off the device; u = 2^-53, D the disc's size, first order in u (the second order is (D u)^2, below 1e-26):
  g       a length-D dot product accumulated in any order, fused or not: |g - g*| <= (D+3) u sum|bank||w|                        (e_g)
  S1      |S1 - S1*| <= (D-1) u sum|w|;  S2 (every product of two widened float32 exact): (D+1) u S2
  var     = S2 - (S1*S1)/D: e_var = u ((D+1) S2 + (2 (D-1) |S1| sum|w| + 2 S1^2)/D + |var|) -- the cancellation bound of var
  score   = g / sqrt(var): e = e_g / sd + |g| e_var / (2 var sd) -- (D+3) 2^-53 sum|bank||w| / sqrt(var) plus var's cancellation term; the
          +3 of e_g covers the device's square root and division -- plus one u |score| for the cast of the longdouble reference to float64
and each later field pushes these through its own expression, first order, with one u |field| per operation of the field's own expression
on the device and one for the reference's (`_match_row`, `tol`).  Integer fields are exact on the device whenever the
winner's score exceeds every other (t, r, s) by more than twice the largest score bound: `gap` is returned for the tests to assert."""
import math

import numpy as np

NMATCH = 24
FIELDS = ["status", "flags", "label", "template", "class", "rotation", "shift_x", "shift_y", "score", "angle_rad", "x_px", "y_px", "offset_x_mm",
          "offset_y_mm", "second_class", "second_score", "margin", "rot_contrast", "scale", "base_mm", "resid_rms_mm", "support_pixels", "valid_shifts"]
F = {n: i for i, n in enumerate(FIELDS)}
INT_FIELDS = ("status", "flags", "label", "template", "class", "rotation", "shift_x", "shift_y", "second_class", "support_pixels", "valid_shifts")
OK, NO_PIXELS, NO_SCALE, NO_SUPPORT = 0, 1, 2, 3
CLIPPED, BORDER_SHIFT, WEAK, AMBIGUOUS = 1, 2, 4, 8
U = 2.0 ** -53
NCONTACT = 16
C_CX, C_CY = 6, 7

# ------------------------------------------------------------------------------------------------ the analytic indenters and their frames
H, W = 40, 48
CENTRE = (22.3, 17.6)
ANGLES = (60.0, 70.0)
AMP = 0.6
EPS = 0.01


def ball(u, v):
    return np.maximum(0.0, 0.5 - (u * u + v * v) / 0.5)


def ridge(u, v):
    return np.where(np.abs(v) <= 0.38, np.maximum(0.0, 0.5 - u * u / 0.12), 0.0)


def tee(u, v):
    stem = (np.abs(u) <= 0.12) & (np.abs(v) <= 0.36)
    bar = (np.abs(v - 0.28) <= 0.1) & (np.abs(u) <= 0.36)
    return np.where(stem | bar, 0.4, 0.0)


SHAPES = (("ball", ball, 0), ("ridge", ridge, 2), ("tee", tee, 1))          # name, height(u, v) in mm, symmetry order
SMALL = dict(P=9, pitch=0.1, R=12, m=2, mpp=(0.1, 0.08))                     # rho = pitch / mpp = 1, 1.25;   M = 1 + 6 + 12 = 19, D = 49
LARGE = dict(P=17, pitch=0.05, R=24, m=3, mpp=(0.1, 0.08))                   # rho = 0.5, 0.625;               M = 1 + 12 + 24 = 37, D = 197


def template_of(fn, P, pitch):
    c = (P - 1) // 2
    x = (np.arange(P) - c) * pitch
    u, v = np.meshgrid(x, x)
    return fn(u, v).astype(np.float32)


def templates(P, pitch, shapes=SHAPES):
    return np.stack([template_of(fn, P, pitch) for _, fn, _ in shapes])


def contact_depth(fn, angle_deg, mpp, h=H, w=W, centre=CENTRE, amp=AMP):
    """the indenter turned by +angle (from x towards y) about `centre`, evaluated analytically at every pixel: float32 [h,w]"""
    a = math.radians(angle_deg)
    x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    du, dv = (x - centre[0]) * mpp, (y - centre[1]) * mpp
    u = math.cos(a) * du + math.sin(a) * dv
    v = -math.sin(a) * du + math.cos(a) * dv
    return (amp * fn(u, v)).astype(np.float32)


def table_of(depth, index, K, eps=EPS):
    """a contacts table [K,16] as far as the read-out reads it: the depth-weighted centroid of the contact pixels of every index, and the box"""
    tab = np.full((K, NCONTACT), np.nan)
    n = 0
    for k in range(K):
        sel = (index == k) & np.isfinite(depth) & (np.nan_to_num(depth, nan=0.0, posinf=0.0, neginf=0.0) > eps)
        if not (index == k).any():
            break
        n = k + 1
        ys, xs = np.nonzero(index == k)
        tab[k] = 0.0
        tab[k, 0] = len(ys)
        tab[k, 9:13] = [xs.min(), ys.min(), xs.max(), ys.max()]
        if sel.any():
            d = depth[sel].astype(np.float64)
            yy, xx = np.nonzero(sel)
            tab[k, 1] = len(yy)
            tab[k, C_CX], tab[k, C_CY] = float((d * xx).sum() / d.sum()), float((d * yy).sum() / d.sum())
        else:
            tab[k, C_CX] = tab[k, C_CY] = np.nan
    return tab, n


def frames24(cfg, K=2):
    """the 12 frames of one bank's half of the 24 cases: dict of depth [12,H,W] f32, index int8, contacts [12,K,16], count, mm_per_px and `truth`,
    per frame (template index, angle in rad, centre)"""
    depth, index, tabs, cnt, mpp, truth = [], [], [], [], [], []
    for s in cfg["mpp"]:
        for t, (_, fn, _) in enumerate(SHAPES):
            for ang in ANGLES:
                d = contact_depth(fn, ang, s)
                ix = np.where(d > 0, 0, -1).astype(np.int8)
                tab, n = table_of(d, ix, K)
                depth.append(d); index.append(ix); tabs.append(tab); cnt.append(n); mpp.append(s)
                truth.append((t, math.radians(ang), CENTRE))
    return dict(depth=np.stack(depth), index=np.stack(index), contacts=np.stack(tabs), count=np.array(cnt, np.int32), mm_per_px=np.array(mpp),
                truth=truth)


# ------------------------------------------------------------------------------------------------ the bank, plain loops
def disc_offsets(P):
    c = (P - 1) // 2
    return [(dx, dy) for dy in range(-c, c + 1) for dx in range(-c, c + 1) if dx * dx + dy * dy <= c * c]


def _bilinear(tp, P, x, y):
    xf, yf = math.floor(x), math.floor(y)
    fx, fy = x - xf, y - yf
    x0, y0 = int(xf), int(yf)

    def at(xx, yy):
        return float(tp[yy][xx]) if 0 <= xx < P and 0 <= yy < P else 0.0
    v00, v10, v01, v11 = at(x0, y0), at(x0 + 1, y0), at(x0, y0 + 1), at(x0 + 1, y0 + 1)
    return (v00 * (1.0 - fx) + v10 * fx) * (1.0 - fy) + (v01 * (1.0 - fx) + v11 * fx) * fy


def ref_bank(tps, symmetry, R, cossin=None):
    """header, step 1: cossin [R,2] (math.cos / math.sin unless handed in), rowtab, disc, mu, norm, rows [M,Dp]"""
    T, P = len(tps), len(tps[0])
    c = (P - 1) // 2
    if cossin is None:
        cossin = [(math.cos((2.0 * math.pi * r) / R), math.sin((2.0 * math.pi * r) / R)) for r in range(R)]
    disc = disc_offsets(P)
    D = len(disc)
    Dp = (D + 3) // 4 * 4
    rowtab, mu, norm, rows = [], [], [], []
    for t in range(T):
        rt = R // symmetry[t] if symmetry[t] else 1
        for r in range(rt):
            co, si = float(cossin[r][0]), float(cossin[r][1])
            v = [_bilinear(tps[t], P, (c + co * dx) + si * dy, (c - si * dx) + co * dy) for dx, dy in disc]
            s = 0.0
            for e in v:
                s += e
            mean = s / D
            ss = 0.0
            for e in v:
                ss += (e - mean) * (e - mean)
            nr = math.sqrt(ss)
            rowtab.append((t, r)); mu.append(mean); norm.append(nr)
            rows.append([(e - mean) / nr for e in v] + [0.0] * (Dp - D))
    return dict(cossin=np.array(cossin), rowtab=np.array(rowtab, np.int32), disc=np.array(disc, np.int32), mu=np.array(mu), norm=np.array(norm),
                rows=np.array(rows), D=D, Dp=Dp, M=len(rows))


def layout_bytes(T, P, R, M, D):
    """THE BANK of the header: its size in bytes"""
    up = lambda v, a: (v + a - 1) // a * a
    rows = up(up(64 + 16 * R + 8 * M + 8 * T, 8) + 8 * D + 16 * M, 256)
    return rows + 8 * M * ((D + 3) // 4 * 4)


# ------------------------------------------------------------------------------------------------ the measure
class _Row:
    """one row's reference: `rec` the 24 doubles, `scores` [T], `patch` [S,S] f32, `bound` the largest score bound of the row, `gap` the
    winner's lead over every other (t, r, s), `tol` the tolerance of every float field"""


def _patch(depth, index, k, cx, cy, rho, P, m):
    h, w = depth.shape
    c = (P - 1) // 2
    q, S = c + m, P + 2 * m
    t = (np.arange(S) - q).astype(np.float64) * rho
    X, Y = np.meshgrid(cx + t, cy + t)
    xf, yf = np.floor(X), np.floor(Y)
    fx, fy = X - xf, Y - yf

    def iso(xx, yy):
        inside = (xx >= 0) & (xx <= w - 1) & (yy >= 0) & (yy <= h - 1)
        xi, yi = np.where(inside, xx, 0).astype(np.int64), np.where(inside, yy, 0).astype(np.int64)
        d = depth[yi, xi]
        ok = inside & (index[yi, xi] == k) & np.isfinite(d)
        return np.where(ok, d, np.float32(0)).astype(np.float64)
    v00, v10, v01, v11 = iso(xf, yf), iso(xf + 1.0, yf), iso(xf, yf + 1.0), iso(xf + 1.0, yf + 1.0)
    v = (v00 * (1.0 - fx) + v10 * fx) * (1.0 - fy) + (v01 * (1.0 - fx) + v11 * fx) * fy
    clipped = bool(np.any(~((xf >= 0) & (xf + 1.0 <= w - 1) & (yf >= 0) & (yf + 1.0 <= h - 1))))
    return v.astype(np.float32), clipped


def _parabola(am, a0, ap, em, e0, ep):
    """(delta, its bound) of header step 6"""
    if not (math.isfinite(am) and math.isfinite(ap)):
        return 0.0, 0.0
    den = (am - 2.0 * a0) + ap
    if not den < 0.0:
        return 0.0, 0.0
    num = 0.5 * (am - ap)
    d = num / den
    return d, (0.5 * (em + ep)) / abs(den) + abs(num) * (em + 2.0 * e0 + ep) / (den * den) + 6.0 * U * abs(d)      # 5 operations + the reference


def _match_row(depth, index, k, cx, cy, rho, bank, eps, m, min_pixels, accept_score, accept_margin):
    P, R, T, M, D = bank.P, bank.R, bank.T, bank.M, bank.D
    c = (P - 1) // 2
    q, Wn = c + m, 2 * m + 1
    NS = Wn * Wn
    out = _Row()
    out.rec = np.full(NMATCH, np.nan)
    out.scores = np.full(T, np.nan)
    out.bound, out.gap, out.tol = 0.0, math.inf, {}
    out.patch, clipped = _patch(depth, index, k, cx, cy, rho, P, m)
    disc, tmpp = np.asarray(bank.disc), bank.template_mm_per_px
    s_idx = np.arange(NS)
    sy, sx = s_idx // Wn - m, s_idx % Wn - m
    wf = out.patch[q + sy[:, None] + disc[None, :, 1], q + sx[:, None] + disc[None, :, 0]]           # [NS, D] float32
    wl = wf.astype(np.longdouble)
    absw = np.abs(wf.astype(np.float64)).sum(axis=1)
    S1, S2 = wl.sum(axis=1), (wl * wl).sum(axis=1)
    var = S2 - S1 * S1 / D
    nz = (wf > np.float32(eps)).sum(axis=1)
    valid = (nz >= min_pixels) & (var > 0)
    rows = np.asarray(bank.rows)[:, :D]
    with np.errstate(all="ignore"):
        G = rows.astype(np.longdouble) @ wl.T                                                       # [M, NS]
        sd = np.sqrt(var)
        score = (G / sd[None, :]).astype(np.float64)
        S1d, S2d, vard, Gd, sdd = S1.astype(np.float64), S2.astype(np.float64), var.astype(np.float64), G.astype(np.float64), sd.astype(np.float64)
        e_g = (D + 3) * U * (np.abs(rows) @ np.abs(wf.astype(np.float64)).T)
        e_var = U * ((D + 1) * S2d + (2.0 * (D - 1) * np.abs(S1d) * absw + 2.0 * S1d * S1d) / D + np.abs(vard))
        e_score = e_g / sdd[None, :] + np.abs(Gd) * (e_var / (2.0 * vard * sdd))[None, :] + U * np.abs(score)
    out.rec[F["valid_shifts"]] = float(valid.sum())
    if not valid.any():
        out.rec[F["status"]] = NO_SUPPORT
        return out
    masked = np.where(valid[None, :], score, -np.inf)
    flat = int(np.argmax(masked))                                  # the first maximum in (row, shift) order: t, r, sy, sx
    wrow, s = divmod(flat, NS)
    others = np.delete(masked.reshape(-1), flat)
    a0 = float(masked[wrow, s])
    out.gap = a0 - float(others.max()) if others.size and np.isfinite(others.max()) else math.inf
    out.bound = float(e_score[:, valid].max())
    rowtab, klass, symmetry = np.asarray(bank.rowtab), np.asarray(bank.klass), np.asarray(bank.symmetry)
    wt, r = int(rowtab[wrow, 0]), int(rowtab[wrow, 1])
    start = wrow - r
    sym = int(symmetry[wt])
    rt = R // sym if sym else 1
    per_row = masked.max(axis=1)
    for t in range(T):
        out.scores[t] = per_row[rowtab[:, 0] == t].max()
    bsx, bsy = int(sx[s]), int(sy[s])
    e0 = float(e_score[wrow, s])

    def at(row, tx, ty):
        if not (-m <= tx <= m and -m <= ty <= m):
            return math.nan, 0.0
        ts = (ty + m) * Wn + (tx + m)
        return (float(score[row, ts]), float(e_score[row, ts])) if valid[ts] else (math.nan, 0.0)
    dr = e_dr = 0.0
    if rt >= 3:
        (am, em), (ap, ep) = at(start + (r - 1) % rt, bsx, bsy), at(start + (r + 1) % rt, bsx, bsy)
        dr, e_dr = _parabola(am, a0, ap, em, e0, ep)
    (am, em), (ap, ep) = at(wrow, bsx - 1, bsy), at(wrow, bsx + 1, bsy)
    dx, e_dx = _parabola(am, a0, ap, em, e0, ep)
    (am, em), (ap, ep) = at(wrow, bsx, bsy - 1), at(wrow, bsx, bsy + 1)
    dy, e_dy = _parabola(am, a0, ap, em, e0, ep)
    ang, per = 0.0, 0.0
    if sym:
        per = 2.0 * math.pi / sym
        ang = ((r + dr) * (2.0 * math.pi)) / R
        if ang < 0.0:
            ang += per
        if ang >= per:
            ang -= per
    other = [t for t in range(T) if klass[t] != klass[wt]]
    st = max(other, key=lambda t: (out.scores[t], -t)) if other else -1
    second = float(out.scores[st]) if st >= 0 else math.nan
    margin = a0 - second
    flags = (CLIPPED if clipped else 0) | (BORDER_SHIFT if m > 0 and (abs(bsx) == m or abs(bsy) == m) else 0)
    flags |= (WEAK if a0 < accept_score else 0) | (AMBIGUOUS if margin < accept_margin else 0)
    g, e_gw = float(Gd[wrow, s]), float(e_g[wrow, s])
    norm, mu = float(bank.norm[wrow]), float(bank.mu[wrow])
    scale = g / norm
    s1, vr, e_vr = float(S1d[s]), float(vard[s]), float(e_var[s])
    rest = vr - g * g
    resid = math.sqrt(max(rest, 0.0) / D)
    rc = out.rec
    rc[F["status"]], rc[F["flags"]] = OK, flags
    rc[F["label"]] = -1 if flags & (WEAK | AMBIGUOUS) else klass[wt]
    rc[F["template"]], rc[F["class"]], rc[F["rotation"]], rc[F["shift_x"]], rc[F["shift_y"]] = wt, klass[wt], r, bsx, bsy
    rc[F["score"]], rc[F["angle_rad"]] = a0, ang
    rc[F["x_px"]], rc[F["y_px"]] = cx + (bsx + dx) * rho, cy + (bsy + dy) * rho
    rc[F["offset_x_mm"]], rc[F["offset_y_mm"]] = (bsx + dx) * tmpp, (bsy + dy) * tmpp
    rc[F["second_class"]], rc[F["second_score"]], rc[F["margin"]] = (klass[st] if st >= 0 else -1), second, margin
    rc[F["rot_contrast"]] = a0 - float(per_row[start:start + rt].min())
    rc[F["scale"]], rc[F["base_mm"]], rc[F["resid_rms_mm"]] = scale, s1 / D - scale * mu, resid
    rc[F["support_pixels"]] = nz[s]
    e_scale = e_gw / norm + 2.0 * U * abs(scale)                      # the division, the reference's own
    e_rest = e_vr + 2.0 * abs(g) * e_gw + 2.0 * U * (abs(vr) + g * g)   # var, g*g to first order, the product and the difference, twice
    out.per = per
    out.tol = {"score": e0, "second_score": out.bound, "margin": e0 + out.bound, "rot_contrast": e0 + out.bound, "scale": e_scale,
               "base_mm": (D - 1) * U * float(absw[s]) / D + e_scale * abs(mu) + 4.0 * U * (abs(s1 / D) + abs(scale * mu)),
               "resid_rms_mm": (e_rest / D / resid if resid * resid > 4.0 * e_rest / D else math.sqrt(e_rest / D)) + 4.0 * U * resid,
               "angle_rad": e_dr * 2.0 * math.pi / R + 8.0 * U * max(per, 1.0),
               "x_px": e_dx * rho + 8.0 * U * (abs(cx) + (m + 1) * rho), "y_px": e_dy * rho + 8.0 * U * (abs(cy) + (m + 1) * rho),
               "offset_x_mm": e_dx * tmpp + 8.0 * U * (m + 1) * tmpp, "offset_y_mm": e_dy * tmpp + 8.0 * U * (m + 1) * tmpp}
    return out


def numpy_matches(depth, index, contacts, count, mm_per_px, bank, eps=EPS, max_shift=3, min_pixels=6, accept_score=0.7, accept_margin=0.05):
    """the read-out of [B,h,w] planes and a [B,K,16] table: dict of matches [B,K,24], scores [B,K,T], patches [B,K,S,S] f32 and `rows`, the
    _Row of every (b, k) (None for a row that is not in use or has no scale or pixels)"""
    B, K = contacts.shape[:2]
    S = bank.P + 2 * max_shift
    res = dict(matches=np.full((B, K, NMATCH), np.nan), scores=np.full((B, K, bank.T), np.nan), patches=np.full((B, K, S, S), np.nan, np.float32),
               rows=[[None] * K for _ in range(B)])
    for b in range(B):
        kk = min(max(int(count[b]), 0), K)
        s = float(mm_per_px[b])
        with np.errstate(all="ignore"):
            rho = float(np.float64(bank.template_mm_per_px) / np.float64(s))
        for k in range(kk):
            cx, cy = float(contacts[b, k, C_CX]), float(contacts[b, k, C_CY])
            if not (math.isfinite(s) and s > 0 and math.isfinite(rho) and rho > 0):
                res["matches"][b, k, 0] = NO_SCALE
            elif not (math.isfinite(cx) and math.isfinite(cy)):
                res["matches"][b, k, 0] = NO_PIXELS
            else:
                row = _match_row(depth[b], index[b], k, cx, cy, rho, bank, eps, max_shift, min_pixels, accept_score, accept_margin)
                res["matches"][b, k], res["scores"][b, k], res["patches"][b, k], res["rows"][b][k] = row.rec, row.scores, row.patch, row
    return res


def hold_device(dev, ref, exact_template=True):
    """the device's outputs (NumPy) against a reference of numpy_matches: patches bit for bit, integer fields exact, float fields within
    their bounds.  Prints each figure's worst ratio to its bound before asserting."""
    assert np.array_equal(dev["patches"].view(np.uint32), ref["patches"].view(np.uint32)), "patches differ in bits"
    dm, rm = dev["matches"], ref["matches"]
    assert np.array_equal(np.isnan(dm), np.isnan(rm)), (np.argwhere(np.isnan(dm) != np.isnan(rm))[:8])
    worst = {}
    B, K = rm.shape[:2]
    for b in range(B):
        for k in range(K):
            row = ref["rows"][b][k]
            if row is None or rm[b, k, 0] != OK:
                assert np.array_equal(dm[b, k], rm[b, k], equal_nan=True), (b, k, dm[b, k], rm[b, k])
                assert np.array_equal(dev["scores"][b, k], ref["scores"][b, k], equal_nan=True), (b, k)
                continue
            for name in INT_FIELDS:
                if exact_template or name not in ("template", "class", "label", "second_class"):
                    assert dm[b, k, F[name]] == rm[b, k, F[name]], (b, k, name, dm[b, k, F[name]], rm[b, k, F[name]])
            for name, tol in row.tol.items():
                d, r = dm[b, k, F[name]], rm[b, k, F[name]]
                if math.isnan(r):
                    assert math.isnan(d), (b, k, name)
                    continue
                err = abs(d - r)
                if name == "angle_rad" and row.per:
                    err = min(err, abs(row.per - err))
                worst[name] = max(worst.get(name, 0.0), err / tol if tol else (0.0 if err == 0 else math.inf))
                assert err <= tol, (b, k, name, d, r, err, tol)
            err = np.abs(dev["scores"][b, k] - ref["scores"][b, k]).max()
            worst["scores"] = max(worst.get("scores", 0.0), err / row.bound)
            assert err <= row.bound, (b, k, "scores", err, row.bound)
    print("worst error / bound:", {n: round(v, 4) for n, v in worst.items()})
    return worst
