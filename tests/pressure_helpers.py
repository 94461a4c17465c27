"""Inputs and the NumPy restatements of the pressure read-out (include/vistaf_pressure.h) for tests/test_pressure.py.

`numpy_pressure` is the definition written with np.fft.rfft2 / irfft2 in float64; `matmul_pressure` writes the same definition with explicit
DFT matrices (twiddles from longdouble angles) and np.matmul, the Hermitian weights spelled out.  The distance between the two is what
float64 arithmetic leaves open, and is the yardstick of the device's plane.  `tables` applies the table definitions to a float32 plane with
math.fsum: every sum is the exact sum rounded once.
"""
import math

import numpy as np

import shapes_helpers as SH

FIELDS = ("pixels", "force_model_N", "tensile_model_N", "force_N", "mean_kPa", "peak_kPa", "peak_index", "cop_x", "cop_y", "offset_x_mm",
          "offset_y_mm", "peak_over_mean", "edge_share")
FRAME_FIELDS = ("contacts", "force_model_N", "tensile_model_N", "outside_model_N", "scale", "E_effective_MPa", "peak_kPa", "peak_index", "peak_row",
                "cop_x", "cop_y", "status")
R = {n: i for i, n in enumerate(FIELDS)}
FR = {n: i for i, n in enumerate(FRAME_FIELDS)}
NROW, NFRAME, NCONTACT = 16, 12, 16
BBOX = (9, 10, 11, 12)                                    # VISTAF_CONTACT_BBOX_X0, Y0, X1, Y1
EXACT = ("pixels", "peak_kPa", "peak_index")              # a count, a stored float32 and an index: equal, not close
FRAME_EXACT = ("contacts", "peak_kPa", "peak_index", "peak_row", "status")
K = 4
U2 = 2.0 ** -53


# ------------------------------------------------------------------------------------------------------------ the model
def layer_S(x, nu):
    """header, step 2: ((3-4nu) sinh 2x - 2x) / ((3-4nu) cosh 2x + 2x^2 + 5 - 12nu + 8nu^2), written without the overflow"""
    x = np.asarray(x, dtype=np.float64)
    k = 3.0 - 4.0 * nu
    e = np.exp(-2.0 * x)
    return (k * (1.0 - e * e) - 4.0 * x * e) / (k * (1.0 + e * e) + (4.0 * x * x + (10.0 - 24.0 * nu + 16.0 * nu * nu)) * e)


def winkler_modulus(E, nu):
    """the oedometric modulus M: a layer of thickness t -> 0 carries p = M u / t"""
    return E * (1.0 - nu) / ((1.0 + nu) * (1.0 - 2.0 * nu))


def gain(q, E, nu, t):
    """G(q) in MPa/mm for q in rad/mm"""
    q = np.asarray(q, dtype=np.float64)
    Es = E / (1.0 - nu * nu)
    if math.isinf(t):
        return Es * q / 2.0
    with np.errstate(divide="ignore", invalid="ignore"):
        g = Es * q / (2.0 * layer_S(q * t, nu))
    return np.where(q == 0.0, E * (1.0 - nu) / ((1.0 + nu) * (1.0 - 2.0 * nu) * t), g)


def clean(depth32, eps):
    d = np.asarray(depth32, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        keep = np.isfinite(d) & (d > np.float32(eps))
    return np.where(keep, d, np.float32(0.0)).astype(np.float64)


def _q(Ph, Pw, s):
    a, c = np.arange(Ph), np.arange(Pw // 2 + 1)
    fy = np.where(a <= Ph // 2, a, a - Ph) / float(Ph)
    fx = c / float(Pw)
    return 2.0 * np.pi * np.sqrt(fx[None, :] * fx[None, :] + fy[:, None] * fy[:, None]) / s


def numpy_pressure(depth32, mm_per_px, eps, pad, E, nu, t, status=None, full=False):
    """float64 planes [B,h,w] in kPa (the padded [B,Ph,Pw] planes with full=True) by rfft2 / irfft2"""
    d = np.asarray(depth32, dtype=np.float32)
    B, h, w = d.shape
    Ph, Pw = h + pad, w + pad
    out = np.zeros((B, Ph, Pw) if full else (B, h, w))
    for b in range(B):
        if status is not None and status[b] != 0:
            continue
        spec = np.fft.rfft2(clean(d[b], eps), s=(Ph, Pw)) * gain(_q(Ph, Pw, float(mm_per_px[b])), E, nu, t)
        p = 1000.0 * np.fft.irfft2(spec, s=(Ph, Pw))
        out[b] = p if full else p[:h, :w]
    return out


def _twiddle(n_rows, n_cols, size, sign):
    """exp(sign 2 pi i r c / size) [n_rows, n_cols], the angle reduced exactly and evaluated in longdouble"""
    m = (np.arange(n_rows, dtype=np.int64)[:, None] * np.arange(n_cols, dtype=np.int64)[None, :]) % size
    ang = 2.0 * np.pi * np.longdouble(1.0) * m.astype(np.longdouble) / np.longdouble(size)
    return np.cos(ang).astype(np.float64) + 1j * sign * np.sin(ang).astype(np.float64)


def matmul_pressure(depth32, mm_per_px, eps, pad, E, nu, t, status=None):
    """the same planes by four dense contractions, in the order the header's steps give them"""
    d = np.asarray(depth32, dtype=np.float32)
    B, h, w = d.shape
    Ph, Pw = h + pad, w + pad
    Wh = Pw // 2 + 1
    Ex, Ey = _twiddle(w, Wh, Pw, -1), _twiddle(Ph, h, Ph, -1)
    Fy, Fx = _twiddle(h, Ph, Ph, +1), _twiddle(Wh, w, Pw, +1)
    c = np.arange(Wh)
    wgt = np.where((c == 0) | (2 * c == Pw), 1.0, 2.0)
    out = np.zeros((B, h, w))
    for b in range(B):
        if status is not None and status[b] != 0:
            continue
        spec = np.matmul(Ey, np.matmul(clean(d[b], eps), Ex))
        z = spec * (gain(_q(Ph, Pw, float(mm_per_px[b])), E, nu, t) * wgt[None, :] * (1000.0 / (float(Ph) * float(Pw))))
        out[b] = np.matmul(np.matmul(Fy, z), Fx).real
    return out


# ------------------------------------------------------------------------------------------------------------ the tables
def tables(p32, mm_per_px, K, E, index=None, contacts=None, count=None, force=None, status=None):
    """(rows [B,K,16] or None, frame [B,12], terms): the header's step 4 on the float32 planes p32 with math.fsum.  terms[(b, k)] is the
    number of pixels of the row, terms[b] that of the frame: the N of the tolerance."""
    p32 = np.asarray(p32, dtype=np.float32)
    B, h, w = p32.shape
    rows = np.full((B, K, NROW), np.nan) if index is not None else None
    frame = np.full((B, NFRAME), np.nan)
    terms = {}
    for b in range(B):
        st = 0 if status is None else int(status[b])
        frame[b, FR["status"]] = st
        if st != 0:
            continue
        p = p32[b].astype(np.float64)
        s = float(mm_per_px[b])
        px = s * s
        F = np.nan if force is None else float(force[b])
        kk = 0 if index is None else min(max(int(count[b]), 0), K)
        raw = []
        for k in range(kk):
            m = SH.box_mask(SH.table_box(contacts[b, k], h, w)[1], h, w) & (index[b] == k)
            ys, xs = np.nonzero(m)
            n = len(ys)
            v = p[ys, xs]
            vp, vn = np.maximum(v, 0.0), np.maximum(-v, 0.0)
            Pp, Pn = math.fsum(vp), math.fsum(vn)
            Xp, Yp = math.fsum(xs * vp), math.fsum(ys * vp)
            pm = np.pad(m, 1)
            inner = pm[:-2, 1:-1] & pm[2:, 1:-1] & pm[1:-1, :-2] & pm[1:-1, 2:]      # all four neighbours in the frame and in the row
            Pe = math.fsum(vp[~inner[ys, xs]])
            raw.append((Pp, Xp, Yp))
            r = rows[b, k]
            r[R["pixels"]] = n
            r[R["force_model_N"]] = 1e-3 * px * Pp
            r[R["tensile_model_N"]] = 1e-3 * px * Pn
            if n:
                i = int(np.argmax(v))                                                # first of the largest, in pixel order
                mean = (Pp - Pn) / n
                r[R["mean_kPa"]], r[R["peak_kPa"]], r[R["peak_index"]] = mean, v[i], ys[i] * w + xs[i]
                if mean > 0.0:
                    r[R["peak_over_mean"]] = v[i] / mean
            if Pp != 0.0:
                cx, cy = Xp / Pp, Yp / Pp
                r[R["cop_x"]], r[R["cop_y"]], r[R["edge_share"]] = cx, cy, Pe / Pp
                r[R["offset_x_mm"]] = (cx - float(xs.sum()) / n) * s
                r[R["offset_y_mm"]] = (cy - float(ys.sum()) / n) * s
            terms[(b, k)] = n
        fm = 0.0
        for k in range(kk):
            fm += rows[b, k, R["force_model_N"]]
        for k in range(kk):
            rows[b, k, R["force_N"]] = np.nan if force is None else (0.0 if fm == 0.0 else F * (rows[b, k, R["force_model_N"]] / fm))
        own = np.zeros((h, w), dtype=bool) if index is None else (index[b] >= 0) & (index[b] < kk)
        sp, sx, sy = (math.fsum(t[j] for t in raw) for j in range(3))
        i = int(np.argmax(p))
        scale = F / fm if (force is not None and fm > 0.0) else np.nan
        f = frame[b]
        f[FR["contacts"]] = kk
        f[FR["force_model_N"]] = fm
        f[FR["tensile_model_N"]] = 1e-3 * px * math.fsum(np.maximum(-p, 0.0).ravel())
        f[FR["outside_model_N"]] = 1e-3 * px * math.fsum(np.abs(p[~own]))
        f[FR["scale"]], f[FR["E_effective_MPa"]] = scale, scale * E
        f[FR["peak_kPa"]], f[FR["peak_index"]] = p.ravel()[i], i
        f[FR["peak_row"]] = index[b].ravel()[i] if own.ravel()[i] else -1
        if sp != 0.0:
            f[FR["cop_x"]], f[FR["cop_y"]] = sx / sp, sy / sp
        terms[b] = h * w
    return rows, frame, terms


def row_scales(rows, frame, mm_per_px, h, w):
    """the magnitude each float field's rounding is relative to: the field itself where its sums have one sign, the sum of the magnitudes
    where two things of one sign are subtracted (the mean, the offsets and what is divided by them)"""
    sc = np.abs(rows).copy()
    for b in range(rows.shape[0]):
        s = float(mm_per_px[b])
        for k in range(rows.shape[1]):
            r = rows[b, k]
            if not np.isfinite(r[0]) or r[0] == 0:
                continue
            gross = (r[R["force_model_N"]] + r[R["tensile_model_N"]]) / (1e-3 * s * s) / r[0]        # (Pp + Pn) / n
            sc[b, k, R["mean_kPa"]] = gross
            if np.isfinite(r[R["peak_over_mean"]]):
                sc[b, k, R["peak_over_mean"]] = abs(r[R["peak_over_mean"]]) * gross / abs(r[R["mean_kPa"]])
            sc[b, k, R["offset_x_mm"]] = 2.0 * w * s
            sc[b, k, R["offset_y_mm"]] = 2.0 * h * s
    return sc


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------------------ analytic surfaces
def radius_mm(n, s):
    yy, xx = np.mgrid[0:n, 0:n].astype(np.float64)
    return np.hypot(xx - n // 2, yy - n // 2) * s


def hertz(n, s, E, nu, R_mm, a_mm):
    """(u [n,n] mm, p [n,n] MPa, p0): the exact surface displacement of a half-space under a ball of radius R at contact radius a, inside and
    outside the contact, and the pressure that causes it (Johnson, Contact Mechanics, 3.41-3.42)"""
    r = radius_mm(n, s)
    Es = E / (1.0 - nu * nu)
    p0 = 2.0 * Es * a_mm / (np.pi * R_mm)
    inside = r <= a_mm
    ro = np.where(inside, a_mm, r)
    u_in = np.pi * p0 / (4.0 * Es * a_mm) * (2.0 * a_mm * a_mm - r * r)
    u_out = p0 / (2.0 * Es * a_mm) * ((2.0 * a_mm * a_mm - ro * ro) * np.arcsin(a_mm / ro) + ro * a_mm * np.sqrt(1.0 - (a_mm / ro) ** 2))
    p = p0 * np.sqrt(np.maximum(1.0 - (r / a_mm) ** 2, 0.0))
    return np.where(inside, u_in, u_out), p, p0


def gaussian_dent(n, s, depth_mm=0.5, width_mm=4.0):
    return depth_mm * np.exp(-(radius_mm(n, s) / width_mm) ** 2)


def disc_contact(mask):
    """index plane, one-row contacts table and count of a single footprint"""
    h, w = mask.shape
    ys, xs = np.nonzero(mask)
    index = np.where(mask, 0, -1).astype(np.int8)[None]
    tab = np.full((1, 1, NCONTACT), np.nan)
    tab[0, 0, list(BBOX)] = (xs.min(), ys.min(), xs.max(), ys.max())
    return index, tab, np.array([1], dtype=np.int32)


# ------------------------------------------------------------------------------------------------------------ the direct cases
EPS = 0.01
SIZES = ((37, 53, 11), (40, 52, 1), (16, 16, 0))          # h, w, pad: 48 x 64 (even Pw); 41 x 53 (odd Pw, no multiple of 16); no padding
BIG = (151, 203, 32)
MODELS = {"halfspace": (0.5, 0.45, math.inf), "layer": (0.8, 0.3, 1.5)}      # E (MPa), nu, thickness (mm): the tests' own, not a material's


def _bumps(h, w, spec):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    d = np.zeros((h, w))
    for x0, y0, amp, sig in spec:
        d += amp * np.exp(-((xx - x0 * w) ** 2 + (yy - y0 * h) ** 2) / (2.0 * (sig * min(h, w)) ** 2))
    return d


def _label(depth32, spec, h, w, K):
    """index plane, table and count of a frame of bumps: bump j owns the pixels above eps that are nearest to its centre, the rows ordered
    by peak depth, descending, as vistaf_ftp_contacts orders them; contacts beyond K are counted and left out of the plane"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    with np.errstate(invalid="ignore"):
        on = np.isfinite(depth32) & (depth32 > np.float32(EPS))
    near = np.argmin(np.stack([(xx - x0 * w) ** 2 + (yy - y0 * h) ** 2 for x0, y0, _, _ in spec]), axis=0)
    owners = [j for j in np.argsort([-a for _, _, a, _ in spec], kind="stable") if (on & (near == j)).any()]
    index = np.full((h, w), -1, dtype=np.int8)
    tab = np.full((K, NCONTACT), np.nan)
    for k, j in enumerate(owners[:K]):
        m = on & (near == j)
        ys, xs = np.nonzero(m)
        index[m] = k
        tab[k, list(BBOX)] = (xs.min(), ys.min(), xs.max(), ys.max())
        tab[k, 0] = m.sum()
    return index, tab, len(owners)


def frame_kinds(h, w, K=K):
    """the four kinds of frame of the direct cases: depth [h,w] f32, index, table, count, status"""
    out = {}
    z = np.zeros((h, w), dtype=np.float32)
    out["empty"] = (z, np.full((h, w), -1, dtype=np.int8), np.full((K, NCONTACT), np.nan), 0, 0)
    spec = [(0.45, 0.5, 0.9, 0.16)]
    d = _bumps(h, w, spec).astype(np.float32)
    d[h // 2 - 1:h // 2 + 1, w // 3:w // 3 + 2] = np.nan                  # NaN patches inside and outside the contact
    d[0:2, w - 3:w] = np.nan
    d[h - 3:h, 0:4] = -0.3                                                # negative pixels
    d[1, 1] = -np.inf
    out["bump"] = (d,) + _label(d, spec, h, w, K) + (0,)
    spec = [(0.2, 0.25, 0.7, 0.09), (0.75, 0.3, 1.1, 0.08), (0.3, 0.78, 0.5, 0.07), (0.8, 0.8, 0.9, 0.06), (0.52, 0.52, 0.3, 0.05)]
    d = _bumps(h, w, spec).astype(np.float32)
    e32 = np.float32(EPS)
    d[0, 0], d[0, 1] = e32, np.nextafter(e32, np.float32(1.0))            # at eps (not a contact pixel) and one float32 step above (one)
    d[h - 1, w - 1], d[h - 1, w - 2] = e32, np.nextafter(e32, np.float32(1.0))
    out["multi"] = (d,) + _label(d, spec, h, w, K) + (0,)
    out["bad"] = (np.full((h, w), np.inf, dtype=np.float32), np.full((h, w), -1, dtype=np.int8), np.full((K, NCONTACT), np.nan), 0, 2)
    return out


def batch(h, w, kinds, K=K):
    """a direct case: the frames `kinds` in order, a scale and a force per frame"""
    fk = frame_kinds(h, w, K)
    fr = [fk[k] for k in kinds]
    B = len(fr)
    return {"depth": np.stack([f[0] for f in fr]), "index": np.stack([f[1] for f in fr]), "tab": np.stack([f[2] for f in fr]),
            "count": np.array([f[3] for f in fr], dtype=np.int32), "status": np.array([f[4] for f in fr], dtype=np.int32),
            "mpp": np.array([0.05 + 0.013 * b for b in range(B)]), "force": np.array([1.5 + 0.6 * b for b in range(B)]), "eps": EPS, "kinds": kinds}


def cases():
    """name -> (case, pad).  Every size has two batches of three frames, which together hold the four kinds of frame; the large size has one
    batch of two."""
    out = {}
    for h, w, pad in SIZES:
        out["%dx%d_a" % (h, w)] = (batch(h, w, ("empty", "bump", "multi")), pad)
        out["%dx%d_b" % (h, w)] = (batch(h, w, ("multi", "bad", "bump")), pad)
    out["%dx%d" % BIG[:2]] = (batch(BIG[0], BIG[1], ("bump", "multi")), BIG[2])
    return out
