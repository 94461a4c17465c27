"""The per-contact shape read-out's definition (include/vistaf_shape.h) written out in NumPy, and hand-made scenes for tests/test_shapes.py.

`numpy_shapes` follows the header step by step in float64; its fit is `np.linalg.lstsq` on the centred, scaled design matrix, with the
rank verdict from the singular values of that matrix with columns of unit length (the header's pivot floor says the same thing about
A - 2^-32 diag(A)).  `numpy_shapes_ne` is the same except for the fit, which forms the normal equations and uses `np.linalg.cholesky`, the
formulation of the device.  The distance between the two on a case (`distances`) is what the formulation alone costs there; the device,
which shares the normal equations and differs in summation order, is held to 4 times that (tests/test_shapes.py).
"""
import numpy as np

NCONTACT, NSHAPE = 16, 24
FIELDS = ("contact_pixels", "boundary_pixels", "footprint_cx", "footprint_cy", "major_axis_mm", "minor_axis_mm", "orientation_rad",
          "fit_pixels", "fit_status", "apex_x", "apex_y", "apex_depth_mm", "curvature_1_per_mm", "curvature_2_per_mm", "curvature_axis_rad",
          "radius_1_mm", "radius_2_mm", "fit_rms_mm")
S = {name: i for i, name in enumerate(FIELDS)}
EXACT = ("contact_pixels", "boundary_pixels", "fit_pixels", "fit_status")
OK, NONE, NOT_A_CAP = 0, 1, 2
C_PIXELS, C_CONTACT_PIXELS, C_PEAK, C_ARGMAX, C_X0, C_Y0, C_X1, C_Y1 = 0, 1, 4, 5, 9, 10, 11, 12      # VISTAF_CONTACT_* indices
FLOOR = 2.0 ** -32
ULP = 2.0 ** -52


def _half_angle(p, q):
    if p == 0.0 and q == 0.0:
        return 0.0
    t = 0.5 * np.arctan2(p, q)
    return np.pi / 2 if t <= -np.pi / 2 else t


def _poly(c, u, v):
    return c[0] + c[1] * u + c[2] * v + c[3] * (u * u) + c[4] * (u * v) + c[5] * (v * v)


def _fit_lstsq(X, d):
    norm = np.sqrt((X * X).sum(axis=0))
    if not (norm > 0).all():
        return None
    sv = np.linalg.svd(X / norm, compute_uv=False)
    if not sv.min() > np.sqrt(FLOOR):
        return None
    return np.linalg.lstsq(X, d, rcond=None)[0]


def _fit_normal_equations(X, d):
    A, rhs = X.T @ X, X.T @ d
    try:
        np.linalg.cholesky(A - FLOOR * np.diag(np.diag(A)))
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return None
    return np.linalg.solve(L.T, np.linalg.solve(L, rhs))


def table_box(row, h, w, margin=0):
    """The box of a contacts-table row as the read-outs' headers read it: ((bx0, by0, bx1, by1), clipped).  The first is the table's own
    integers; a value that is not finite or beyond +-1e9 gives no box, (0, 0, -1, -1).  `clipped` is (x0, y0, x1, y1), the box grown by
    `margin` on every side and cut to the h x w frame, or None where there is no box or nothing of it lies inside."""
    v = np.asarray(row, dtype=np.float64)[[C_X0, C_Y0, C_X1, C_Y1]]
    if not (np.isfinite(v).all() and (np.abs(v) <= 1.0e9).all()):
        return (0, 0, -1, -1), None
    bx0, by0, bx1, by1 = own = tuple(int(t) for t in v)
    x0, y0, x1, y1 = max(bx0 - margin, 0), max(by0 - margin, 0), min(bx1 + margin, w - 1), min(by1 + margin, h - 1)
    return own, ((x0, y0, x1, y1) if x1 >= x0 and y1 >= y0 else None)


def box_mask(clipped, h, w):
    m = np.zeros((h, w), bool)
    if clipped is not None:
        x0, y0, x1, y1 = clipped
        m[y0:y1 + 1, x0:x1 + 1] = True
    return m


def _shapes(depth_mm, contact_index, contacts, count, mm_per_px, eps, frac, fit):
    depth_mm, contact_index = np.asarray(depth_mm, dtype=np.float32), np.asarray(contact_index)
    contacts = np.asarray(contacts, dtype=np.float64)
    B, h, w = contact_index.shape
    K = contacts.shape[1]
    out = np.full((B, K, NSHAPE), np.nan)
    for b in range(B):
        d32 = np.nan_to_num(depth_mm[b], nan=0.0)
        s = float(mm_per_px[b])
        kk = min(max(int(count[b]), 0), K)
        for k in range(kk):
            row, o = contacts[b, k], out[b, k]
            (bx0, by0, bx1, by1), clipped = table_box(row, h, w)
            cm = box_mask(clipped, h, w) & (contact_index[b] == k) & (d32 > np.float32(eps))
            pad = np.pad(cm, 1)
            inner = cm & pad[1:-1, :-2] & pad[1:-1, 2:] & pad[:-2, 1:-1] & pad[2:, 1:-1]
            ys, xs = np.nonzero(cm)
            n = int(cm.sum())
            o[S["contact_pixels"]], o[S["boundary_pixels"]] = n, n - int(inner.sum())
            if n:
                xi, yi = [int(v) for v in xs], [int(v) for v in ys]                       # Python integers: exact sums
                dn = float(n)
                cx, cy = float(sum(xi)) / dn, float(sum(yi)) / dn
                mu20 = float(sum(x * x for x in xi)) / dn - cx * cx
                mu02 = float(sum(y * y for y in yi)) / dn - cy * cy
                mu11 = float(sum(x * y for x, y in zip(xi, yi))) / dn - cx * cy
                hd = (mu20 - mu02) / 2.0
                r, mean = np.sqrt(hd * hd + mu11 * mu11), (mu20 + mu02) / 2.0
                o[S["footprint_cx"]], o[S["footprint_cy"]] = cx, cy
                o[S["major_axis_mm"]] = 4.0 * np.sqrt(max(mean + r, 0.0)) * s
                o[S["minor_axis_mm"]] = 4.0 * np.sqrt(max(mean - r, 0.0)) * s
                o[S["orientation_rad"]] = _half_angle(2.0 * mu11, mu20 - mu02)
            thr = np.float32(frac * row[C_PEAK])
            fm = cm if frac == 0.0 else cm & (d32 >= thr)
            m = int(fm.sum())
            o[S["fit_pixels"]], o[S["fit_status"]] = m, NONE
            if m < 6:
                continue
            ys, xs = np.nonzero(fm)
            xc, yc = (bx0 + bx1) / 2.0, (by0 + by1) / 2.0
            hx, hy = max((bx1 - bx0) / 2.0, 1.0), max((by1 - by0) / 2.0, 1.0)
            u, v, d = (xs - xc) / hx, (ys - yc) / hy, d32[fm].astype(np.float64)
            X = np.stack([np.ones(m), u, v, u * u, u * v, v * v], axis=1)
            c = fit(X, d)
            if c is None:
                continue
            ax, ay = hx * s, hy * s
            q3, q4, q5 = c[3] / (ax * ax), c[4] / (ax * ay), c[5] / (ay * ay)
            mean, dev = q3 + q5, np.sqrt((q3 - q5) * (q3 - q5) + q4 * q4)
            low = mean <= 0.0
            k1, k2 = (mean - dev, mean + dev) if low else (mean + dev, mean - dev)
            status = OK if mean + dev < 0.0 else NOT_A_CAP
            o[S["fit_status"]] = status
            o[S["curvature_1_per_mm"]], o[S["curvature_2_per_mm"]] = k1, k2
            o[S["curvature_axis_rad"]] = _half_angle(-q4, q5 - q3) if low else _half_angle(q4, q3 - q5)
            if status == OK:
                det = 4.0 * c[3] * c[5] - c[4] * c[4]
                ua, va = (c[4] * c[2] - 2.0 * c[5] * c[1]) / det, (c[4] * c[1] - 2.0 * c[3] * c[2]) / det
                o[S["apex_x"]], o[S["apex_y"]], o[S["apex_depth_mm"]] = xc + ua * hx, yc + va * hy, _poly(c, ua, va)
                o[S["radius_1_mm"]], o[S["radius_2_mm"]] = -1.0 / k1, -1.0 / k2
            res = d - _poly(c, u, v)
            o[S["fit_rms_mm"]] = np.sqrt((res * res).sum() / m)
    return out


def numpy_shapes(depth_mm, contact_index, contacts, count, mm_per_px, eps, frac):
    """depth_mm [B,h,w] float32, contact_index [B,h,w] int8, contacts [B,K,16] float64, count [B], mm_per_px [B] -> shapes [B,K,24] float64"""
    return _shapes(depth_mm, contact_index, contacts, count, mm_per_px, eps, frac, _fit_lstsq)


def numpy_shapes_ne(depth_mm, contact_index, contacts, count, mm_per_px, eps, frac):
    return _shapes(depth_mm, contact_index, contacts, count, mm_per_px, eps, frac, _fit_normal_equations)


def exact_equal(a, b):
    """the exact fields equal and NaN in the same places of the whole table"""
    a, b = np.asarray(a), np.asarray(b)
    cols = [S[f] for f in EXACT]
    na, nb = np.isnan(a[..., cols]), np.isnan(b[..., cols])
    return bool(a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(na, nb) and
                np.array_equal(a[..., cols][~na], b[..., cols][~nb]))


def distances(a, b, contacts, mm_per_px):
    """Largest distance between two shape tables of the same frames, every float field relative to its own scale (taken from `b`, the
    reference, and the contacts table): footprint centroid and apex position against the box size in pixels, the axes against the box size
    in mm, the curvatures against |curvature_1|, apex depth and rms against the peak.  Directions are compared as tensor components --
    (l1 - l2) (cos 2t, sin 2t) of the second-moment tensor against the squared box size, (k1 - k2) (cos 2t, sin 2t) of the Hessian
    against |curvature_1| -- so an isotropic footprint or cap, whose direction is arbitrary, needs no exception.  A radius is -1/k, so an
    error dk of the curvature moves it by dk * R^2: it is held against R^2 * |curvature_1|, which asks of it what is asked of k.
    Returns {group: distance}; fields NaN in both tables do not count."""
    a, b, contacts = np.asarray(a), np.asarray(b), np.asarray(contacts)
    out = {"footprint": 0.0, "fit": 0.0}
    for f in np.ndindex(a.shape[:2]):
        ra, rb, row, s = a[f], b[f], contacts[f], float(mm_per_px[f[0]])
        if np.isnan(rb[0]):
            continue
        box = max(row[C_X1] - row[C_X0], row[C_Y1] - row[C_Y0], 1.0)
        peak = abs(row[C_PEAK])

        def tensor(r, lo, hi, ang):
            return np.array([(r[lo] - r[hi]) * np.cos(2 * r[ang]), (r[lo] - r[hi]) * np.sin(2 * r[ang])])
        if rb[S["contact_pixels"]] > 0:
            d = [abs(ra[S[n]] - rb[S[n]]) / box for n in ("footprint_cx", "footprint_cy")]
            d += [abs(ra[S[n]] - rb[S[n]]) / (box * s) for n in ("major_axis_mm", "minor_axis_mm")]
            la, lb = [[(r[S[n]] / (4 * s)) ** 2 for n in ("major_axis_mm", "minor_axis_mm")] + [r[S["orientation_rad"]]] for r in (ra, rb)]
            d += list(np.abs(tensor(la, 0, 1, 2) - tensor(lb, 0, 1, 2)) / (box * box))
            out["footprint"] = max([out["footprint"]] + d)
        if rb[S["fit_status"]] != NONE:
            k1 = abs(rb[S["curvature_1_per_mm"]])
            d = [abs(ra[S[n]] - rb[S[n]]) / k1 for n in ("curvature_1_per_mm", "curvature_2_per_mm")]
            c1, c2, ca = S["curvature_1_per_mm"], S["curvature_2_per_mm"], S["curvature_axis_rad"]
            d += list(np.abs(tensor(ra, c1, c2, ca) - tensor(rb, c1, c2, ca)) / k1)
            d.append(abs(ra[S["fit_rms_mm"]] - rb[S["fit_rms_mm"]]) / peak)
            if rb[S["fit_status"]] == OK:
                d += [abs(ra[S[n]] - rb[S[n]]) / box for n in ("apex_x", "apex_y")]
                d.append(abs(ra[S["apex_depth_mm"]] - rb[S["apex_depth_mm"]]) / peak)
                d += [abs(ra[S[n]] - rb[S[n]]) / (rb[S[n]] ** 2 * k1) for n in ("radius_1_mm", "radius_2_mm")]
            out["fit"] = max([out["fit"]] + d)
    return out


# ---------------------------------------------------------------------------------------------------------------- scenes
def table_from_planes(depth_mm, contact_index, K, eps, count=None):
    """the rows vistaf_ftp_contacts would have written for these planes, as far as the shape read-out reads them (pixels, contact pixels,
    peak, arg-max, box); rows without a pixel in the plane stay NaN.  count defaults to the number of rows present."""
    depth_mm, contact_index = np.asarray(depth_mm, dtype=np.float32), np.asarray(contact_index)
    B, h, w = contact_index.shape
    tab = np.full((B, K, NCONTACT), np.nan)
    cnt = np.zeros(B, np.int32)
    for b in range(B):
        d = np.nan_to_num(depth_mm[b], nan=0.0)
        for k in range(K):
            mk = contact_index[b] == k
            if not mk.any():
                continue
            cnt[b] = k + 1
            ys, xs = np.nonzero(mk)
            flat = np.flatnonzero(mk.ravel())
            j = int(np.argmax(d.ravel()[flat]))
            tab[b, k, [C_PIXELS, C_CONTACT_PIXELS, C_PEAK, C_ARGMAX]] = [mk.sum(), (mk & (d > np.float32(eps))).sum(), d.ravel()[flat][j], flat[j]]
            tab[b, k, [C_X0, C_Y0, C_X1, C_Y1]] = [xs.min(), ys.min(), xs.max(), ys.max()]
    return tab, (cnt if count is None else np.asarray(count, np.int32))


def quadric(h, w, xa, ya, d0, r1, r2, angle, s):
    """d = d0 - (u'^2 / (2 r1) + v'^2 / (2 r2)) in float64: apex (xa, ya) in pixels, radii in mm along axes turned by `angle`, s mm per pixel.
    A negative radius bends upwards (r1 < 0 < r2: a saddle; both negative: a bowl)."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    xm, ym = (xx - xa) * s, (yy - ya) * s
    up, vp = np.cos(angle) * xm + np.sin(angle) * ym, -np.sin(angle) * xm + np.cos(angle) * ym
    return d0 - (up * up / (2.0 * r1) + vp * vp / (2.0 * r2))


class Scene:
    """one frame under construction: paint(k, mask, depth) labels the mask's pixels with row k and gives them depths"""

    def __init__(self, h, w, background=np.nan):
        self.depth = np.full((h, w), background, np.float32)
        self.index = np.full((h, w), -1, np.int8)

    def paint(self, k, mask, depth):
        self.index[mask] = k
        self.depth[mask] = np.broadcast_to(np.asarray(depth, dtype=np.float64), mask.shape)[mask].astype(np.float32)
        return self


def rect(h, w, x0, y0, x1, y1):
    m = np.zeros((h, w), bool)
    m[y0:y1 + 1, x0:x1 + 1] = True
    return m


def disc(h, w, xa, ya, r_out, r_in=-1.0):
    yy, xx = np.mgrid[0:h, 0:w]
    r2 = (xx - xa) ** 2 + (yy - ya) ** 2
    return (r2 <= r_out * r_out) & (r2 > r_in * abs(r_in))


H, W, EPS = 37, 53, 0.01


def pack(scenes, K, s, frac, eps=EPS, count=None):
    """a case: the arguments of numpy_shapes / ContactShapes.measure for a list of Scene frames"""
    depth, index = np.stack([sc.depth for sc in scenes]), np.stack([sc.index for sc in scenes])
    tab, cnt = table_from_planes(depth, index, K, eps, count)
    mpp = np.full(len(scenes), s) if np.isscalar(s) else np.asarray(s, dtype=np.float64)
    return {"depth": depth, "index": index, "tab": tab, "count": cnt, "mpp": mpp, "eps": eps, "frac": frac, "K": K}


def frames_37x53():
    """the single-frame scenes of the base shape, K = 4, by name"""
    h, w = H, W
    f = {}
    f["single_pixel"] = Scene(h, w).paint(0, rect(h, w, 10, 7, 10, 7), 0.5)
    f["lines"] = Scene(h, w).paint(0, rect(h, w, 20, 30, 28, 30), 0.5 + 0.01 * np.arange(w)[None, :])
    diag = np.zeros((h, w), bool)
    diag[np.arange(5, 14), np.arange(8, 17)] = True
    f["lines"].paint(1, diag, 0.4)
    f["lines"].paint(2, rect(h, w, 40, 3, 51, 4), quadric(h, w, 45.5, 3.5, 0.6, 30.0, 30.0, 0.0, 0.2))      # two rows: 1, v, v*v dependent
    six = np.zeros((h, w), bool)
    for x, y in ((1, 0), (0, 1), (1, 1), (2, 1), (1, 2), (0, 0)):
        six[20 + y, 30 + x] = True
    f["six_pixels"] = Scene(h, w).paint(0, rect(h, w, 29, 19, 33, 23), 0.3).paint(0, six, quadric(h, w, 31.2, 20.7, 1.0, 4.0, 6.0, 0.3, 0.5))
    f["whole_frame"] = Scene(h, w).paint(0, rect(h, w, 0, 0, w - 1, h - 1), quadric(h, w, 25.3, 17.6, 1.5, 90.0, 140.0, 0.4, 0.31))
    c = Scene(h, w, 0.0)
    for k, (x0, y0) in enumerate(((0, 0), (w - 7, 0), (0, h - 6), (w - 7, h - 6))):
        c.paint(k, rect(h, w, x0, y0, x0 + 6, y0 + 5), quadric(h, w, x0 + 2.8 + 0.1 * k, y0 + 2.4, 0.9 - 0.1 * k, 8.0, 12.0, 0.2 * k, 0.25))
    f["corners"] = c
    f["ring"] = Scene(h, w).paint(0, disc(h, w, 26, 18, 12.0, 6.0), quadric(h, w, 26.4, 17.7, 0.8, 60.0, 45.0, -0.5, 0.2))
    sb = Scene(h, w)
    sb.paint(0, disc(h, w, 12, 18, 9.5), quadric(h, w, 12.3, 17.8, 0.7, -20.0, 20.0, 0.3, 0.2))              # saddle
    sb.paint(1, disc(h, w, 38, 18, 9.5), quadric(h, w, 38.2, 18.1, 0.3, -25.0, -15.0, -0.2, 0.2))            # bowl: deepest at the rim
    f["saddle_bowl"] = sb
    ne = Scene(h, w).paint(0, rect(h, w, 8, 6, 30, 25), quadric(h, w, 19.4, 15.2, 1.2, 40.0, 25.0, 1.0, 0.3))
    ne.depth[10:13, 12:15] = np.nan
    ne.depth[20, 9:28] = 0.005                                                             # <= eps: a slit through the contact
    ne.depth[15, 19] = EPS
    f["nan_and_eps"] = ne
    st = Scene(h, w).paint(0, disc(h, w, 14, 12, 7.5), quadric(h, w, 14.2, 11.9, 1.0, 20.0, 30.0, 0.7, 0.2))
    st.paint(1, disc(h, w, 36, 24, 6.5), quadric(h, w, 36.0, 24.3, 0.8, 15.0, 15.0, 0.0, 0.2))
    st.paint(2, rect(h, w, 30, 2, 40, 9), 0.9).paint(3, rect(h, w, 2, 28, 9, 34), 0.9).paint(5, rect(h, w, 45, 28, 50, 34), 0.9)
    f["stray_rows"] = st                                                                   # with count 2: rows 2, 3, 5 of the plane are nobody's
    return f


def cases():
    """every direct case by name: the arguments of numpy_shapes / ContactShapes.measure"""
    f = frames_37x53()
    c = {name: pack([f[name]], 4, 0.2, 0.5) for name in ("single_pixel", "lines", "whole_frame", "corners", "ring", "saddle_bowl", "nan_and_eps")}
    c["six_pixels"] = pack([f["six_pixels"]], 4, 0.5, 0.5)
    c["whole_frame_all_pixels"] = pack([f["whole_frame"]], 4, 0.31, 0.0)
    c["stray_rows_and_count_0"] = pack([f["stray_rows"], f["stray_rows"]], 4, 0.2, 0.5, count=[2, 0])
    c["count_above_k"] = pack([f["stray_rows"]], 2, 0.2, 0.5, count=[5])
    many = Scene(H, W, 0.0)
    rng = np.random.default_rng(64)
    for k in range(64):
        r, q = divmod(k, 8)
        m = np.zeros((H, W), bool)
        cells = rng.permutation(9)[:1 + k % 9]
        m[1 + 4 * r + cells // 3, 1 + 6 * q + cells % 3] = True
        many.paint(k, m, rng.uniform(0.2, 1.0, (H, W)))
    c["k64"] = pack([many], 64, 0.2, 0.0)
    c["mixed_batch"] = pack([f[n] for n in ("corners", "ring", "saddle_bowl", "nan_and_eps", "stray_rows")], 4, [0.2, 0.25, 0.3, 0.2, 0.22], 0.5,
                            count=[4, 1, 2, 1, 0])
    strip = Scene(3, 1100).paint(0, rect(3, 1100, 0, 0, 1099, 2), quadric(3, 1100, 560.3, 1.2, 2.0, 4000.0, 3.0, 0.0, 0.1))
    c["strip_3x1100"] = pack([strip], 4, 0.1, 0.5)
    big = Scene(150, 150, 0.0).paint(0, rect(150, 150, 9, 12, 138, 141), quadric(150, 150, 71.7, 80.2, 1.8, 700.0, 500.0, 0.6, 0.15))
    c["big_130x130"] = pack([big], 4, 0.15, 0.25)
    return c


def analytic_case(angle, h=H, w=W, xa=26.37, ya=18.21, d0=1.25, r1=18.0, r2=41.0, s=0.23, level=0.35, frac=0.5):
    """a cap d0 - (u'^2/2 r1 + v'^2/2 r2) sampled in float32, contact = the pixels deeper than `level`; returns (case, truth, d64)"""
    d64 = quadric(h, w, xa, ya, d0, r1, r2, angle, s)
    sc = Scene(h, w, 0.0).paint(0, d64 > level, d64)
    t = (angle + np.pi / 2) % np.pi - np.pi / 2
    truth = {"apex_x": xa, "apex_y": ya, "apex_depth_mm": d0, "radius_1_mm": r1, "radius_2_mm": r2, "curvature_1_per_mm": -1.0 / r1,
             "curvature_2_per_mm": -1.0 / r2, "curvature_axis_rad": np.pi / 2 if t <= -np.pi / 2 else t}
    return pack([sc], 4, s, frac), truth, d64


def analytic_errors(row, truth, case):
    """errors of one fitted row against the true surface, relative to the scales of `distances`"""
    box = max(case["tab"][0, 0, C_X1] - case["tab"][0, 0, C_X0], case["tab"][0, 0, C_Y1] - case["tab"][0, 0, C_Y0])
    k1 = abs(truth["curvature_1_per_mm"])
    e = [abs(row[S[n]] - truth[n]) / box for n in ("apex_x", "apex_y")]
    e.append(abs(row[S["apex_depth_mm"]] - truth["apex_depth_mm"]) / truth["apex_depth_mm"])
    e += [abs(row[S[n]] - truth[n]) / (truth[n] ** 2 * k1) for n in ("radius_1_mm", "radius_2_mm")]
    dk = truth["curvature_1_per_mm"] - truth["curvature_2_per_mm"]
    gk = row[S["curvature_1_per_mm"]] - row[S["curvature_2_per_mm"]]
    e.append(abs(gk * np.cos(2 * row[S["curvature_axis_rad"]]) - dk * np.cos(2 * truth["curvature_axis_rad"])) / k1)
    e.append(abs(gk * np.sin(2 * row[S["curvature_axis_rad"]]) - dk * np.sin(2 * truth["curvature_axis_rad"])) / k1)
    return max(e)
