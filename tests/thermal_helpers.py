"""The thermal read-out's definition (include/vistaf_thermal.h) written out in NumPy, and hand-made scenes for tests/test_thermal.py.

`numpy_register` is the registration formula in float64, vectorised: the same sequence of IEEE operations as the device, so the device must
equal it bit for bit.  `numpy_thermal` follows the contact and frame rows step by step with plain float64 sums in row-major order;
`numpy_thermal_fsum` is the same with `math.fsum` (correctly rounded sums).  The distance between the two on a case (`distances`) is what the
summation order alone costs there; the device, which differs from `numpy_thermal` in summation order only, is held to 4 times that
(tests/test_thermal.py).  The scenes are built with the painter of tests/shapes_helpers.py.
"""
import math

import numpy as np

import shapes_helpers as SH

NCONTACT, NTHERMAL, NTHERMALFRAME, NINFO = 16, 16, 8, 12
FIELDS = ("contact_pixels", "valid_pixels", "coverage", "mean_C", "weighted_mean_C", "min_C", "max_C", "std_C", "peak_temp_C", "surround_pixels",
          "surround_mean_C", "contrast_C")
FRAME_FIELDS = ("registered_pixels", "skin_mean_C", "contact_pixels", "contact_mean_C", "contrast_C", "hottest_contact", "coldest_contact")
T = {name: i for i, name in enumerate(FIELDS)}
F = {name: i for i, name in enumerate(FRAME_FIELDS)}
COUNTS = ("contact_pixels", "valid_pixels", "surround_pixels")                       # integers: equal
SELECTED = ("min_C", "max_C", "peak_temp_C")                                           # selections: bit-equal
SUMMED = ("coverage", "mean_C", "weighted_mean_C", "std_C", "surround_mean_C", "contrast_C")
FRAME_EXACT = ("registered_pixels", "contact_pixels", "hottest_contact", "coldest_contact")
FRAME_SUMMED = ("skin_mean_C", "contact_mean_C", "contrast_C")
ULP = 2.0 ** -52
H, W, EPS = SH.H, SH.W, SH.EPS                                                       # the crop: 37 x 53
PH, PW, ORIGIN = 61, 83, (9, 5)                                                      # the photograph and the crop's origin (x1, y1) in it


# ---------------------------------------------------------------------------------------------------------------- registration
def numpy_register(temp_map, info, h, w, crop_x1, crop_y1, apply_global_shift=True):
    """temp_map [B,PH,PW] float32, info [B,12] float64 or None -> [B,h,w] float32, the header's formula operation by operation"""
    tm = np.asarray(temp_map, dtype=np.float32)
    B, ph, pw = tm.shape
    out = np.empty((B, h, w), np.float32)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    for b in range(B):
        sx = sy = np.float64(0.0)
        M = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0])
        if info is not None:
            row = np.asarray(info, dtype=np.float64)[b]
            M = row[3:9]
            if apply_global_shift:
                sx, sy = row[0], row[1]
        with np.errstate(invalid="ignore", over="ignore"):
            u = ((M[0] * xx + M[1] * yy) + M[2]) + np.float64(crop_x1) - sx
            v = ((M[3] * xx + M[4] * yy) + M[5]) + np.float64(crop_y1) - sy
            ok = np.isfinite(u) & np.isfinite(v) & (u >= 0.0) & (u <= pw - 1.0) & (v >= 0.0) & (v <= ph - 1.0)
            x0 = np.minimum(np.floor(np.where(ok, u, 0.0)), pw - 2.0)
            y0 = np.minimum(np.floor(np.where(ok, v, 0.0)), ph - 2.0)
            fx, fy = u - x0, v - y0
            xi, yi = x0.astype(np.int64), y0.astype(np.int64)
            t64 = tm[b].astype(np.float64)
            t00, t01, t10, t11 = t64[yi, xi], t64[yi, xi + 1], t64[yi + 1, xi], t64[yi + 1, xi + 1]
            t = (1.0 - fy) * ((1.0 - fx) * t00 + fx * t01) + fy * ((1.0 - fx) * t10 + fx * t11)
            ok &= np.isfinite(t00) & np.isfinite(t01) & np.isfinite(t10) & np.isfinite(t11)
            out[b] = np.where(ok, t, np.nan).astype(np.float32)
    return out


def same_bits(a, b):
    """float arrays equal bit for bit, NaN where NaN (every NaN the device and NumPy write is the quiet NaN)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    bits = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(bits), b.view(bits)))


def temperature_map(ph=PH, pw=PW, seed=0):
    """a smooth made-up temperature field with float32 noise, 24 .. 40 C"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:ph, 0:pw].astype(np.float64)
    t = 31.0 + 4.0 * np.sin(xx / 9.0 + 0.3 * seed) * np.cos(yy / 7.0) + 3.0 * np.exp(-((xx - 0.55 * pw) ** 2 + (yy - 0.4 * ph) ** 2) / 150.0)
    return (t + rng.uniform(-0.5, 0.5, t.shape)).astype(np.float32)


def info_row(shift=(0.0, 0.0), warp=(1.0, 0.0, 0.0, 0.0, 1.0, 0.0)):
    """a record as vistaf_align_batch writes it: shift, response, warp, rho, iterations, failed"""
    return np.array([shift[0], shift[1], 0.9, *warp, 0.99, 12.0, 0.0], np.float64)


def rotation_about(theta, cx, cy):
    c, s = math.cos(theta), math.sin(theta)
    return (c, -s, cx - c * cx + s * cy, s, c, cy - s * cx - c * cy)


def register_cases():
    """name -> (temp_map [B,PH,PW], info [B,12] or None, apply_global_shift)"""
    m = temperature_map()
    holes = m.copy()
    for y, x in ((12, 20), (30, 40), (5, 9), (41, 61), (25, 33), (25, 34)):            # inside the crop's footprint, two of them neighbours
        holes[y, x] = np.nan
    holes[18, 50] = np.inf
    bad = np.stack([info_row(warp=(1.0, 0.0, np.nan, 0.0, 1.0, 0.0)), info_row(shift=(np.inf, 0.0)), info_row(warp=(np.inf, 0.0, 0.0, 0.0, 1.0, 0.0)),
                    info_row(shift=(0.0, np.nan))])
    three = np.stack([info_row((1.5, -0.75), rotation_about(-0.05, 26.0, 18.0)), info_row(), info_row((-2.0, 3.0), (1.0, 0.0, 0.3, 0.0, 1.0, -0.6))])
    return {
        "identity_null_info": (m[None], None, True),
        "integer_shift": (m[None], info_row((3.0, -2.0))[None], True),
        "fractional_shift": (m[None], info_row((2.25, -1.4))[None], True),
        "rotation_0.3": (m[None], info_row(warp=rotation_about(0.3, 26.0, 18.0))[None], True),
        "last_row_and_column": (m[None], info_row((-21.0, -19.0))[None], True),            # x = 52 -> u = PW-1, y = 36 -> v = PH-1
        "nan_holes": (holes[None], None, True),
        "non_finite_info": (np.stack([m] * 4), bad, True),
        "shift_not_applied": (m[None], info_row((3.0, -2.0))[None], False),
        "batch_of_3": (np.stack([temperature_map(seed=s) for s in (1, 2, 3)]), three, True),
    }


# ---------------------------------------------------------------------------------------------------------------- the rows
def _plain(a):
    a = np.asarray(a, dtype=np.float64).ravel()
    return float(np.cumsum(a)[-1]) if a.size else 0.0                                  # cumsum adds one element after the other


def _fsum(a):
    return math.fsum(np.asarray(a, dtype=np.float64).ravel().tolist())


def _box(row, h, w, margin):
    """(box mask, grown box mask) of a table row, as the header reads it"""
    (x0, y0, x1, y1), own = SH.table_box(row, h, w)
    grown = SH.table_box(row, h, w, margin)[1] if x1 >= x0 and y1 >= y0 else None     # an inverted box is no box: it does not grow into one
    return SH.box_mask(own, h, w), SH.box_mask(grown, h, w)


def _thermal(temp_crop, depth_mm, contact_index, contacts, count, eps, margin, status, total):
    temp_crop, depth_mm = np.asarray(temp_crop, dtype=np.float32), np.asarray(depth_mm, dtype=np.float32)
    contact_index, contacts = np.asarray(contact_index), np.asarray(contacts, dtype=np.float64)
    B, h, w = contact_index.shape
    K = contacts.shape[1]
    out, frame = np.full((B, K, NTHERMAL), np.nan), np.full((B, NTHERMALFRAME), np.nan)
    for b in range(B):
        if status is not None and int(status[b]) != 0:
            continue
        d32 = np.nan_to_num(depth_mm[b], nan=0.0)
        t32 = temp_crop[b]
        fin, t64, d64 = np.isfinite(t32), t32.astype(np.float64), d32.astype(np.float64)
        deep = d32 > np.float32(eps)
        idx = contact_index[b].astype(np.int64)
        kk = min(max(int(count[b]), 0), K)
        skin = (idx < 0) | (idx >= kk)
        for k in range(kk):
            row, o = contacts[b, k], out[b, k]
            own, grown = _box(row, h, w, margin)
            cm = own & (idx == k) & deep
            vm = cm & fin
            n, nv = int(cm.sum()), int(vm.sum())
            o[T["contact_pixels"]], o[T["valid_pixels"]] = n, nv
            if n:
                o[T["coverage"]] = nv / n
            if nv:
                tv, dv = t64[vm], d64[vm]                                        # row-major order
                mean = total(tv) / nv
                o[T["mean_C"]] = mean
                o[T["weighted_mean_C"]] = total(dv * tv) / total(dv)
                o[T["min_C"]], o[T["max_C"]] = tv.min(), tv.max()
                o[T["std_C"]] = np.sqrt(total((tv - mean) * (tv - mean)) / nv)
            a = row[SH.C_ARGMAX]
            if np.isfinite(a) and 0.0 <= a < h * w and fin.ravel()[int(a)]:
                o[T["peak_temp_C"]] = t64.ravel()[int(a)]
            sm = grown & skin & fin
            ns = int(sm.sum())
            o[T["surround_pixels"]] = ns
            if ns:
                o[T["surround_mean_C"]] = total(t64[sm]) / ns
            o[T["contrast_C"]] = o[T["mean_C"]] - o[T["surround_mean_C"]]
        f = frame[b]
        sk, cn = fin & skin, fin & ~skin & deep
        f[F["registered_pixels"]], f[F["contact_pixels"]] = int(fin.sum()), int(cn.sum())
        if sk.any():
            f[F["skin_mean_C"]] = total(t64[sk]) / int(sk.sum())
        if cn.any():
            f[F["contact_mean_C"]] = total(t64[cn]) / int(cn.sum())
        f[F["contrast_C"]] = f[F["contact_mean_C"]] - f[F["skin_mean_C"]]
        hot = cold = None
        for k in range(kk):
            m = out[b, k, T["mean_C"]]
            if np.isnan(m):
                continue
            if hot is None or m > out[b, hot, T["mean_C"]]:
                hot = k
            if cold is None or m < out[b, cold, T["mean_C"]]:
                cold = k
        if hot is not None:
            f[F["hottest_contact"]], f[F["coldest_contact"]] = hot, cold
    return out, frame


def numpy_thermal(temp_crop, depth_mm, contact_index, contacts, count, eps, margin, status=None):
    """-> (thermal [B,K,16], frame [B,8]) float64, every sum plain float64 in row-major order"""
    return _thermal(temp_crop, depth_mm, contact_index, contacts, count, eps, margin, status, _plain)


def numpy_thermal_fsum(temp_crop, depth_mm, contact_index, contacts, count, eps, margin, status=None):
    return _thermal(temp_crop, depth_mm, contact_index, contacts, count, eps, margin, status, _fsum)


def _equal_where_present(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na], b[~nb]))


def exact_equal(got, want):
    """(thermal, frame) pairs: NaN in the same places of both tables, the counts equal and the selections bit-equal"""
    (a, fa), (b, fb) = got, want
    a, b, fa, fb = np.asarray(a), np.asarray(b), np.asarray(fa), np.asarray(fb)
    if a.shape != b.shape or fa.shape != fb.shape or not np.array_equal(np.isnan(a), np.isnan(b)) or not np.array_equal(np.isnan(fa), np.isnan(fb)):
        return False
    rows = all(_equal_where_present(a[..., T[n]], b[..., T[n]]) for n in COUNTS + SELECTED)
    return bool(rows and all(_equal_where_present(fa[..., F[n]], fb[..., F[n]]) for n in FRAME_EXACT))


def distances(got, want, temp_crop):
    """Largest distance between two (thermal, frame) pairs over the summed fields, relative to the field's scale: the largest |temperature|
    of the frame's registered plane for the temperatures (1 for a frame without a finite pixel), 1 for the coverage.  Returns {"rows", "frame"};
    fields NaN in both do not count."""
    (a, fa), (b, fb) = got, want
    out = {"rows": 0.0, "frame": 0.0}
    for f in range(a.shape[0]):
        t = np.asarray(temp_crop[f], dtype=np.float64)
        scale = float(np.abs(t[np.isfinite(t)]).max()) if np.isfinite(t).any() else 1.0
        for n in SUMMED:
            d = np.abs(a[f, :, T[n]] - b[f, :, T[n]]) / (1.0 if n == "coverage" else scale)
            if (~np.isnan(d)).any():
                out["rows"] = max(out["rows"], float(np.nanmax(d)))
        for n in FRAME_SUMMED:
            d = abs(fa[f, F[n]] - fb[f, F[n]]) / scale
            if not np.isnan(d):
                out["frame"] = max(out["frame"], float(d))
    return out


# ---------------------------------------------------------------------------------------------------------------- scenes
def temperature_crop(h, w, seed=0, warm=()):
    """a made-up registered plane: a smooth skin temperature with float32 noise, `warm` = (mask, degrees) pairs added on top"""
    rng = np.random.default_rng(100 + seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    t = 30.0 + 1.5 * np.sin(xx / 11.0 + seed) + 1.0 * np.cos(yy / 6.0) + rng.uniform(-0.3, 0.3, (h, w))
    for mask, deg in warm:
        t = t + deg * mask
    return t.astype(np.float32)


def pack(scenes, temps, K, margin=8, eps=EPS, count=None, status=None):
    """a case: the arguments of numpy_thermal / ThermalReadout.measure for a list of SH.Scene frames and their registered planes"""
    c = SH.pack(scenes, K, 0.2, 0.5, eps, count)
    return {"temp": np.stack(temps), "depth": c["depth"], "index": c["index"], "tab": c["tab"], "count": c["count"], "eps": eps, "margin": margin, "K": K,
            "status": None if status is None else np.asarray(status, np.int32)}


def args(c):
    return c["temp"], c["depth"], c["index"], c["tab"], c["count"], c["eps"], c["margin"], c["status"]


def cases():
    """every direct case by name"""
    f = SH.frames_37x53()
    h, w = H, W

    def warm(scene, seed=0, deg=4.0):
        return temperature_crop(h, w, seed, [(scene.index == k, deg + 1.5 * k) for k in range(4)])
    c = {}
    c["single_pixel"] = pack([f["single_pixel"]], [warm(f["single_pixel"])], 4)
    c["corners_margin_clipped"] = pack([f["corners"]], [warm(f["corners"], 1)], 4, margin=8)
    c["margin_0"] = pack([f["corners"]], [warm(f["corners"], 1)], 4, margin=0)
    touch = SH.Scene(h, w, 0.0).paint(0, SH.rect(h, w, 10, 8, 19, 20), 0.8).paint(1, SH.rect(h, w, 20, 8, 31, 20), 0.6)
    touch.paint(0, SH.rect(h, w, 12, 10, 17, 18), SH.quadric(h, w, 14.6, 14.2, 1.1, 9.0, 12.0, 0.2, 0.25))
    c["touching"] = pack([touch], [warm(touch, 2)], 4, margin=5)
    two = SH.Scene(h, w, 0.0).paint(0, SH.disc(h, w, 14, 12, 7.5), SH.quadric(h, w, 14.2, 11.9, 1.0, 20.0, 30.0, 0.7, 0.2))
    two.paint(1, SH.disc(h, w, 38, 24, 6.5), SH.quadric(h, w, 38.0, 24.3, 0.8, 15.0, 15.0, 0.0, 0.2))
    t = warm(two, 3)
    t[two.index == 0] = np.nan                                                         # contact 0 has no temperature at all
    c["no_finite_temperature"] = pack([two], [t], 4)
    t = warm(two, 4)
    t[:, :15] = np.nan                                                                 # the photograph ends inside contact 0
    t[24:, 30:] = np.nan                                                               # ... and inside contact 1
    c["half_covered"] = pack([two], [t], 4)
    c["depth_eps_and_nan"] = pack([f["nan_and_eps"]], [warm(f["nan_and_eps"], 5)], 4)
    c["count_0"] = pack([f["stray_rows"]], [warm(f["stray_rows"], 6)], 4, count=[0])
    c["count_above_k"] = pack([f["stray_rows"]], [warm(f["stray_rows"], 6)], 2, count=[5])
    c["stray_index_values"] = pack([f["stray_rows"]], [warm(f["stray_rows"], 6)], 4, count=[2])
    many = SH.cases()["k64"]
    t = temperature_crop(h, w, 7, [(many["index"][0] == k, 0.05 * k) for k in range(64)])
    c["k64"] = {"temp": t[None], "depth": many["depth"], "index": many["index"], "tab": many["tab"], "count": many["count"], "eps": EPS, "margin": 2, "K": 64,
                "status": None}
    c["status_in_the_middle"] = pack([f["corners"], two, f["ring"]], [warm(f["corners"], 8), warm(two, 9), warm(f["ring"], 10)], 4, status=[0, 2, 0])
    strip = SH.Scene(3, 1100).paint(0, SH.rect(3, 1100, 0, 0, 1099, 2), SH.quadric(3, 1100, 560.3, 1.2, 2.0, 4000.0, 3.0, 0.0, 0.1))
    c["strip_3x1100"] = pack([strip], [temperature_crop(3, 1100, 11)], 4)
    big = SH.Scene(150, 150, 0.0).paint(0, SH.rect(150, 150, 9, 12, 138, 141), SH.quadric(150, 150, 71.7, 80.2, 1.8, 700.0, 500.0, 0.6, 0.15))
    t = temperature_crop(150, 150, 12, [(big.index == 0, 6.0)])
    t[:3] = np.nan
    c["big_130x130"] = pack([big], [t], 4)
    five = [f["corners"], f["ring"], two, f["nan_and_eps"], f["stray_rows"]]
    temps = [warm(s, 20 + i) for i, s in enumerate(five)]
    temps[2][:, :15] = np.nan
    c["mixed_batch"] = pack(five, temps, 4, margin=6, count=[4, 1, 2, 1, 0], status=[0, 0, 0, 0, 0])
    return c
