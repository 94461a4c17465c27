"""The point-cloud read-out (include/vistaf_cloud.h) restated in NumPy, the hand-made planes of tests/test_cloud.py and the comparison.

`numpy_cloud` follows the header step by step with float64 arrays: the cleaned float32 depth widened and padded with mode="edge" (the clamped
neighbours), then one NumPy ufunc per operation of the definition, in the definition's parenthesisation -- an element-wise ufunc is one
correctly rounded IEEE operation and never fuses a product with a sum, so the eight float32 fields of a point, the offsets, pixel, label,
counts and MAX_SLOPE_INDEX must equal the device's bit for bit.  The float64 sums of a frame row (rt, nx, ny, nz) are formed by `summer`:
math.fsum (exact) for the reference, and np.sum over the chunks of the pixel list in reversed order for the second restatement
(`numpy_cloud(..., summer=reversed_chunk_sum)`).  The two must agree on every exact field; their distance on a summed field is what the
order of a float64 sum alone costs there, and THE BAR for the device is max(4 x that distance, 64 float64 ulps) of the field's scale
(`bars`): the surface area against itself, the mean normal against 1 (it is a unit vector), TILT_DEG and MAX_SLOPE_DEG, which go through
atan2 / atan, against degrees(1).

THE CAP (`cap_errors`): a spherical cap R = 8 mm, 0.6 mm deep, float32 depth, at 37 x 53 and 40 x 52 and s = 0.1 and 0.0625 mm per pixel,
the ball's centre 0.3 / -0.2 pixels off the crop centre, over the points whose 3 x 3 neighbourhood is all positive (1770 .. 1900 of them).
Measured with this restatement (the largest of the four cases): normals within 2.8e-5 of (-X, -Y, sqrt(R^2 - r^2)) / R (absolute, of a
unit vector; at s = 0.1), Hc within 2.1e-4 of -1/R relative to 1/R, Kc within 4.2e-4 of 1/R^2 relative to 1/R^2 (both at s = 0.0625) --
discretisation (central differences on a sphere: (s/R)^2-sized terms) plus the float32 depth (an ulp of 0.6 mm over s^2 in the second
differences, which is why the finer grid has the larger curvature error).  The test's bar is four times these: CAP_BARS.
"""
import math

import numpy as np

ULP = 2.0 ** -52
POINT_NAMES = ["x", "y", "z", "nx", "ny", "nz", "curvature", "gaussian_curvature"]
FRAME_NAMES = ["surface_pixels", "points", "points_written", "projected_area_mm2", "surface_area_mm2", "mean_normal_x", "mean_normal_y",
               "mean_normal_z", "tilt_deg", "max_slope_deg", "max_slope_index"]
F_ = {n: i for i, n in enumerate(FRAME_NAMES)}
NPOINT, NFRAME = 8, 12
EXACT = ["surface_pixels", "points", "points_written", "projected_area_mm2", "max_slope_index"]
SUMMED = ["surface_area_mm2", "mean_normal_x", "mean_normal_y", "mean_normal_z", "tilt_deg", "max_slope_deg"]
CAP_R, CAP_D0 = 8.0, 0.6
CAP_MEASURED = {"normal": 2.8e-5, "mean": 2.1e-4, "gauss": 4.2e-4}
CAP_BARS = {k: 4.0 * v for k, v in CAP_MEASURED.items()}
EPS = 0.01


def fsum(v):
    return math.fsum(np.asarray(v, np.float64).tolist())


def reversed_chunk_sum(v, chunk=97):
    v = np.asarray(v, np.float64)
    total = np.float64(0.0)
    for lo in reversed(range(0, len(v), chunk)):
        total = total + np.sum(v[lo:lo + chunk])
    return float(total)


def numpy_cloud(depth, mm_per_px, depth_eps_mm, status=None, contact_index=None, stride=1, origin=None, summer=fsum):
    """depth [B,h,w] f32, mm_per_px [B], status [B] or None, contact_index [B,h,w] i8 or None.  Returns a dict: points [N,8] f32, pixel [N]
    i32, label [N] i8 (or None), offsets [B+1] i64, frame [B,12] f64 -- ALL points of the batch, as with a max_points that holds them; what a
    smaller max_points changes (the device's arrays are the first max_points entries, POINTS_WRITTEN) is `capped`."""
    depth = np.asarray(depth, np.float32)
    B, h, w = depth.shape
    eps = np.float32(depth_eps_mm)
    ox, oy = ((w - 1) / 2.0, (h - 1) / 2.0) if origin is None else (float(origin[0]), float(origin[1]))
    yy, xx = np.mgrid[0:h, 0:w]
    lattice = (xx % stride == 0) & (yy % stride == 0)
    offsets = np.zeros(B + 1, np.int64)
    frame = np.full((B, NFRAME), np.nan, np.float64)
    pts, pix, lab = [], [], []
    one, two, four = np.float64(1.0), np.float64(2.0), np.float64(4.0)
    for b in range(B):
        offsets[b + 1] = offsets[b]
        if status is not None and int(status[b]) != 0:
            continue
        x32 = depth[b]
        d32 = np.where(np.isfinite(x32), x32, np.float32(0.0)).astype(np.float32)
        surf = d32 > eps
        s = np.float64(mm_per_px[b])
        D = np.pad(d32.astype(np.float64), 1, mode="edge")
        c, l, r, u, dn = D[1:-1, 1:-1], D[1:-1, :-2], D[1:-1, 2:], D[:-2, 1:-1], D[2:, 1:-1]
        ul, ur, bl, br = D[:-2, :-2], D[:-2, 2:], D[2:, :-2], D[2:, 2:]
        with np.errstate(all="ignore"):
            s2, ss = two * s, s * s
            dx, dy = (r - l) / s2, (dn - u) / s2
            dxx, dyy = ((r - c) - (c - l)) / ss, ((dn - c) - (c - u)) / ss
            dxy = ((br - bl) - (ur - ul)) / (four * ss)
            ax, ay = one + dx * dx, one + dy * dy
            g = ax + dy * dy
            rt = np.sqrt(g)
            nx, ny, nz = dx / rt, dy / rt, one / rt
            Hc = ((ay * dxx - (two * (dx * dy)) * dxy) + ax * dyy) / (two * (g * rt))
            Kc = (dxx * dyy - dxy * dxy) / (g * g)
            q = dx * dx + dy * dy
            X, Y, Z = (xx.astype(np.float64) - ox) * s, (yy.astype(np.float64) - oy) * s, -c
        rec = np.stack([X, Y, Z, nx, ny, nz, Hc, Kc], axis=-1).astype(np.float32)
        sel = np.flatnonzero((surf & lattice).ravel())
        pts.append(rec.reshape(-1, NPOINT)[sel])
        pix.append(sel.astype(np.int32))
        if contact_index is not None:
            lab.append(np.asarray(contact_index[b], np.int8).ravel()[sel])
        offsets[b + 1] = offsets[b] + len(sel)
        f = frame[b]
        idx = np.flatnonzero(surf.ravel())
        n = len(idx)
        f[F_["surface_pixels"]], f[F_["points"]] = n, len(sel)
        f[F_["points_written"]] = len(sel)
        f[F_["projected_area_mm2"]] = np.float64(n) * ss if n else 0.0
        f[F_["surface_area_mm2"]] = np.float64(summer(rt.ravel()[idx])) * ss if n else 0.0
        if n:
            sx, sy, sz = (np.float64(summer(v.ravel()[idx])) for v in (nx, ny, nz))
            length = np.sqrt((sx * sx + sy * sy) + sz * sz)
            mx, my, mz = sx / length, sy / length, sz / length
            f[5:8] = mx, my, mz
            f[F_["tilt_deg"]] = np.arctan2(np.hypot(mx, my), mz) * (180.0 / math.pi)
            qs = q.ravel()[idx]
            k = int(np.argmax(qs))                                                         # the first occurrence of the maximum
            f[F_["max_slope_deg"]] = np.arctan(np.sqrt(qs[k])) * (180.0 / math.pi)
            f[F_["max_slope_index"]] = idx[k]
    return dict(points=np.concatenate(pts) if pts else np.zeros((0, NPOINT), np.float32),
                pixel=np.concatenate(pix) if pix else np.zeros(0, np.int32),
                label=(np.concatenate(lab) if lab else np.zeros(0, np.int8)) if contact_index is not None else None,
                offsets=offsets, frame=frame)


def capped(ref, max_points):
    """the frame rows of numpy_cloud's result under a capacity: POINTS_WRITTEN counts the points of the frame numbered below max_points"""
    frame, off = ref["frame"].copy(), np.minimum(ref["offsets"], int(max_points))
    frame[:, F_["points_written"]] = np.where(np.isnan(frame[:, 0]), np.nan, off[1:] - off[:-1])
    return frame


# ---------------------------------------------------------------------------------------------------------------- comparison
def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def exact_frame_equal(got, want):
    """the NaN pattern of every field and the value of every field without a sum or an arc tangent behind it"""
    return got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)) and \
        all(np.array_equal(got[:, F_[k]], want[:, F_[k]], equal_nan=True) for k in EXACT)


def distances(a, b):
    """largest |a - b| of every summed field over the frames, relative to the field's scale (taken from b)"""
    out = {k: 0.0 for k in SUMMED}
    for ra, rb in zip(a, b):
        if np.isnan(rb[F_["mean_normal_x"]]):
            continue
        for k in SUMMED:
            scale = rb[F_[k]] if k == "surface_area_mm2" else (math.degrees(1.0) if k.endswith("_deg") else 1.0)
            out[k] = max(out[k], abs(ra[F_[k]] - rb[F_[k]]) / scale)
    return out


def bars(want, other):
    return {k: max(4.0 * e, 64.0 * ULP) for k, e in distances(other, want).items()}


# ---------------------------------------------------------------------------------------------------------------- planes
def bump(h, w, cx, cy, sigma, amp):
    yy, xx = np.mgrid[0:h, 0:w]
    return (amp * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2.0 * sigma * sigma))).astype(np.float32)


def cap_plane(h, w, s, cx, cy):
    """a ball of radius CAP_R pressed CAP_D0 deep at pixel (cx, cy): float32 depth, 0 outside the cap"""
    yy, xx = np.mgrid[0:h, 0:w]
    r2 = ((xx - cx) * s) ** 2 + ((yy - cy) * s) ** 2
    d = np.sqrt(np.maximum(CAP_R * CAP_R - r2, 0.0)) - (CAP_R - CAP_D0)
    return np.maximum(d, 0.0).astype(np.float32)


def cap_errors(h, w, s):
    """errors of numpy_cloud on the cap against analysis, over the points whose 3 x 3 neighbourhood is all positive; and their number"""
    cx, cy = (w - 1) / 2.0 + 0.3, (h - 1) / 2.0 - 0.2
    d = cap_plane(h, w, s, cx, cy)
    out = numpy_cloud(d[None], [s], 0.0, origin=(cx, cy))
    pos = np.pad(d > 0, 1, mode="constant")
    inner = np.ones_like(d, bool)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            inner &= pos[dy:dy + h, dx:dx + w]
    keep = inner.ravel()[out["pixel"]]
    p = out["points"][keep].astype(np.float64)
    r2 = p[:, 0] ** 2 + p[:, 1] ** 2
    normal = np.stack([-p[:, 0], -p[:, 1], np.sqrt(CAP_R * CAP_R - r2)], axis=1) / CAP_R
    return {"normal": float(np.abs(p[:, 3:6] - normal).max()), "mean": float(np.abs(p[:, 6] + 1.0 / CAP_R).max() * CAP_R),
            "gauss": float(np.abs(p[:, 7] - 1.0 / CAP_R ** 2).max() * CAP_R ** 2)}, int(keep.sum()), len(out["pixel"])


def hard_batch(h, w, seed=0):
    """Nine frames in which every case of the definition occurs (asserted on the reference by the test): 0 empty; 1 one bump; 2 bumps cut
    by all four borders and one in a corner; 3 a plateau whose four corners tie the largest slope; 4 pixels exactly at eps and one float32
    step above; 5 a noisy floor with negative, NaN and +-inf pixels under a bump; 6 status != 0 and full of garbage; 7 a bump again;
    8 two bumps in one contact.  A random int8 label plane goes with it."""
    rng = np.random.default_rng(seed)
    B = 9
    d = np.zeros((B, h, w), np.float32)
    d[1] = bump(h, w, 0.45 * w, 0.55 * h, 4.0, 0.8)
    for cx, cy in ((0.5 * w, -1.0), (0.5 * w, h + 0.5), (-1.5, 0.5 * h), (w - 0.2, 0.45 * h), (w - 1.0, h - 1.0)):
        d[2] = np.maximum(d[2], bump(h, w, cx, cy, 3.0, 0.6))
    d[3, 9:20, 12:31] = 1.0
    e = np.float32(EPS)
    d[4, 5, 3:9] = e
    d[4, 7, 3:9] = np.nextafter(e, np.float32(1.0))
    d[4, 9, 3:9] = np.nextafter(e, np.float32(0.0))
    d[5] = (rng.random((h, w)) * 0.014 - 0.005).astype(np.float32) + bump(h, w, 0.6 * w, 0.4 * h, 3.5, 0.5)
    bad = rng.choice(h * w, 60, replace=False)
    d[5].ravel()[bad[:20]] = np.nan
    d[5].ravel()[bad[20:40]] = np.inf
    d[5].ravel()[bad[40:]] = -np.inf
    d[6] = np.float32(1e30)
    d[6, ::2] = np.nan
    d[7] = bump(h, w, 0.3 * w, 0.3 * h, 5.0, 1.1)
    d[8] = bump(h, w, 0.4 * w, 0.5 * h, 3.0, 0.7) + bump(h, w, 0.4 * w + 7, 0.5 * h + 2, 2.5, 0.5)
    status = np.array([0, 0, 0, 0, 0, 0, 3, 0, 0], np.int32)
    mpp = np.array([0.05, 0.05, 0.0625, 0.1, 0.047, 0.05, 0.05, 0.0531, 0.05])
    index = rng.integers(-1, 4, size=(B, h, w)).astype(np.int8)
    return dict(depth=d, mpp=mpp, status=status, index=index, eps=EPS, shape=(h, w))


def sparse_batch(h, w, B, seed=1):
    """B frames, all accepted, two points in a hundred pixels, and a point in the first and the last pixel of the first and the last frame"""
    rng = np.random.default_rng(seed)
    d = np.where(rng.random((B, h, w)) < 0.02, rng.random((B, h, w)) * 0.9 + 0.1, 0.0).astype(np.float32)
    d[1] = 0.0                                                                              # an empty frame inside
    for b in (0, B - 1):
        d[b, 0, 0], d[b, -1, -1] = 0.75, 0.5
    return dict(depth=d, mpp=np.full(B, 0.05) + 0.001 * np.arange(B), status=None, index=None, eps=EPS, shape=(h, w))
