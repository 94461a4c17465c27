"""Hand-made planes and plain NumPy references for the back end of a predict -- everything post_demod runs after the core medians (k_post.hip,
k_holes.hip, the fused kernels of k_blurchain.hip and k_backend.hip, the three force tails).  No GPU here: tests/test_post_direct.py feeds
these planes to the production launchers through csrc/test_hooks_post.h and compares.

Every reference is built on the oracle's own stage functions (oracle/ftp_oracle.py) in the order of process_frame; where a launcher takes as an
argument what the oracle computes for itself (the distance planes, the blurred ROI, the medians) the case computes it the oracle's way and the
CPU tests of test_post_direct.py pin the restatement to the oracle's function.  Values are dyadic (k / 64, k / 256, float32 neighbours of
such) wherever a sum is compared, so the float32 pairwise sums of NumPy and the float64 sums of the kernels are both exact."""
import math

import numpy as np

import mask_cases as M
from oracle import cvlite
from oracle import ftp_oracle as O

QNAN32 = 0x7fc00000
QNAN64 = 0x7ff8000000000000
HUGE_DIST = np.frombuffer(b"\x7f\x7f\x7f\x7f", np.float32)[0]      # what a session's memset(0x7f) leaves in the distance plane without a band


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def ulp32(r):
    """spacing of float32 at the float64 value(s) r"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.spacing(np.abs(np.asarray(r, np.float64)).astype(np.float32)).astype(np.float64)


def within_depth_rule(got, r):
    """The bound for values formed through the device's float64 exp (and a possible fma) against NumPy's: got == float32(r), or
    |got - r| <= 1/2 ulp32(r) (1 + 2^-20), i.e. either neighbour when r lies within a few float64 ulps of a float32 rounding tie.
    Elementwise; NaN positions are the caller's to compare."""
    got = np.asarray(got, np.float64)
    r = np.asarray(r, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        same = got == r.astype(np.float32).astype(np.float64)
        near = np.abs(got - r) <= 0.5 * ulp32(r) * (1.0 + 2.0 ** -20)
    return same | near


# =======================================================================================================================================
# calibration curves (Curve of common.hpp: type 0..5 with a, b, c)

CURVE_NAMES = ("linear0", "linear", "poly2", "sat_exp", "growth", "hinge_saturating")
# (type, a, b, c): every type, with signs and sizes that keep exp() in range
CURVES = [(0, 1.75, 0.0, 0.0), (1, 0.8125, 0.03125, 0.0), (2, 0.21, 0.9, -0.015625), (3, 2.3, 0.71, 0.0), (4, 0.37, 0.93, 0.0), (5, 3.1, 0.83, 0.4375)]


def curve_model(t, a, b, c):
    """the oracle's model dict of curve (t, a, b, c)"""
    params = {0: {"a": a}, 1: {"a": a, "b": b}, 2: {"c2": a, "c1": b, "c0": c}, 3: {"a": a, "b": b}, 4: {"a": a, "b": b}, 5: {"a": a, "b": b, "c": c}}[t]
    return {"type": CURVE_NAMES[t], "params": params}


def ref_curve(t, a, b, c, v):
    """predict_force_from_volume's expressions, vectorised, float64"""
    v = np.asarray(v, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        if t == 0:
            return a * v
        if t == 1:
            return a * v + b
        if t == 2:
            return a * v * v + b * v + c
        if t == 3:
            return a * (1.0 - np.exp(-b * np.maximum(v, 0.0)))
        if t == 4:
            return a * (np.exp(b * np.maximum(v, 0.0)) - 1.0)
        return a * ((1.0 - np.exp(-b * np.maximum(v - c, 0.0))) - (1.0 - np.exp(-b * np.maximum(0.0 - c, 0.0))))


def ref_to_mm(unitless, curve, use_neg):
    """height_unitless_to_depth_mm before its cast to float32: the float64 depth of every pixel (NaN stays NaN)"""
    h = np.asarray(unitless, np.float32)
    x = ((-h) if use_neg else h).astype(np.float64)
    return ref_curve(*curve, np.maximum(x, 0.0))


TO_MM_P = 3001


def to_mm_case(use_neg):
    """(unitless [3, P], roi [P]) for launch_to_mm alone.  Frame 0: the largest argument of the curve, NaN and both infinities sit off the ROI (NaN and
    one infinity on it too); frame 1: every ROI pixel has argument 0 and only pixels off the ROI would be candidates; frame 2: a plain frame."""
    P = TO_MM_P
    rng = np.random.default_rng(41 + use_neg)
    roi = (rng.random(P) < 0.7).astype(np.uint8)
    off, on = np.flatnonzero(roi == 0), np.flatnonzero(roi)
    u = _dyadic(rng, 3 * P, -192, 192).reshape(3, P)         # arguments up to 3 on either side
    deep = np.float32(-50.0 if use_neg else 50.0)           # the curve's argument 50: beyond every ROI pixel's
    u[0, off[:3]] = deep
    u[0, off[3:9]] = np.array(_SPECIAL * 2, np.float32)
    # on the ROI: NaN and the infinity whose argument clamps to 0 (the other one would be the frame's maximum under a saturating curve)
    u[0, on[:6]] = np.array([np.nan, np.inf if use_neg else -np.inf] * 3, np.float32)
    u[0, on[6]] = np.float32(-0.0)
    u[1, on] = np.abs(u[1, on]) * np.float32(1 if use_neg else -1)
    u[1, off[:3]] = deep
    return u, roi


# =======================================================================================================================================
# the force tail and the arg-extrema

TAIL_EPS = 1.0 / 64.0                   # depth_eps_mm of the tail cases: a dyadic float32
TAIL_MM_PER_PX = 0.25                   # area per pixel 1 / 16: products with it are exact in float32 too
TAIL_PERIOD = 7.75
TAIL_FORCE = CURVES[5]
TAIL_P = [1, 1023, 1024, 1025, 4095, 4096, 4097, 256 * 4096 + 1]      # the 4 x 1024 and 16 x 256 strides; 257 blocks: k_tail_final loops twice
# where a tie's two pixels sit: neighbouring threads, either side of a wave, of k_tail's 1024-thread stride, of k_tail_part's 4096-pixel block,
# and far apart
TIE_PAIRS = [(0, 1), (62, 65), (1020, 1027), (4090, 4100)]


def tie_pairs(P):
    out = [(i, j) for i, j in TIE_PAIRS if j < P]
    if P >= 8:
        out.append((3, P - 1))
    return out


def tail_roi_static(P):
    rng = np.random.default_rng(77 + P)
    roi = (rng.random(P) < 0.8).astype(np.uint8)
    for i, j in tie_pairs(P):
        roi[i] = roi[j] = 1
    if P == 1:
        roi[0] = 1
    return roi


def _dyadic(rng, n, lo, hi, q=64.0):
    return (rng.integers(lo, hi + 1, n).astype(np.float64) / q).astype(np.float32)


def tail_kinds(P):
    """the frames of the tail catalogue at P pixels, by name"""
    kinds = ["pos", "neg", "tie", "below_eps", "no_finite_roi", "specials", "specials_neg"]
    pairs = tie_pairs(P)
    if P > 65536:           # the large plane: the frames that can go wrong across blocks, the last pairs only
        return ["pos", "specials_neg", "tie"] + ["%s%d" % (k, n) for n in (len(pairs) - 2, len(pairs) - 1) for k in ("zeromax", "zerorev", "valtie")]
    return kinds + ["%s%d" % (k, n) for n in range(len(pairs)) for k in ("zeromax", "zerorev", "valtie")]


_SPECIAL = [np.nan, np.inf, -np.inf]


def tail_frame(kind, P):
    """(height, roi_frame, unitless) of one frame, float32 / uint8 / float32 [P]; roi_static is tail_roi_static(P)"""
    rng = np.random.default_rng([P, sum(kind.encode())])
    roi_static = tail_roi_static(P)
    eps = np.float32(TAIL_EPS)
    mag = _dyadic(rng, P, 2, 256)                           # 1/32 .. 4: all above eps
    h = mag.copy()
    minority = rng.random(P) < 0.25                         # the other sign: a quarter of the pixels at a quarter of the size
    h[minority] = -mag[minority] / np.float32(4)
    u = -_dyadic(rng, P, 0, 200)                            # unitless heights are <= 0
    roi_frame = (rng.random(P) < 0.85).astype(np.uint8)
    base = kind.rstrip("0123456789")
    if base in ("neg", "specials_neg"):
        h = -h
    if base == "tie":                                       # h next to -h: the two sums are equal, the positive side is kept
        n = P // 2
        h[:] = 0
        h[0:2 * n:2] = mag[:n]
        h[1:2 * n:2] = -mag[:n]
    if base == "below_eps":                                 # |h| <= eps everywhere: k / 256, |k| <= 4
        h = _dyadic(rng, P, -4, 4, 256.0)
        h[::7] = np.float32(-0.0)
    if base in ("specials", "specials_neg"):                # non-finite values inside and outside both ROIs (an infinity of the frame's own sign:
        # one of each would make both sums infinite); depths at eps and one ulp above
        idx = rng.permutation(P)[:min(P, 48)]
        sign = np.float32(-1 if base == "specials_neg" else 1)
        vals = [np.nan, sign * np.inf, np.nan] + [sign * eps, sign * np.nextafter(eps, np.float32(1)), -sign * eps, -sign * np.nextafter(eps, np.float32(1))]
        roi_frame[idx[:2]] = 0                              # a NaN and an infinity outside the frame's own ROI, the next ones inside
        roi_frame[idx[7:9]] = 1
        for n, i in enumerate(idx):
            h[i] = vals[n % len(vals)]
            u[idx[(n + 5) % len(idx)]] = _SPECIAL[n % 3]
    if base == "no_finite_roi":
        on = np.flatnonzero(roi_static)
        h[on] = np.array(_SPECIAL, np.float32)[np.arange(len(on)) % 3]
        u[on] = np.array(_SPECIAL, np.float32)[(np.arange(len(on)) + 1) % 3]
    if base in ("zeromax", "zerorev", "valtie") and tie_pairs(P):
        i, j = tie_pairs(P)[int(kind[len(base):])]
        if base == "valtie":                                # the same non-zero extremum twice
            h[i] = h[j] = np.float32(5.0)
            u[i] = u[j] = np.float32(-4.0)
        else:                                               # the extremum is zero, once with each sign
            h = -np.abs(h) - eps
            u = np.abs(u) + eps
            first, later = (np.float32(-0.0), np.float32(0.0)) if base == "zeromax" else (np.float32(0.0), np.float32(-0.0))
            h[i], h[j] = first, later                       # zeromax: the later zero has the larger bits ...
            u[i], u[j] = later, first                       # ... and the later zero of the minimum the smaller ones
    return h, roi_frame, u


def ref_tail(height, roi_frame, unitless, roi_static, mm_per_px=TAIL_MM_PER_PX, eps=TAIL_EPS):
    """depth_map_to_volume_cm3 restated with exact sums, argmax_depth_mm and compute_min_height, for one frame [P].  roi_frame None: isfinite.
    The volume is left as its parts: `vol32` the correctly rounded float32 of the exact sum of the float32 depths, `area_px`."""
    z = np.asarray(height, np.float32).ravel()
    with np.errstate(invalid="ignore"):
        pos, neg = np.clip(z, 0.0, np.inf), np.clip(-z, 0.0, np.inf)
    sp = math.fsum(pos[~np.isnan(pos)].astype(np.float64))
    sn = math.fsum(neg[~np.isnan(neg)].astype(np.float64))
    use_neg = bool(np.float32(sn) > np.float32(sp))
    depth = (neg if use_neg else pos).copy()
    roi = np.isfinite(z) if roi_frame is None else np.asarray(roi_frame).ravel() != 0
    depth[~roi] = 0.0
    depth = np.where(np.isfinite(depth), depth, np.float32(0)).astype(np.float32)
    contact = depth > np.float32(eps)
    n = int(contact.sum())
    area_px = float(mm_per_px) * float(mm_per_px)
    out = dict(use_neg=use_neg, count=n, area_px=area_px, area=n * area_px, maxd=float(depth[contact].max()) if n else 0.0,
               vol_exact=math.fsum(depth[contact].astype(np.float64)), sums=(sp, sn), arg=-1, minval=float("nan"), minidx=-1)
    out["vol32"] = np.float32(out["vol_exact"])
    if roi_static is not None:
        rs = np.asarray(roi_static).reshape(1, -1) != 0
        out["arg"] = O.argmax_depth_mm(z.reshape(1, -1), rs)
        if unitless is not None:
            val, xy = O.compute_min_height(np.asarray(unitless, np.float32).reshape(1, -1), rs)
            if xy is not None:
                out["minval"], out["minidx"] = val, xy[0]
    return out


def volume_cm3(vol32, area_px):
    """the kernels' expression for S[0] from the float32 sum"""
    return float(np.float32(vol32)) * area_px / 1000.0


# =======================================================================================================================================
# sign flip

CORE_MEDIANS = np.array([np.nan, -0.0, 0.0, 1e-45, -1.5, 2.0, np.nextafter(np.float32(0), np.float32(-1))], np.float32)      # 1e-45: the smallest subnormal


def core_flip_planes(P=1500):
    rng = np.random.default_rng(5)
    hm = _dyadic(rng, len(CORE_MEDIANS) * P, -300, 300).reshape(len(CORE_MEDIANS), P)
    hm[:, 3::11] = np.nan
    hm[:, 4::13] = np.inf
    hm[:, 5::17] = -np.inf
    hm[:, 6::19] = np.float32(-0.0)
    hm[:, 7::23] = np.float32(0.0)
    return hm


def ref_core_flip(hmap, med):
    """process_frame :785-788 for one frame"""
    out = np.array(hmap, np.float32)
    flipped = False
    if float(med) > 0:
        out *= -1.0
        flipped = True
    return out, flipped


# =======================================================================================================================================
# frames for the smoothing, the composition and the hole stage

def disk(h, w, frac, cy=None, cx=None):
    yy, xx = np.mgrid[0:h, 0:w]
    cy = (h - 1) / 2.0 if cy is None else cy
    cx = (w - 1) / 2.0 if cx is None else cx
    return (yy - cy) ** 2 + (xx - cx) ** 2 <= (frac * min(h, w)) ** 2


def frame_roi(h, w):
    return disk(h, w, 0.46)


RELIABLE_KINDS = ("blob", "empty", "full", "ring", "border", "speckle")


def reliable_mask(kind, h, w, seed=0):
    """bool [h, w]; `border` also leaves the ROI"""
    roi = frame_roi(h, w)
    if kind == "empty":
        return np.zeros((h, w), bool)
    if kind == "full":
        return roi.copy()
    if kind == "blob":
        return disk(h, w, 0.3, (h - 1) / 2.0 - 0.07 * h, (w - 1) / 2.0 + 0.05 * w) & roi
    if kind == "ring":                                      # one pixel wide
        d = disk(h, w, 0.33)
        inner = np.zeros_like(d)
        inner[1:-1, 1:-1] = d[1:-1, 1:-1] & d[:-2, 1:-1] & d[2:, 1:-1] & d[1:-1, :-2] & d[1:-1, 2:]
        return d & ~inner
    if kind == "border":                                    # the left half of the frame: along the ROI's border and beyond it
        m = np.zeros((h, w), bool)
        m[:, : w // 2] = True
        return m
    rng = np.random.default_rng(seed + 11 * h + w)
    return (rng.random((h, w)) < 0.6) & roi


def height_plane(rel, seed):
    """heights on rel: dyadic, mostly negative, some positive (to clamp), some -0.0; off it what must not leak: NaN, +-inf, huge values"""
    rng = np.random.default_rng(seed)
    h, w = rel.shape
    hm = _dyadic(rng, h * w, -128, 32).reshape(h, w)
    hm[(rng.random((h, w)) < 0.03) & rel] = np.float32(-0.0)
    junk = np.array([np.nan, np.inf, -np.inf, 1e30, -7.5, -1e30], np.float32)
    off = np.flatnonzero(~rel.ravel())
    hm.ravel()[off] = junk[np.arange(len(off)) % len(junk)]
    return hm


def dist_planes(rel_roi, use_band):
    """(dist_in, dist_out) as apply_frontier_zero_transition forms them, or the session's plane of huge distances without a band"""
    if not use_band:
        huge = np.full(rel_roi.shape, HUGE_DIST, np.float32)
        return huge, huge.copy()
    return (cvlite.dist_l2_3x3(rel_roi.astype(np.uint8) * 255).astype(np.float32),
            cvlite.dist_l2_3x3((~rel_roi).astype(np.uint8) * 255).astype(np.float32))


def roi_den_plane(roi, sigma):
    """masked_gaussian_smooth's denominator for the mask roi"""
    if not sigma > 0:
        return np.ones(roi.shape, np.float32)
    return (cvlite.gaussian_blur(roi.astype(np.float32), sigma) + 1e-6).astype(np.float32)


def ref_masked_smooth(z, mask, sigma, den):
    """masked_gaussian_smooth with the denominator plane handed in (the kernels take the ROI's as an argument)"""
    z0 = z.copy().astype(np.float32)
    z0[~mask] = 0.0
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        return (cvlite.gaussian_blur(z0, sigma) / den).astype(np.float32)


def ref_height_finish(hmap, orel, roi, band, use_band, sigma, roi_den, curve, use_neg):
    """process_frame :804-824 for one frame -> (unitless float32, depth float64 before its cast)"""
    rel = (np.asarray(orel) != 0) & roi
    height_rel = np.full(roi.shape, np.nan, np.float32)
    height_rel[rel] = hmap[rel]
    if use_band:
        height_rel = O.apply_frontier_zero_transition(height_rel, roi, rel, band, apply_inside=True, apply_outside=False)
    hf = np.full(roi.shape, np.nan, np.float32)
    hf[roi] = 0.0
    hf[rel] = height_rel[rel]
    if sigma > 0:
        smooth_all = ref_masked_smooth(hf, roi, sigma, roi_den)
        upd = roi & ~rel
        hf[upd] = smooth_all[upd]
    if use_band:
        hf = O.apply_frontier_zero_transition(hf, roi, rel, band, apply_inside=False, apply_outside=True)
    hf = O.clamp_positive_to_zero(hf, roi)
    return hf, ref_to_mm(hf, curve, use_neg)


# sigma -> taps: 3, 7, 15 (the tile kernels), 17 (streaming only), none
SIGMAS = {0.25: 3, 0.75: 7, 1.75: 15, 2.0: 17, 0.0: 0}
FINISH_SHAPES = [(4, 5), (8, 8), (17, 31), (64, 64), (151, 203)]       # 4 x 5 and 8 x 8: the reflection folds more than once under 15 taps
# (sigma, use_band, band, curve, use_neg, what else)
FINISH_CONFIGS = [(0.25, 1, 3.0, 0, 1, ""), (0.75, 0, 0.0, 1, 0, "den_min"), (1.75, 1, 6.0, 2, 1, ""), (2.0, 1, 2.5, 3, 0, ""), (0.0, 0, 0.0, 4, 1, "specials"),
                  (0.0, 1, 2.0, 5, 1, ""), (1.75, 0, 0.0, 4, 0, ""), (0.75, 1, 1.0, 5, 0, ""), (0.25, 0, 0.0, 3, 1, "positive"), (2.0, 0, 0.0, 2, 0, ""),
                  (0.0, 0, 0.0, 0, 0, "specials"), (0.75, 1, 4.0, 1, 1, "")]


def finish_case(h, w, cfg_index, group):
    """One launch of the composition: B = 3 frames with different reliable masks (group 0 / 1: the first / last three kinds).  Returns a dict of
    the planes ([3, h, w] or [h, w]) and the per-frame references."""
    sigma, use_band, band, curve_i, use_neg, extra = FINISH_CONFIGS[cfg_index]
    roi = frame_roi(h, w)
    kinds = RELIABLE_KINDS[3 * group:3 * group + 3]
    roi_den = roi_den_plane(roi, sigma)
    if extra == "den_min":                                  # the denominator at its floor, 0 + 1e-6
        roi_den = roi_den.copy()
        roi_den[::3, 1::2] = np.float32(1e-6)
    planes = dict(hmap=[], reliable=[], dist_in=[], dist_out=[], unitless=[], depth64=[])
    for n, kind in enumerate(kinds):
        orel = reliable_mask(kind, h, w, cfg_index)
        hm = height_plane(orel & roi, 1000 * cfg_index + 10 * group + n)
        if extra == "specials":                             # values only the mm curve meets: no blur, no taper in this configuration
            on = np.flatnonzero((orel & roi).ravel())
            for k, v in enumerate((np.nan, np.inf, -np.inf, -0.0, 0.0)):
                if len(on) >= 5:
                    hm.ravel()[on[k * len(on) // 5]] = np.float32(v)
        if extra == "positive":                             # nothing below zero: every pixel clamps to 0, no candidate, gmax stays 0
            hm = np.where(orel & roi, np.abs(hm), hm).astype(np.float32)
        di, do = dist_planes(orel & roi, use_band)
        ul, d64 = ref_height_finish(hm, orel, roi, band, use_band, sigma, roi_den, CURVES[curve_i], use_neg)
        for key, v in zip(("hmap", "reliable", "dist_in", "dist_out", "unitless", "depth64"), (hm, orel.astype(np.uint8), di, do, ul, d64)):
            planes[key].append(v)
    out = {k: np.stack(v) for k, v in planes.items()}
    out.update(roi=roi.astype(np.uint8), roi_den=roi_den, sigma=sigma, use_band=use_band, band=band, curve=CURVES[curve_i], use_neg=use_neg, kinds=kinds,
               extra=extra, taps=SIGMAS[sigma])
    return out


# ---- the reliable-only smoothing

SMOOTH_GROUPS = (("speckle", "border", "blob"), ("empty", "full", "ring"))


def smooth_case(h, w, sigma, group=0):
    """B = 3 frames of (detr, bg_med, reliable) and the reference hmap; group 1: an all-zero reliable plane, the whole ROI, a one-pixel ring"""
    rng = np.random.default_rng([h, w, int(sigma * 100), group])
    detr, rels, want = [], [], []
    # group 0 ends on a NaN median: no pixel is finite after the subtraction
    bg = np.array([0.5, -0.265625, np.nan], np.float32) if group == 0 else np.array([-1.0, 0.0, 0.28125], np.float32)
    for n, kind in enumerate(SMOOTH_GROUPS[group]):
        rel = reliable_mask(kind, h, w, n)
        d = height_plane(rel, 31 * h + w + n)
        d[(rng.random((h, w)) < 0.05) & rel] = np.nan       # reliable pixels the unwrap never reached
        zeroed = d - float(bg[n])
        if sigma > 0:
            ref = O.masked_gaussian_smooth(zeroed, rel & np.isfinite(zeroed), sigma)
        else:
            ref = np.where(rel, zeroed, np.float32(np.nan)).astype(np.float32)
        detr.append(d); rels.append(rel.astype(np.uint8)); want.append(ref)
    if group == 1 and h * w >= 64:                          # literally all zeros and all ones: no pixel of the frame, every pixel of it
        assert not rels[0].any()
        rels[1][:] = 1
        rel = rels[1] != 0
        zeroed = detr[1] - float(bg[1])
        want[1] = O.masked_gaussian_smooth(zeroed, rel & np.isfinite(zeroed), sigma) if sigma > 0 else zeroed.astype(np.float32)
    return dict(detr=np.stack(detr), bg_med=bg, reliable=np.stack(rels), hmap=np.stack(want), sigma=sigma, taps=SIGMAS[sigma])


# ---- the hole stage

HOLE_SHAPES = [(24, 24), (64, 64)]
HOLE_KSIZES = [3, 11, 71]


def hole_frame(h, w, kind):
    """(hmap, reliable): reliable reaches the frame's border on two sides, so the windows reflect across it; NaN marks the unknown pixels"""
    rng = np.random.default_rng([h, w, len(kind)])
    rel = np.zeros((h, w), bool)
    rel[: h - 3, 2:] = True
    rel[h // 2:, : w // 3] = False
    hm = _dyadic(rng, h * w, -128, 32).reshape(h, w)
    hm[~rel] = np.nan
    if kind == "all_nan":
        hm[:] = np.nan
        return hm, rel
    hm[5, 9] = np.nan                                       # single pixels and small clusters well inside
    hm[h // 3:h // 3 + 2, w // 2:w // 2 + 2] = np.nan
    hm[0, w - 4] = np.nan                                   # on the frame's border, at the edge of the reliable region
    hm[1, w - 1] = np.nan
    hm[h - 4, w // 2] = np.nan                              # one pixel from the region's lower edge
    hm[2:9, w - 9:w - 2] = np.nan                           # a 7 x 7 block: few known neighbours at its centre
    if kind == "sparse":
        hm[(rng.random((h, w)) < 0.35) & rel] = np.nan
    return hm, rel


def hole_inputs(hm, rel, ksize):
    """(known fraction float32, distance float32) as compute_internal_holes_within_mask forms them"""
    known = rel & np.isfinite(hm)
    k = max(3, int(ksize) | 1)
    frac = cvlite.box_sum(known.astype(np.float32), k) / (cvlite.box_sum(rel.astype(np.float32), k) + 1e-6)
    return frac.astype(np.float32), cvlite.dist_l2_3x3(rel.astype(np.uint8) * 255)


def hole_thresholds(h, w, ksize, kind):
    """(frac_thr, min_dist) that sit exactly on one hole pixel's own fraction and distance: that pixel passes both tests with equality"""
    hm, rel = hole_frame(h, w, kind)
    frac, dist = hole_inputs(hm, rel, ksize)
    holes = rel & ~np.isfinite(hm)
    ok = holes & (frac >= np.float32(0.3)) & (dist >= np.float32(1.5))
    if not ok.any():
        return 0.6, 2.0
    fr = np.sort(np.unique(frac[ok]))
    frac_thr = fr[len(fr) // 2]
    return float(frac_thr), float(dist[ok & (frac == frac_thr)].min())


def ref_hole_tmp(hm, rel, cand):
    """process_frame :797-799 and inpaint_only_mask :515: (the plane k_hole_tmp writes, the median it takes)"""
    known = rel & np.isfinite(hm)
    tmp = np.where(known, hm, np.float32(np.nan)).astype(np.float32)
    med = float(np.nanmedian(tmp[known])) if np.any(known) else 0.0
    tmp[rel & ~known] = med
    known2 = rel & ~cand & np.isfinite(tmp)
    med32 = np.float32(np.nanmedian(hm[known])) if np.any(known) else np.float32(np.nan)      # a selection without an element hands back NaN
    return np.where(known2, tmp, np.float32(np.nan)).astype(np.float32), med32


def ref_hole_zin(tmp):
    """inpaint_only_mask :516-518 on the plane above: (zin, the median it takes)"""
    known = np.isfinite(tmp)
    fill = float(np.nanmedian(tmp[known])) if np.any(known) else 0.0
    zin = np.full_like(tmp, fill, dtype=np.float32)
    zin[known] = tmp[known]
    return zin, (np.float32(fill) if np.any(known) else np.float32(np.nan))


def ref_hole_merge(hm, rel, cand, zin):
    """process_frame :791-802: (height_rel, output_reliable)"""
    known = rel & np.isfinite(hm)
    height_rel = np.full(hm.shape, np.nan, np.float32)
    height_rel[known] = hm[known]
    height_rel[cand] = zin[cand]
    return height_rel, (rel & np.isfinite(height_rel)).astype(np.uint8)


# =======================================================================================================================================
# the back end from the candidates on

BACKEND_LAYOUTS = ("interlocked_combs", "border_ring", "zeros", "random_0.41", "checker", "tie_equal_areas")
# (min_peak_mm, rel_frac): the relative threshold wins; the absolute one wins; rel_frac < 0 switches the relative one off
BACKEND_THRESHOLDS = [(0.2, 0.5), (1.25, 0.3), (0.55, -1.0)]
BACKEND_GMAX = np.float32(2.0)


def backend_roi(h, w):
    roi = np.ones((h, w), np.uint8)
    if h > 8 and w > 8:
        roi[h // 2, w // 3:w // 3 + 3] = 0                  # a few pixels inside the blobs' area that are not ROI
    return roi


def backend_frame(h, w, layout, min_peak, rel_frac, seed):
    """(depth, cand, gmax, unitless) of one frame.  The blobs are a hard mask's components; the largest holds the frame maximum, the next one
    peaks exactly at the blob threshold and the third one float32 below it."""
    roi = backend_roi(h, w) != 0
    rng = np.random.default_rng([h, w, seed])
    if layout == "border_ring":                             # one component touching all four borders
        m = np.zeros((h, w), bool)
        m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = True
    else:
        m = M.hard_masks(h, w, 1000 * h + w)[layout] != 0
    m &= roi
    depth = np.zeros((h, w), np.float32)
    depth[m] = _dyadic(rng, int(m.sum()), 1, 120)           # 1/64 .. 1.875, below the frame maximum
    lab = M.ref_labels(m)
    roots, areas = M.component_areas(lab)
    order = roots[np.argsort(-areas, kind="stable")]
    thr = M.blob_threshold(BACKEND_GMAX, min_peak, rel_frac)
    pinned = {}
    for root, peak, name in zip(order[:3], (BACKEND_GMAX, thr, np.nextafter(thr, np.float32(0))), ("max", "at_thr", "below_thr")):
        sel = lab == root
        depth[sel] = np.minimum(depth[sel], peak)
        idx = np.flatnonzero(sel.ravel())
        depth.ravel()[idx[len(idx) // 2]] = peak
        pinned[name] = int(root)
    depth[~roi] = np.nan
    cand = roi & np.isfinite(depth) & (depth > 0)
    gmax = np.float32(depth[cand].max()) if cand.any() else np.float32(0)
    unitless = np.where(roi, -_dyadic(rng, h * w, 0, 200).reshape(h, w), np.float32(np.nan)).astype(np.float32)
    return depth, cand.astype(np.uint8), gmax, unitless, pinned


def ref_backend(depth, roi, unitless, status, reliable, min_peak, rel_frac, mm_per_px=TAIL_MM_PER_PX, eps=TAIL_EPS):
    """filter_blobs_by_peak_depth_mm, the force tail as process_frame calls it, and the copy to the caller's planes, for one frame"""
    out, kept = O.filter_blobs_by_peak_depth_mm(depth, roi, min_peak, rel_frac if rel_frac >= 0 else None)
    cand = (np.asarray(roi) != 0) & np.isfinite(depth) & (depth > 0)
    lab = M.ref_labels(cand)
    tail = ref_tail(out, None, unitless, roi, mm_per_px, eps)
    empty = status in (1, 3)
    out_h = np.full(out.shape, np.nan, np.float32) if empty else out
    out_r = np.zeros(out.shape, np.uint8) if empty else (np.asarray(reliable) != 0).astype(np.uint8)
    return dict(depth=out, kept=kept.astype(np.uint8), labels=lab, tail=tail, out_h=out_h, out_r=out_r)
