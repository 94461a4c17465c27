"""The temporal read-out (include/vistaf_temporal.h) restated in NumPy, the hand-made streams of tests/test_temporal.py and the comparison.

`numpy_temporal` follows the header frame by frame with explicit np.float32 / np.float64 operations (NumPy's element-wise ufuncs never fuse
a product with a sum); the float64 sum behind the volume is math.fsum, which is exact, so the bar below is the error of the device's sum alone.

THE BAR on FILTERED_VOLUME_CM3 is (2 N + 16) * 2^-53 of the volume, N the frame's touch pixels: the bar of taxels_helpers.worst_excess for a
float64 sum of N non-negative terms in any order (N - 1 roundings, each below 2^-53 of the final sum) with room for the three operations
that scale it.  DVOLUME_CM3_PER_S is a difference of two such volumes over the interval: the same factor, relative to the larger of the two
volumes over the interval.  Every other field, the planes, the state and the NaN pattern must be equal.
"""
import math

import numpy as np

U = 2.0 ** -53
NAMES = ["touch_pixels", "onset_pixels", "release_pixels", "loading_pixels", "unloading_pixels", "filtered_volume_cm3", "dvolume_cm3_per_s",
         "max_filtered_mm", "argmax_index", "max_rate_mm_per_s", "max_rate_index", "min_rate_mm_per_s", "min_rate_index",
         "longest_dwell_frames", "events", "gap_frames"]
R_ = {n: i for i, n in enumerate(NAMES)}
NTEMPORAL = 16
SUMMED = ("filtered_volume_cm3", "dvolume_cm3_per_s")
EXACT = [n for n in NAMES if n not in SUMMED]
BEGAN, ENDED = 1, 2
STATE_PLANES = (("filt", np.float32), ("rate", np.float32), ("touch", np.uint8), ("dwell", np.int32), ("hold", np.float32))
DYADIC = dict(alpha=0.5, on_mm=0.5, off_mm=0.25, frame_period_s=1.0 / 32.0)
GENERAL = dict(alpha=0.3, on_mm=0.05, off_mm=0.02, frame_period_s=1.0 / 30.0)


def new_state(P):
    """the state after create or reset"""
    return dict(filt=np.zeros(P, np.float32), rate=np.zeros(P, np.float32), touch=np.zeros(P, np.uint8), dwell=np.zeros(P, np.int32),
                hold=np.zeros(P, np.float32), primed=False, gap=0, prev_touch=0, prev_volume=float("nan"))


def numpy_temporal(depth, mm_per_px, status, alpha, on_mm, off_mm, frame_period_s, state=None, trace=None):
    """depth [B,h,w], mm_per_px [B], status [B] or None.  Returns (rows [B,16] f64, filtered [B,h,w] f32, touch [B,h,w] u8, state): the
    state dict (flat planes and the stream scalars) is a new one, `state` (None: after create) is left alone.  trace, a list, receives per
    accepted frame a dict of the frame's f, fp, rate, was, now (flat arrays) for the coverage assertions of the stream builders."""
    depth = np.asarray(depth, np.float32)
    B, h, w = depth.shape
    P = h * w
    a, on, off, zero = np.float32(alpha), np.float32(on_mm), np.float32(off_mm), np.float32(0.0)
    period = np.float64(frame_period_s)
    st = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in (state or new_state(P)).items()}
    rows = np.full((B, NTEMPORAL), np.nan, np.float64)
    filtered, touch = np.empty((B, P), np.float32), np.empty((B, P), np.uint8)
    for b in range(B):
        rows[b, R_["gap_frames"]] = st["gap"]
        if status is not None and int(status[b]) != 0:
            filtered[b], touch[b] = st["filt"], st["touch"]
            st["gap"] += 1
            continue
        x = depth[b].ravel()
        d = np.where(np.isfinite(x), x, zero).astype(np.float32)
        fp = st["filt"] if st["primed"] else d
        with np.errstate(all="ignore"):
            diff = (d - fp).astype(np.float32)
            prod = (a * diff).astype(np.float32)
            f = (fp + prod).astype(np.float32)
            den = np.float64(st["gap"] + 1) * period
            rate = ((f - fp).astype(np.float32).astype(np.float64) / den).astype(np.float32)
        was = st["touch"].astype(bool)
        now = np.where(was, f > off, f >= on)
        dwell = np.where(now == was, st["dwell"] + 1, 0).astype(np.int32)
        base = np.where(was, st["hold"], zero).astype(np.float32)
        hold = np.where(now, np.where(d > base, d, base), zero).astype(np.float32)
        if trace is not None:
            trace.append(dict(frame=b, f=f, fp=fp.copy(), rate=rate, was=was, now=now, d=d))
        n = int(now.sum())
        s = float(mm_per_px[b])
        vol = math.fsum(f[now].astype(np.float64).tolist()) * (s * s) / 1000.0 if n else 0.0
        r = rows[b]
        r[0], r[1], r[2] = n, int((now & ~was).sum()), int((was & ~now).sum())
        r[3], r[4] = int((now & (f > fp)).sum()), int((now & (f < fp)).sum())
        r[5] = vol
        r[6] = (np.float64(vol) - np.float64(st["prev_volume"])) / den if st["primed"] else np.nan
        if n:
            idx = np.flatnonzero(now)
            r[7], r[8] = float(f[idx].max()), int(idx[np.argmax(f[idx])])                  # argmax / argmin: the first occurrence
            r[9], r[10] = float(rate[idx].max()), int(idx[np.argmax(rate[idx])])
            r[11], r[12] = float(rate[idx].min()), int(idx[np.argmin(rate[idx])])
            r[13] = int(dwell[idx].max())
        r[14] = (BEGAN if st["prev_touch"] == 0 and n > 0 else 0) | (ENDED if st["prev_touch"] > 0 and n == 0 else 0)
        st.update(filt=f, rate=rate, touch=now.astype(np.uint8), dwell=dwell, hold=hold, primed=True, gap=0, prev_touch=n, prev_volume=vol)
        filtered[b], touch[b] = f, st["touch"]
    return rows, filtered.reshape(B, h, w), touch.reshape(B, h, w), st


# ---------------------------------------------------------------------------------------------------------------- streams
def _blob(rng, B, rows, cols, top, low, grid):
    """random depths on the 1/grid lattice in [0, top], frames 0 and 1 in [0, low]"""
    q = rng.integers(0, int(top * grid) + 1, size=(B, rows, cols)).astype(np.float32) / np.float32(grid)
    q[:2] = rng.integers(0, int(low * grid) + 1, size=(2, rows, cols)).astype(np.float32) / np.float32(grid)
    return q


def stream(h, w, params, seed=0):
    """Seven frames in which every branch of the definition occurs, asserted below on the reference's own trace.  Written for the DYADIC
    parameters (alpha 0.5, on 0.5, off 0.25; depths on the 1/64 lattice, so every f is exact and the threshold equalities are hit); for
    other parameters the depths are scaled by on / 0.5 and the equalities are not asserted.  status: frame 0 (the very first of the stream)
    and frame 3 are skipped and full of 1e30; frame 1, the first accepted one, touches nowhere."""
    B, P = 7, h * w
    assert P > 1600
    dyadic = params == DYADIC
    rng = np.random.default_rng(seed)
    status = np.array([2, 0, 0, 1, 0, 0, 0], np.int32)
    d = rng.integers(0, 9, size=(B, P)).astype(np.float32) / np.float32(64.0)                # the floor: 0 .. 0.125, below off
    blob = _blob(rng, B, 16, 33, 1.5, 0.25, 64)                                              # frame 1: <= 0.25, below on; |f - fp| <= 0.75
    img = d.reshape(B, h, w)
    img[:, 10:26, 8:41] = blob
    A, Bx, C, D, E1, E2, G1, G2, N1, N2, N3, N4, R = 5, P - 1, 300, 1400, 450, 1500, 64, 65, 130, 131, 1450, 1550, 1420
    for p in (A, Bx, C, D, E1, E2, G1, G2, N1, N2, N3, N4, R):
        y, x = divmod(p, w)
        assert not (10 <= y < 26 and 8 <= x < 41), p                                         # the role pixels lie outside the blob
    nan, inf = np.float32("nan"), np.float32("inf")
    #            frame:  0  1      2     3  4     5      6
    roles = {A: (0, 0.25, 0.75, 0, 0.75, 0.75, 0.75),        # f = 0.5 == on in frame 2: must touch
             Bx: (0, 0.0, 1.0, 0, 0.0, 0.0, 1.0),            # touches in 2, f = 0.25 == off in frame 4: must release
             C: (0, 0.375, 0.375, 0, 0.375, 0.375, 0.375),   # between the thresholds, never touching
             D: (0, 0.0, 1.5, 0, 0.0, 0.375, 0.375) if dyadic else (0, 0.0, 3.0, 0, 0.0, 0.0, 0.44),   # touching, then f between the thresholds: holds
             E1: (0, 0.0, 8.0, 0, 8.0, 8.0, 0.0), E2: (0, 0.0, 8.0, 0, 8.0, 8.0, 0.0),       # tie the maximum and the largest rate
             G1: (0, 0.0, 7.0, 0, 0.0, 7.0, 7.0), G2: (0, 0.0, 7.0, 0, 0.0, 7.0, 7.0),       # tie the smallest rate in frame 4
             R: (0, 0.0, 2.0, 0, -1.0, 0.0, 0.0),            # touches in 2, a negative depth releases it in 4, whatever the parameters
             N1: (0, nan, nan, 0, 1.0, nan, 1.0), N2: (0, 0.0, inf, 0, 1.0, 1.0, -inf),
             N3: (0, 0.0, 1.0, 0, -inf, inf, nan), N4: (0, 0.0, 1.0, 0, inf, 1.0, 1.0)}      # inf while touching: d = 0, f = 0.25, releases
    for p, v in roles.items():
        d[:, p] = np.array(v, np.float32)
    scale = np.float32(1.0) if dyadic else np.float32(params["on_mm"] / 0.5)
    d = (d * scale).astype(np.float32)
    d[0], d[3] = np.float32(1e30), np.float32(1e30)                                          # skipped: must not be read
    depth = d.reshape(B, h, w)
    mpp = np.array([0.05, 0.05, 0.0625, 0.05, 0.05, 0.047, 0.05])
    c = dict(depth=depth, mpp=mpp, status=status, params=params, shape=(h, w))
    trace = []
    rows, _, _, _ = numpy_temporal(depth, mpp, status, trace=trace, **params)
    tr = {t["frame"]: t for t in trace}
    on, off = np.float32(params["on_mm"]), np.float32(params["off_mm"])
    assert sorted(tr) == [1, 2, 4, 5, 6] and rows[1, 0] == 0 and rows[2, 0] > 20                       # an all-empty frame, then many pixels
    assert np.isnan(rows[[0, 3], :15]).all() and rows[:, 15].tolist() == [0, 1, 0, 0, 1, 0, 0]          # skipped first frame, skipped in the middle
    assert rows[2, 14] == BEGAN and rows[1, 14] == 0
    if dyadic:
        assert tr[2]["f"][A] == on and tr[2]["now"][A] and not tr[2]["was"][A]                         # f == on touches
        assert tr[4]["f"][Bx] == off and tr[4]["was"][Bx] and not tr[4]["now"][Bx]                     # f == off releases
        assert tr[4]["f"][N4] == off and not tr[4]["now"][N4]
    for t in (1, 2, 4, 5, 6):
        assert off < tr[t]["f"][C] < on and not tr[t]["now"][C]                                       # between, not touching
    for t in (4, 5, 6) if dyadic else (5, 6):
        assert off < tr[t]["f"][D] < on and tr[t]["now"][D] and tr[t]["was"][D]                       # between, touching
    assert not np.isfinite(depth[[1, 2, 4, 5, 6]]).all() and np.isnan(depth[2]).any() and np.isposinf(depth[2]).any() and np.isneginf(depth[4]).any()
    for t, field, pair in ((2, "max_filtered_mm", (E1, E2)), (2, "max_rate_mm_per_s", (E1, E2)), (4, "max_filtered_mm", (E1, E2)),
                           (4, "min_rate_mm_per_s", (G1, G2))):
        key = "f" if field == "max_filtered_mm" else "rate"
        v = tr[t][key]
        assert v[pair[0]] == v[pair[1]] == rows[t, R_[field]] and rows[t, R_[field] + 1] == pair[0], (t, field)   # two pixels tie, the lower index wins
        assert (v[tr[t]["now"]] == v[pair[0]]).sum() == 2
    assert (np.nansum(rows[:, 1:5], axis=0) > 0).all() and (rows[[4, 5, 6], 1] > 0).all() and rows[4, 2] > 0                 # onsets, releases, loading, unloading
    return c


def big_stream(h=131, w=127, seed=3):
    """Three frames, every frame accepted, 16 637 pixels: more than 64 chunks of 256, touching pixels in all of them, the maximum tied by a
    pixel of the first chunk and one of the last."""
    B, P = 3, h * w
    rng = np.random.default_rng(seed)
    d = (rng.integers(0, 129, size=(B, P)).astype(np.float32) / np.float32(64.0))
    d[0] = rng.integers(0, 17, size=P).astype(np.float32) / np.float32(64.0)
    d[:, [100, P - 50]] = np.array([0.0, 4.0, 4.0], np.float32)[:, None]
    c = dict(depth=d.reshape(B, h, w), mpp=np.array([0.05, 0.051, 0.049]), status=None, params=DYADIC, shape=(h, w))
    rows = numpy_temporal(c["depth"], c["mpp"], None, **DYADIC)[0]
    assert rows[0, 0] == 0 and rows[1, 0] > 3000 and rows[1, 8] == 100 and rows[2, 8] == 100 and (P + 255) // 256 > 64
    return c


def reference(c):
    return numpy_temporal(c["depth"], c["mpp"], c["status"], **c["params"])


# ---------------------------------------------------------------------------------------------------------------- comparison
def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def exact_rows_equal(got, want):
    """the NaN pattern of every field and the value of every field without a sum behind it"""
    return got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)) and \
        all(np.array_equal(got[:, R_[k]], want[:, R_[k]], equal_nan=True) for k in EXACT)


def worst_excess(got, want, frame_period_s):
    """largest |got - want| / bar over the two summed fields and the frames (<= 1 passes), and where; a bar of 0 asks for equality"""
    worst, where = 0.0, None
    prev = None
    for b in range(want.shape[0]):
        if np.isnan(want[b, 0]):
            continue
        bar = (2.0 * want[b, 0] + 16.0) * U
        vol = want[b, 5]
        scales = {"filtered_volume_cm3": vol}
        if prev is not None:
            scales["dvolume_cm3_per_s"] = max(vol, prev) / ((want[b, 15] + 1.0) * frame_period_s)
        for k, sc in scales.items():
            err = abs(got[b, R_[k]] - want[b, R_[k]])
            ratio = 0.0 if err == 0.0 else (err / (bar * sc) if sc > 0.0 else np.inf)
            if ratio > worst:
                worst, where = float(ratio), (k, b)
        prev = vol
    return worst, where
