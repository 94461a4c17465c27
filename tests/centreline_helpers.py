"""The centreline read-out (include_ext/vistaf_centreline.h) restated in NumPy and plain Python float64: Guo-Hall thinning by whole-plane boolean
operations, the exact squared distance by a column pass and an integer minimum over the row, the walk by a plain queue, the measures by the
header's expressions one IEEE operation at a time.  Slow and obvious on purpose: the kernel thins bit-sliced on 64-pixel words, finds the
distance by probing the rows around a pixel and walks with a bit-plane frontier; this does none of that."""
import math
from collections import deque

import numpy as np

from outline_helpers import Scene, clamp_count, components, pack, rect, ring, row_mask  # noqa: F401  (scenes and the box rules are shared)

NCENTRELINE = 40
FIELDS = ["pixels", "skeleton_pixels", "thinning_passes", "end_pixels", "branch_pixels", "stations", "stations_written", "status", "a_x", "a_y",
          "b_x", "b_y", "path_length_mm", "length_mm", "chord_mm", "tortuosity", "sagitta_mm", "sagitta_station", "interior_stations",
          "width_mean_mm", "width_min_mm", "width_min_station", "width_max_mm", "width_max_station", "width_seed_mm", "elongation", "a_tx", "a_ty",
          "b_tx", "b_ty", "a_at_border", "b_at_border", "depth_mean_mm", "depth_a_mm", "depth_b_mm", "depth_peak_mm", "depth_peak_station"]
F = {n: i for i, n in enumerate(FIELDS)}
OK, NO_PIXELS, POINT, BRANCHED, TRUNCATED = 0, 1, 2, 8, 16
NAN = float("nan")
# the walk's neighbour order: N, E, S, W, NE, SE, SW, NW as (dx, dy), y pointing down
STEPS = [(0, -1), (1, 0), (0, 1), (-1, 0), (1, -1), (1, 1), (-1, 1), (-1, -1)]


# ------------------------------------------------------------------------------------------------------------------------------- thinning
def neighbours(s):
    """P2..P9 of every pixel (N, NE, E, SE, S, SW, W, NW), zero outside the plane"""
    p = np.pad(s, 1)
    h, w = s.shape

    def at(dx, dy):
        return p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    return at(0, -1), at(1, -1), at(1, 0), at(1, 1), at(0, 1), at(-1, 1), at(-1, 0), at(-1, -1)


def thin(m):
    """(skeleton, passes): Guo-Hall thinning of the boolean plane m, the pair of sub-iterations repeated until a pair deletes nothing"""
    s, passes = np.array(m, bool), 0
    while True:
        deleted = False
        for it in (0, 1):
            P2, P3, P4, P5, P6, P7, P8, P9 = neighbours(s)
            C = (~P2 & (P3 | P4)).astype(int) + (~P4 & (P5 | P6)) + (~P6 & (P7 | P8)) + (~P8 & (P9 | P2))
            N1 = (P9 | P2).astype(int) + (P3 | P4) + (P5 | P6) + (P7 | P8)
            N2 = (P2 | P3).astype(int) + (P4 | P5) + (P6 | P7) + (P8 | P9)
            N = np.minimum(N1, N2)
            keep = ((P2 | P3 | ~P5) & P4) if it == 0 else ((P6 | P7 | ~P9) & P8)
            d = s & (C == 1) & (N >= 2) & (N <= 3) & ~keep
            if d.any():
                deleted = True
                s = s & ~d
        if not deleted:
            return s, passes
        passes += 1


def holes(m):
    """4-connected background components that do not reach the outside"""
    return components(np.pad(~np.asarray(m, bool), 1, constant_values=True), False) - 1


def end_and_branch_pixels(s):
    P = neighbours(s)
    n = sum(p.astype(int) for p in P)
    ring8 = list(P) + [P[0]]
    t = sum((~ring8[i] & ring8[i + 1]).astype(int) for i in range(8))
    return int((s & (n == 1)).sum()), int((s & (t >= 3)).sum())


# ------------------------------------------------------------------------------------------------------------------------------- distance
def d2_plane(m):
    """exact squared Euclidean distance (int64) from every pixel of m to the nearest position that is not in m; the ring just outside the plane
    counts as not in m (and nothing farther out can be nearer).  Separable: the distance g within the column, then the minimum of
    dx^2 + g(x + dx)^2 over the row, |dx| up to the largest g."""
    h, w = m.shape
    p = np.pad(np.asarray(m, bool), 1)
    up = np.zeros(p.shape, np.int64)
    for y in range(1, h + 2):
        up[y] = np.where(p[y], up[y - 1] + 1, 0)
    down = np.zeros(p.shape, np.int64)
    for y in range(h, -1, -1):
        down[y] = np.where(p[y], down[y + 1] + 1, 0)
    g = np.minimum(up, down)
    best = g * g
    gmax = int(g.max())
    for dx in range(1, gmax + 1):
        for sgn in (-1, 1):
            sh = np.zeros(g.shape, np.int64)                      # beyond the ring: not in m either, g = 0
            if sgn > 0:
                sh[:, :-dx] = g[:, dx:]
            else:
                sh[:, dx:] = g[:, :-dx]
            best = np.minimum(best, dx * dx + sh * sh)
    return np.where(p, best, 0)[1:-1, 1:-1]


def d2_brute(m):
    h, w = m.shape
    p = np.pad(np.asarray(m, bool), 1)
    ys, xs = np.nonzero(~p)
    out = np.zeros((h, w), np.int64)
    for y, x in zip(*np.nonzero(m)):
        out[y, x] = ((ys - (y + 1)) ** 2 + (xs - (x + 1)) ** 2).min()
    return out


# ----------------------------------------------------------------------------------------------------------------------------------- walk
def hops(s, start):
    """hop counts over 8-adjacent pixels of s from start (x, y), -1 where s is not reached"""
    h, w = s.shape
    d = -np.ones((h, w), np.int64)
    d[start[1], start[0]] = 0
    q = deque([start])
    while q:
        x, y = q.popleft()
        for dx, dy in STEPS:
            u, v = x + dx, y + dy
            if 0 <= u < w and 0 <= v < h and s[v, u] and d[v, u] < 0:
                d[v, u] = d[y, x] + 1
                q.append((u, v))
    return d


def first_largest(values, where):
    """(x, y) of the largest value among the pixels of `where`, ties to the smallest (y, x)"""
    ys, xs = np.nonzero(where)                                      # row-major: (y, x) ascending
    v = values[ys, xs]
    i = int(np.argmax(v))                                           # the first of the largest
    return int(xs[i]), int(ys[i])


def walk(s, d2):
    """(path from A to B as a list of (x, y), seed): header, step 4"""
    seed = first_largest(d2, s)
    from_seed = hops(s, seed)
    a0 = first_largest(from_seed, from_seed >= 0)
    lev = hops(s, a0)
    b0 = first_largest(lev, lev >= 0)
    h, w = s.shape
    path, cur = [b0], b0
    while cur != a0:
        x, y = cur
        for dx, dy in STEPS:
            u, v = x + dx, y + dy
            if 0 <= u < w and 0 <= v < h and lev[v, u] == lev[y, x] - 1:
                cur = (u, v)
                break
        else:
            raise AssertionError("no neighbour one hop nearer")
        path.append(cur)
    if (path[-1][1], path[-1][0]) < (path[0][1], path[0][0]):
        path.reverse()
    return path, seed


# ------------------------------------------------------------------------------------------------------------------------------- measures
def measure_mask(m, s, depth=None, tangent_span=8):
    """the record (list of 40) of the boolean frame-sized plane m at scale s, its stations [(x, y)], their D2 and the skeleton plane.
    STATIONS_WRITTEN is 0 and TRUNCATED set as if no polyline were asked for: `reference` applies the capacity rule."""
    h, w = m.shape
    rec = [NAN] * NCENTRELINE
    if not m.any():
        for i in range(7):
            rec[i] = 0.0
        rec[F["status"]] = float(NO_PIXELS)
        return rec, [], [], np.zeros((h, w), bool)
    d2 = d2_plane(m)
    sk, passes = thin(m)
    ends, branches = end_and_branch_pixels(sk)
    path, seed = walk(sk, d2)
    n = len(path)
    A, B = path[0], path[-1]
    dd = [int(d2[y, x]) for x, y in path]
    a = sum(1 for p, q in zip(path, path[1:]) if (p[0] == q[0]) != (p[1] == q[1]))
    b = n - 1 - a
    s = float(s)
    chord2 = (B[0] - A[0]) ** 2 + (B[1] - A[1]) ** 2
    core = float(a) + float(b) * math.sqrt(2.0)
    rec[F["pixels"]], rec[F["skeleton_pixels"]], rec[F["thinning_passes"]] = float(m.sum()), float(sk.sum()), float(passes)
    rec[F["end_pixels"]], rec[F["branch_pixels"]], rec[F["stations"]], rec[F["stations_written"]] = float(ends), float(branches), float(n), 0.0
    rec[F["status"]] = float((POINT if n == 1 else OK) | (BRANCHED if branches else 0) | TRUNCATED)
    rec[F["a_x"]], rec[F["a_y"]], rec[F["b_x"]], rec[F["b_y"]] = float(A[0]), float(A[1]), float(B[0]), float(B[1])
    rec[F["path_length_mm"]] = core * s
    rec[F["length_mm"]] = (((core + math.sqrt(float(dd[0]))) + math.sqrt(float(dd[-1]))) - 1.0) * s
    rec[F["chord_mm"]] = math.sqrt(float(chord2)) * s
    if n >= 2:
        rec[F["tortuosity"]] = rec[F["path_length_mm"]] / rec[F["chord_mm"]]
    best, at = 0, 0
    for i, (x, y) in enumerate(path):
        c = (B[0] - A[0]) * (y - A[1]) - (B[1] - A[1]) * (x - A[0])
        if abs(c) > abs(best):
            best, at = c, i
    if n >= 2:
        rec[F["sagitta_mm"]] = float(best) / math.sqrt(float(chord2)) * s
    rec[F["sagitta_station"]] = float(at)
    cnt, total, lo, lo_at, hi, hi_at = 0, 0.0, NAN, NAN, NAN, NAN
    for i, (x, y) in enumerate(path):
        if (x - A[0]) ** 2 + (y - A[1]) ** 2 >= 4 * dd[i] and (x - B[0]) ** 2 + (y - B[1]) ** 2 >= 4 * dd[i]:
            wd = (2.0 * math.sqrt(float(dd[i])) - 1.0) * s
            total = wd if cnt == 0 else total + wd
            if cnt == 0 or wd < lo:
                lo, lo_at = wd, float(i)
            if cnt == 0 or wd > hi:
                hi, hi_at = wd, float(i)
            cnt += 1
    rec[F["interior_stations"]] = float(cnt)
    if cnt:
        rec[F["width_mean_mm"]] = total / float(cnt)
        rec[F["width_min_mm"]], rec[F["width_min_station"]], rec[F["width_max_mm"]], rec[F["width_max_station"]] = lo, lo_at, hi, hi_at
    rec[F["width_seed_mm"]] = (2.0 * math.sqrt(float(d2[seed[1], seed[0]])) - 1.0) * s
    rec[F["elongation"]] = rec[F["length_mm"]] / rec[F["width_seed_mm"]]
    if n >= 2:
        j = min(n - 1, tangent_span)
        for name, o, q in (("a", A, path[j]), ("b", B, path[n - 1 - j])):
            r = math.sqrt(float((q[0] - o[0]) ** 2 + (q[1] - o[1]) ** 2))
            rec[F[name + "_tx"]], rec[F[name + "_ty"]] = float(q[0] - o[0]) / r, float(q[1] - o[1]) / r
    for name, (x, y), d in (("a", A, dd[0]), ("b", B, dd[-1])):
        rec[F[name + "_at_border"]] = 1.0 if min(x + 1, y + 1, w - x, h - y) ** 2 <= d else 0.0
    if depth is not None:
        z = [float(depth[y, x]) for x, y in path]
        k = min(n, tangent_span + 1)

        def mean(v):
            t = v[0]
            for u in v[1:]:
                t = t + u
            return t / float(len(v))
        rec[F["depth_mean_mm"]], rec[F["depth_a_mm"]], rec[F["depth_b_mm"]] = mean(z), mean(z[:k]), mean(z[n - k:])
        pk, pk_at = z[0], 0
        for i, v in enumerate(z):
            if v > pk:
                pk, pk_at = v, i
        rec[F["depth_peak_mm"]], rec[F["depth_peak_station"]] = pk, float(pk_at)
    return rec, path, dd, sk


def reference(index, contacts, count, mm_per_px, depth=None, tangent_span=8, max_stations=None):
    """{"centrelines" [B,K,40], "stations": per frame the list of (x, y) written, "d2": per frame their D2, "offsets" [B,K+1] int32,
    "skeleton" [B,h,w] int8}; max_stations None: no polyline asked for"""
    B, K = contacts.shape[:2]
    out = np.full((B, K, NCENTRELINE), np.nan)
    stations, d2s, offsets = [], [], np.zeros((B, K + 1), np.int32)
    skeleton = np.full(index.shape, -1, np.int8)
    for b in range(B):
        total, ok, sb, db = 0, True, [], []
        for k in range(K):
            if k < clamp_count(count[b], K):
                rec, path, dd, sk = measure_mask(row_mask(index[b], contacts[b, k], k), mm_per_px[b], None if depth is None else depth[b], tangent_span)
                skeleton[b][sk] = k
                total += len(path)
                ok = ok and max_stations is not None and total <= max_stations
                if ok and path:
                    sb += path
                    db += dd
                    rec[F["stations_written"]] = float(len(path))
                    rec[F["status"]] = float(int(rec[F["status"]]) & ~TRUNCATED)
                out[b, k] = rec
            offsets[b, k + 1] = len(sb)
        stations.append(sb)
        d2s.append(db)
    return {"centrelines": out, "stations": stations, "d2": d2s, "offsets": offsets, "skeleton": skeleton}


# ---------------------------------------------------------------------------------------------------------------------------------- scenes
def bar(h, w, x0, y0, x1, y1):
    return rect(h, w, x0, y0, x1, y1)


def disc(h, w, cx, cy, r):
    yy, xx = np.mgrid[0:h, 0:w]
    return (xx - cx) ** 2 + (yy - cy) ** 2 <= r * r


def arc(h, w, cx, cy, r, thick, a0, a1):
    """the part of the annulus of mean radius r and thickness `thick` about (cx, cy) between the angles a0 < a1 (radians, atan2(dy, dx))"""
    yy, xx = np.mgrid[0:h, 0:w]
    rr, ang = np.hypot(xx - cx, yy - cy), np.arctan2(yy - cy, xx - cx)
    return (np.abs(rr - r) <= thick / 2.0) & (ang >= a0) & (ang <= a1)


def sine_cable(h, w, amp, period, thick):
    """a cable across the whole width of the frame about its middle row"""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.abs(yy - (h / 2.0 + amp * np.sin(2.0 * np.pi * xx / period))) <= thick / 2.0


def diagonal_bar(h, w, x0, y0, n, thick):
    m = np.zeros((h, w), bool)
    for i in range(n):
        m[y0 + i, x0 + i:x0 + i + thick] = True
    return m


def tee(h, w, x0, y0, length, stem, thick):
    """a bar of `length` x `thick` from (x0, y0) with a stem of `stem` pixels hanging from its middle"""
    xm = x0 + length // 2
    return rect(h, w, x0, y0, x0 + length - 1, y0 + thick - 1) | rect(h, w, xm - thick // 2, y0, xm - thick // 2 + thick - 1, y0 + thick - 1 + stem)


def hand_made(h, w):
    """the hand-made frames of the read-out's tests at h x w (at least 24 x 32), K = 8.  Returns (names, packed case); the depth plane of the
    case is a fixed smooth float32 field"""
    scenes, names = [], []

    def add(name):
        names.append(name)
        scenes.append(Scene(h, w))
        return scenes[-1]
    sc = add("bars")
    sc.paint(0, bar(h, w, 3, 1, w - 4, 1)).paint(1, bar(h, w, 2, 3, w - 6, 4)).paint(2, bar(h, w, 4, 6, w - 3, 12)).paint(3, bar(h, w, 1, 14, w - 2, 21))
    sc = add("diagonal_tee_pixel")
    one = np.zeros((h, w), bool)
    one[2, w - 3] = True
    sc.paint(0, diagonal_bar(h, w, 1, 1, 12, 3)).paint(1, tee(h, w, 14, 8, 15, 9, 3)).paint(2, one)
    sc.paint(3, bar(h, w, 1, 16, 1, 22))                                                       # a vertical bar of width 1
    sc = add("ring_disc_empty_pieces")
    sc.paint(0, ring(h, w, 8, 8, 7, 3)).paint(1, disc(h, w, 24, 7, 6))
    sc.paint(2, np.zeros((h, w), bool), box=[3, 17, 8, 20])                                    # a row in use without a pixel
    sc.paint(3, bar(h, w, 1, 18, 9, 20) | bar(h, w, 14, 17, 29, 21))                           # a label in two pieces
    sc = add("borders_and_corner")
    sc.paint(0, bar(h, w, 0, 9, 11, 11)).paint(1, bar(h, w, w - 10, 4, w - 1, 6)).paint(2, bar(h, w, 15, 0, 17, 9))
    sc.paint(3, bar(h, w, 20, h - 9, 21, h - 1)).paint(4, bar(h, w, 0, 0, 8, 2)).paint(5, bar(h, w, w - 3, h - 8, w - 1, h - 1))
    sc.paint(6, bar(h, w, 0, h - 2, 12, h - 1)).paint(7, bar(h, w, 4, 14, 13, 17))             # the last one touches nothing
    sc = add("clipped_and_bad_boxes")
    sc.paint(0, bar(h, w, 2, 2, 20, 5), box=[6, 2, 20, 5])                                     # a box that cuts its label
    sc.paint(1, bar(h, w, 1, 17, 9, 21), box=[-5, 15, 9, 1000])                                # a box that leaves the frame
    sc.paint(2, bar(h, w, 12, 8, 25, 10), box=[np.nan, 8, 25, 10])                             # a box that cannot be read
    sc.paint(3, bar(h, w, 12, 13, 25, 15), box=[25, 13, 12, 15])                               # an inverted box
    sc.paint(4, bar(h, w, 24, 17, 30, 22), box=[w + 3, 17, w + 9, 22])                         # a box wholly outside the frame
    for name, cnt in (("count_above_K", 11), ("count_zero", 0)):
        sc = add(name)
        sc.paint(0, bar(h, w, 2, 2, 20, 6)).paint(1, ring(h, w, 16, 15, 6, 3))
        sc.count = cnt
    case = pack(scenes, 0.0731)
    yy, xx = np.mgrid[0:h, 0:w]
    case["depth"] = np.stack([(0.25 + 0.01 * ((3 * xx + 5 * yy + 7 * b) % 23) + 0.003 * xx).astype(np.float32) for b in range(len(scenes))])
    return names, case
