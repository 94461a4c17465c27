"""The lobe read-out (include_ext/vistaf_lobes.h) restated in NumPy and plain Python: steps 0 to 10 of the header, the ascent pixel by pixel,
the merge by Kruskal over ALL passes with a plain union-find, the sums by plain float64 additions in row-major order.  Slow and
obvious on purpose: the kernel packs the order into one key, jumps pointers, builds the spanning forest by Boruvka rounds and replays only its
edges; this does none of that."""
import math

import numpy as np

from outline_helpers import Scene, clamp_count, components, pack, rect, ring, row_mask  # noqa: F401  (scenes and the box rules are shared)

NLOBE, NLOBEROW, NCONTACT = 16, 12, 16
LOBE_FIELDS = ["x", "y", "depth_mm", "prominence_mm", "saddle_x", "saddle_y", "saddle_depth_mm", "neighbour", "pixels", "contact_pixels", "area_mm2",
               "volume_cm3", "centroid_x", "centroid_y", "force_share_N", "basins"]
ROW_FIELDS = ["pixels", "raw_maxima", "peaks", "peaks_written", "status", "threshold_mm", "separation_mm", "deepest_saddle_mm", "next_prominence_mm"]
LF = {n: i for i, n in enumerate(LOBE_FIELDS)}
RF = {n: i for i, n in enumerate(ROW_FIELDS)}
OK, NO_PIXELS, TRUNCATED = 0, 1, 16
C_FORCE = 8                       # VISTAF_CONTACT_FORCE_N
NAN = float("nan")
# the summed fields of a lobe record and of a split row: float64 sums whose order the definition leaves open
LOBE_SUMMED = ("volume_cm3", "centroid_x", "centroid_y", "force_share_N")
SPLIT_SUMMED = (3, 6, 7, 8)       # VOLUME_CM3, CENTROID_X, CENTROID_Y, FORCE_N
NB8 = [(-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1)]


def clean_depth(depth):
    """float32, a sample that is not finite counts as 0"""
    d = np.array(depth, np.float32)
    d[~np.isfinite(d)] = 0.0
    return d


def lobes_of_mask(m, depth, tau_mm, tau_frac):
    """Steps 1 to 6 on the boolean plane m with the float32 plane `depth` (cleaned).  Returns a dict: maxima (list of (y, x) in descending
    order), prominence / saddle / into per maximum (saddle None for one that never died; into = the maximum of the basin), peaks (list of
    maxima, descending), lobe (int plane: number of the lobe of every pixel, -1 off the mask), lobe_of_max, tau, chain_ended."""
    h, w = m.shape
    pix = [(int(y), int(x)) for y, x in zip(*np.nonzero(m))]

    def key(p):
        return (float(depth[p]), -(p[0] * w + p[1]))
    inside = set(pix)
    up = {}
    for p in pix:
        best = p
        for dx, dy in NB8:
            q = (p[0] + dy, p[1] + dx)
            if q in inside and key(q) > key(best):
                best = q
        up[p] = best
    top = {}
    for p in pix:
        q = p
        while up[q] != q:
            q = up[q]
        top[p] = q
    maxima = sorted((p for p in pix if up[p] == p), key=key, reverse=True)
    passes = []
    for p in pix:
        for dx, dy in NB8:
            q = (p[0] + dy, p[1] + dx)
            if q in inside and top[q] != top[p] and key(q) > key(p):
                passes.append((key(p), key(q), p, q))
    passes.sort(reverse=True)
    parent = {mx: mx for mx in maxima}
    elder = {mx: mx for mx in maxima}

    def find(a):
        while parent[a] != a:
            a = parent[a]
        return a
    saddle, into, prom = {}, {}, {}
    for _, _, lo, hi in passes:
        ra, rb = find(top[lo]), find(top[hi])
        if ra == rb:
            continue
        ea, eb = elder[ra], elder[rb]
        if key(ea) < key(eb):
            dead, other_end, rd, rw = ea, top[hi], ra, rb
        else:
            dead, other_end, rd, rw = eb, top[lo], rb, ra
        saddle[dead], into[dead] = lo, other_end
        prom[dead] = float(depth[dead]) - float(depth[lo])
        parent[rd] = rw
    for mx in maxima:
        if mx not in saddle:
            saddle[mx], into[mx], prom[mx] = None, None, float(depth[mx])
    tau = max(float(tau_mm), float(tau_frac) * float(depth[maxima[0]])) if maxima else NAN
    is_peak = {mx: saddle[mx] is None or prom[mx] > tau for mx in maxima}
    peaks = [mx for mx in maxima if is_peak[mx]]
    number = {mx: j for j, mx in enumerate(peaks)}
    lobe_of_max, ended = {}, True
    for mx in maxima:
        q, steps = mx, 0
        while not is_peak[q] and steps <= len(maxima):
            q, steps = into[q], steps + 1
        ended = ended and is_peak[q]
        lobe_of_max[mx] = number.get(q, -1)
    lobe = np.full((h, w), -1, int)
    for p in pix:
        lobe[p] = lobe_of_max[top[p]]
    return {"maxima": maxima, "prominence": prom, "saddle": saddle, "into": into, "peaks": peaks, "lobe": lobe, "lobe_of_max": lobe_of_max,
            "tau": tau, "chain_ended": ended}


def measure_mask(m, depth, s, force, max_lobes, tau_mm, tau_frac, eps):
    """(row record [12], lobe records [max_lobes, 16], lobe plane int (-1 off the mask, -2 beyond max_lobes), per written lobe a dict with
    what the split table needs)"""
    row, recs = [NAN] * NLOBEROW, np.full((max_lobes, NLOBE), np.nan)
    h, w = m.shape
    if not m.any():
        row[:4] = [0.0] * 4
        row[RF["status"]] = float(NO_PIXELS)
        return row, recs, np.full((h, w), -1, int), []
    r = lobes_of_mask(m, depth, tau_mm, tau_frac)
    peaks, lobe = r["peaks"], r["lobe"]
    s = float(s)
    s2 = s * s
    eps32 = np.float32(eps)
    L = min(len(peaks), max_lobes)
    contact = m & (depth > eps32)
    s_all = 0.0
    for y, x in zip(*np.nonzero(contact)):
        s_all += float(depth[y, x])
    extra = []
    for j in range(L):
        pk = peaks[j]
        mine = lobe == j
        S = SX = SY = 0.0
        ys, xs = np.nonzero(mine & contact)
        for y, x in zip(ys, xs):
            d = float(depth[y, x])
            S += d
            SX += float(x) * d
            SY += float(y) * d
        rec = recs[j]
        rec[LF["x"]], rec[LF["y"]], rec[LF["depth_mm"]], rec[LF["prominence_mm"]] = pk[1], pk[0], float(depth[pk]), r["prominence"][pk]
        sd = r["saddle"][pk]
        if sd is None:
            rec[LF["neighbour"]] = -1.0
        else:
            rec[LF["saddle_x"]], rec[LF["saddle_y"]], rec[LF["saddle_depth_mm"]] = sd[1], sd[0], float(depth[sd])
            rec[LF["neighbour"]] = float(r["lobe_of_max"][r["into"][pk]])
        n_c = len(ys)
        rec[LF["pixels"]], rec[LF["contact_pixels"]], rec[LF["area_mm2"]] = float(mine.sum()), float(n_c), float(n_c) * s2
        rec[LF["volume_cm3"]] = S * s2 / 1000.0
        if n_c:
            rec[LF["centroid_x"]], rec[LF["centroid_y"]] = SX / S, SY / S
        rec[LF["force_share_N"]] = NAN if s_all == 0.0 else float(force) * S / s_all
        rec[LF["basins"]] = float(sum(1 for mx in r["maxima"] if r["lobe_of_max"][mx] == j))
        py, px = np.nonzero(mine)
        extra.append({"S": S, "peak": pk, "box": [int(px.min()), int(py.min()), int(px.max()), int(py.max())]})
    row[RF["pixels"]], row[RF["raw_maxima"]], row[RF["peaks"]], row[RF["peaks_written"]] = float(m.sum()), float(len(r["maxima"])), float(len(peaks)), float(L)
    row[RF["status"]] = float(OK | (TRUNCATED if len(peaks) > max_lobes else 0))
    row[RF["threshold_mm"]] = r["tau"]
    if len(peaks) >= 2:
        dx, dy = peaks[1][1] - peaks[0][1], peaks[1][0] - peaks[0][0]
        row[RF["separation_mm"]] = math.sqrt(float(dx * dx + dy * dy)) * s
    sads = [float(depth[r["saddle"][pk]]) for pk in peaks if r["saddle"][pk] is not None]
    if sads:
        row[RF["deepest_saddle_mm"]] = max(sads)
    rest = [r["prominence"][mx] for mx in r["maxima"] if mx not in set(peaks)]
    if rest:
        row[RF["next_prominence_mm"]] = max(rest)
    plane = np.where(lobe >= max_lobes, -2, lobe)
    return row, recs, plane, extra


def reference(index, contacts, count, mm_per_px, depth, max_lobes=4, tau_mm=0.02, tau_frac=0.1, eps=0.0):
    """{"lobes" [B,K,max_lobes,16], "rows" [B,K,12], "lobe_index" [B,h,w] int8, "split_contacts" [B,K,16], "split_count" [B] int32,
    "split_index" [B,h,w] int8, "split_parent" [B,K,2] int32, "pixels" [B,K]: the pixel count of the parent of every split row (for the
    tolerance of the summed fields)}"""
    B, K = contacts.shape[:2]
    h, w = index.shape[1:]
    lobes, rows = np.full((B, K, max_lobes, NLOBE), np.nan), np.full((B, K, NLOBEROW), np.nan)
    lobe_index = np.full(index.shape, -1, np.int8)
    split, split_count = np.full((B, K, NCONTACT), np.nan), np.zeros(B, np.int32)
    split_index, parent = np.full(index.shape, -1, np.int8), np.full((B, K, 2), -1, np.int32)
    parent_pixels = np.zeros((B, K))
    for b in range(B):
        d = clean_depth(depth[b])
        s = float(mm_per_px[b])
        entries = []
        for k in range(clamp_count(count[b], K)):
            m = row_mask(index[b], contacts[b, k], k)
            rows[b, k], lobes[b, k], plane, extra = measure_mask(m, d, s, contacts[b, k, C_FORCE], max_lobes, tau_mm, tau_frac, eps)
            lobe_index[b][m] = plane[m]
            for j, e in enumerate(extra):
                entries.append(((float(d[e["peak"]]), -(e["peak"][0] * w + e["peak"][1])), k, j, e, m.sum()))
        entries.sort(key=lambda t: t[0], reverse=True)
        split_count[b] = len(entries)
        for r, (_, k, j, e, npx) in enumerate(entries[:K]):
            rec, o = lobes[b, k, j], split[b, r]
            cnt = rec[LF["contact_pixels"]]
            o[0], o[1], o[2] = rec[LF["pixels"]], cnt, rec[LF["area_mm2"]]
            o[3] = float(np.float32(e["S"])) * (s * s) / 1000.0 if cnt > 0 else 0.0
            o[4], o[5] = rec[LF["depth_mm"]], float(e["peak"][0] * w + e["peak"][1])
            o[6], o[7], o[8] = rec[LF["centroid_x"]], rec[LF["centroid_y"]], rec[LF["force_share_N"]]
            o[9:13] = e["box"]
            parent[b, r] = (k, j)
            parent_pixels[b, r] = npx
            split_index[b][(index[b] == k) & (lobe_index[b] == j) & row_mask(index[b], contacts[b, k], k)] = r
    return {"lobes": lobes, "rows": rows, "lobe_index": lobe_index, "split_contacts": split, "split_count": split_count, "split_index": split_index,
            "split_parent": parent, "pixels": parent_pixels}


# ---------------------------------------------------------------------------------------------------------------------------------- scenes
def bumps(h, w, specs, denom):
    """sum of amp * exp(-((x - cx)^2 + (y - cy)^2) / denom) over specs [(amp, cx, cy)], float32"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    return sum(a * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / denom) for a, cx, cy in specs).astype(np.float32)


def two_bumps(h=24, w=40):
    d = bumps(h, w, [(1.0, 12, 12), (0.7, 27, 11)], 30.0)
    return d, d > 0.15


def three_bumps(h=24, w=40):
    d = bumps(h, w, [(1.0, 8, 12), (0.8, 20, 12), (0.6, 32, 12)], 20.0)
    return d, d > 0.1


def grid_depth(h, w):
    """depth 1 on even-even pixels, 0 elsewhere: a quarter of the pixels are maxima"""
    d = np.zeros((h, w), np.float32)
    d[0::2, 0::2] = 1.0
    return d


def disc(h, w, cx, cy, r):
    yy, xx = np.mgrid[0:h, 0:w]
    return (xx - cx) ** 2 + (yy - cy) ** 2 <= r * r


def periodic_depth(h, w, b=0):
    """a fixed field with a maximum every few pixels and many exact ties"""
    yy, xx = np.mgrid[0:h, 0:w]
    return (0.2 + 0.01 * ((7 * xx + 3 * yy + 5 * b) % 11) + 0.02 * ((xx // 5 + 2 * (yy // 4)) % 3) + 0.001 * ((xx * yy) % 7)).astype(np.float32)


def hand_made(h, w):
    """the hand-made frames of the read-out's tests at h x w (at least 24 x 32), K = 8: (names, packed case with its depth planes).  The bump
    fields are laid over the frame's own size; the known numbers of the issue are checked on the 24 x 40 fields in the CPU tests."""
    scenes, names, depths = [], [], []
    yy, xx = np.mgrid[0:h, 0:w]
    base = (0.05 + 0.002 * ((3 * xx + 5 * yy) % 13)).astype(np.float32)

    def add(name, depth):
        names.append(name)
        scenes.append(Scene(h, w))
        depths.append(np.array(depth, np.float32))
        return scenes[-1]
    d = bumps(h, w, [(1.0, 8, 9), (0.7, 21, 8)], 22.0)
    add("two_bumps", d).paint(0, d > 0.15)
    d = bumps(h, w, [(1.0, 5, 12), (0.8, 15, 12), (0.6, 25, 12)], 14.0)
    add("three_bumps", d).paint(0, d > 0.1)
    d = bumps(h, w, [(1.0, 1, 2), (0.9, w - 2, h - 3), (0.5, w - 9, h - 2)], 18.0) + base
    one = np.zeros((h, w), bool)
    one[11, 14] = True
    sc = add("clipped_pixel_empty", d)
    sc.paint(0, rect(h, w, 0, 0, 9, 8)).paint(1, rect(h, w, w - 14, h - 9, w - 1, h - 1)).paint(2, one)
    sc.paint(3, np.zeros((h, w), bool), box=[3, 17, 8, 20])                                    # a row in use without a pixel
    sc.paint(4, rect(h, w, 12, 1, 20, 6), box=[14, 1, 20, 6])                                  # a box that cuts its label
    sc.paint(5, rect(h, w, 0, 10, 7, 14), box=[-5, 9, 7, 1000])                                # a contact on the border whose box leaves the frame
    d = bumps(h, w, [(0.9, 6, 6), (0.6, 14, 7), (0.8, 20, 18)], 16.0) + base
    d[3, 4], d[5, 9], d[17, 19], d[18, 22] = np.nan, np.inf, -np.inf, -0.0
    d[10:14, 2:12] = 0.004                                                                      # below eps
    sc = add("nonfinite_subeps_badbox", d)
    sc.paint(0, rect(h, w, 1, 1, 17, 9)).paint(1, rect(h, w, 15, 14, 26, 21)).paint(2, rect(h, w, 2, 10, 11, 13))
    sc.paint(3, rect(h, w, 20, 2, 28, 8), box=[np.nan, 2, 28, 8])                               # a box that cannot be read
    sc.paint(4, rect(h, w, 1, 16, 9, 21), box=[9, 16, 1, 21])                                   # an inverted box
    add("grid", grid_depth(h, w)).paint(0, np.ones((h, w), bool))
    d = bumps(h, w, [(1.0, 7, 7), (0.9, 22, 15)], 20.0) + base
    flat = disc(h, w, 8, 16, 4)
    d[flat] = 0.5
    sc = add("plateau_and_ring", d)
    sc.paint(0, flat).paint(1, ring(h, w, 22, 9, 7, 3)).paint(2, rect(h, w, 1, 1, 14, 10))
    for name, cnt in (("count_above_K", 11), ("count_zero", 0)):
        d = bumps(h, w, [(1.0, 6, 5), (0.8, 15, 6), (0.7, 12, 17), (0.65, 24, 16)], 12.0) + base
        sc = add(name, d)
        sc.paint(0, rect(h, w, 1, 1, 22, 10)).paint(1, rect(h, w, 5, 12, 30, 21))
        sc.count = cnt
    case = pack(scenes, 0.0731)
    case["depth"] = np.stack(depths)
    rng = np.random.default_rng(5)
    case["tab"][..., C_FORCE] = np.where(np.isnan(case["tab"][..., 0]), np.nan, rng.uniform(0.5, 3.0, case["tab"].shape[:2]))
    return names, case
