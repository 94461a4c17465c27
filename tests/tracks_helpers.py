"""The contact tracker's definition (include/vistaf_track.h) written out in NumPy, and hand-made scenes for tests/test_tracks.py.

`numpy_tracks` follows the header step by step: the exact overlap matrix, best_next / best_prev with ties to the lowest row, mutual links,
the greedy gate stage on float64 d2 = dx*dx + dy*dy, ids in ascending row order.  `scene` turns lists of labelled rectangles into the int8
index planes and contacts tables the tracker reads, so a test states a scene as geometry.
"""
import numpy as np

NCONTACT, NTRACK = 16, 16
FIELDS = ("track_id", "age_frames", "parent_row", "events", "overlap_px", "dx", "dy", "dforce_N", "dvolume_cm3", "origin_track_id")
T = {name: i for i, name in enumerate(FIELDS)}
BORN, SPLIT, MERGED, GATED = 1, 2, 4, 8
C_VOLUME, C_CX, C_CY, C_FORCE = 3, 6, 7, 8          # VISTAF_CONTACT_* indices the tracker reads
NO_ROW = -2 ** 31


def empty_carry(shape, K):
    return {"plane": np.full(shape, -1, np.int8), "rows": np.full((K, NCONTACT), np.nan), "ids": np.zeros(K, np.int64),
            "ages": np.zeros(K, np.int64), "m": 0, "next_id": 0}


def numpy_tracks(index_planes, contacts, counts, K, gate_px, carry=None):
    """index_planes [B,h,w] int8, contacts [B,K,16] float64, counts [B].  Returns (tracks [B,K,16] float64, fate [B,K] int32, carry); pass
    the carry of one call to the next to continue the sequence."""
    index_planes, contacts = np.asarray(index_planes), np.asarray(contacts, dtype=np.float64)
    B = index_planes.shape[0]
    st = empty_carry(index_planes.shape[1:], K) if carry is None else {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in carry.items()}
    tracks = np.full((B, K, NTRACK), np.nan)
    fate = np.full((B, K), NO_ROW, np.int32)
    gate2 = np.float64(gate_px) * np.float64(gate_px)
    for t in range(B):
        prev, cur = st["plane"].ravel().astype(np.int64), index_planes[t].ravel().astype(np.int64)
        prow, crow = st["rows"], contacts[t]
        m, n = st["m"], int(min(max(int(counts[t]), 0), K))
        both = (prev >= 0) & (prev < m) & (cur >= 0) & (cur < n)
        O = np.zeros((K, K), np.int64)
        np.add.at(O, (prev[both], cur[both]), 1)
        best_next = np.array([int(np.argmax(O[i, :n])) if n and O[i, :n].max() > 0 else -1 for i in range(m)], np.int64)       # argmax: first maximum
        best_prev = np.array([int(np.argmax(O[:m, j])) if m and O[:m, j].max() > 0 else -1 for j in range(n)], np.int64)
        parent = np.full(n, -1, np.int64)
        succ = np.full(m, -1, np.int64)
        gated = np.zeros(n, bool)
        for j in range(n):
            i = best_prev[j]
            if i >= 0 and best_next[i] == j:
                parent[j], succ[i] = i, j
        if gate_px > 0:
            ci = [i for i in range(m) if best_next[i] == -1 and np.isfinite(prow[i, C_CX]) and np.isfinite(prow[i, C_CY])]
            cj = [j for j in range(n) if best_prev[j] == -1 and np.isfinite(crow[j, C_CX]) and np.isfinite(crow[j, C_CY])]
            cand = []
            for i in ci:
                for j in cj:
                    dx, dy = crow[j, C_CX] - prow[i, C_CX], crow[j, C_CY] - prow[i, C_CY]
                    d2 = dx * dx + dy * dy
                    if d2 <= gate2:
                        cand.append((d2, i, j))
            cand.sort()
            used_i, used_j = set(), set()
            for d2, i, j in cand:
                if i in used_i or j in used_j:
                    continue
                used_i.add(i)
                used_j.add(j)
                parent[j], succ[i], gated[j] = i, j, True
        for i in range(m):
            fate[t, i] = succ[i] if succ[i] >= 0 else (-(2 + best_next[i]) if best_next[i] >= 0 else -1)
        ids, ages = np.zeros(K, np.int64), np.zeros(K, np.int64)
        for j in range(n):
            row = tracks[t, j]
            ev = 0
            if any(succ[i] < 0 and best_next[i] == j for i in range(m)):
                ev |= MERGED
            row[T["origin_track_id"]] = -1
            if parent[j] >= 0:
                i = parent[j]
                ids[j], ages[j] = st["ids"][i], st["ages"][i] + 1
                ev |= GATED if gated[j] else 0
                row[T["overlap_px"]] = O[i, j]
                row[T["dx"]], row[T["dy"]] = crow[j, C_CX] - prow[i, C_CX], crow[j, C_CY] - prow[i, C_CY]
                row[T["dforce_N"]] = crow[j, C_FORCE] - prow[i, C_FORCE]
                row[T["dvolume_cm3"]] = crow[j, C_VOLUME] - prow[i, C_VOLUME]
            else:
                ids[j], ages[j] = st["next_id"], 0
                st["next_id"] += 1
                ev |= BORN
                row[T["overlap_px"]] = 0
                if best_prev[j] >= 0:
                    ev |= SPLIT
                    row[T["origin_track_id"]] = st["ids"][best_prev[j]]
            row[T["track_id"]], row[T["age_frames"]], row[T["parent_row"]], row[T["events"]] = ids[j], ages[j], parent[j], ev
        st = {"plane": index_planes[t].copy(), "rows": crow.copy(), "ids": ids, "ages": ages, "m": n, "next_id": st["next_id"]}
    return tracks, fate, st


def same_bits(a, b):
    """equal bit for bit where neither is NaN, and NaN in the same places"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.int64)[~na], b.view(np.int64)[~nb]))


def scene(h, w, frames, K, centroids=None):
    """frames: per frame a list of rectangles (x0, y0, x1, y1), inclusive, in table order (row k = k-th rectangle; a later rectangle paints
    over an earlier one).  Returns (planes [B,h,w] int8, contacts [B,K,16], counts [B]): rectangles beyond K are counted but neither drawn
    nor tabled, as vistaf_ftp_contacts truncates.  The table carries what the tracker reads: the centroid (the rectangle's centre, or
    centroids[t][k]; None for NaN), and a volume / force derived from the rectangle so that the differences are not trivial."""
    B = len(frames)
    planes = np.full((B, h, w), -1, np.int8)
    tab = np.full((B, K, NCONTACT), np.nan)
    counts = np.zeros(B, np.int32)
    for t, rects in enumerate(frames):
        counts[t] = len(rects)
        for k, (x0, y0, x1, y1) in enumerate(rects[:K]):
            planes[t, y0:y1 + 1, x0:x1 + 1] = k
            area = (x1 - x0 + 1) * (y1 - y0 + 1)
            tab[t, k, :13] = [area, area, area * 0.01, area * 1.25e-4 + 1e-3 * t, 0.5, y0 * w + x0, (x0 + x1) / 2.0, (y0 + y1) / 2.0,
                              np.sqrt(area) * 0.1 + 0.003 * k, x0, y0, x1, y1]
            if centroids is not None and centroids[t] is not None:
                c = centroids[t][k]
                tab[t, k, C_CX], tab[t, k, C_CY] = (np.nan, np.nan) if c is None else c
    return planes, tab, counts


def random_scene(h, w, B, K, seed, max_rects=6):
    """B frames of random labelled rectangles: a pool of rectangles that drift, appear and vanish, shuffled into a new table order every
    frame (rows swap as they do when one touch gets deeper than another)"""
    rng = np.random.default_rng(seed)
    pool = []
    frames = []
    for t in range(B):
        pool = [(x + int(rng.integers(-3, 4)), y + int(rng.integers(-3, 4)), bw, bh) for (x, y, bw, bh) in pool if rng.random() > 0.12]
        while len(pool) < max_rects and rng.random() < 0.5:
            pool.append((int(rng.integers(0, w - 4)), int(rng.integers(0, h - 4)), int(rng.integers(1, 12)), int(rng.integers(1, 12))))
        if t % 13 == 7:
            pool = []                                                   # an empty frame now and then
        order = rng.permutation(len(pool))
        rects = []
        for k in order:
            x, y, bw, bh = pool[k]
            x0, y0 = min(max(x, 0), w - 1), min(max(y, 0), h - 1)
            rects.append((x0, y0, min(x0 + bw, w - 1), min(y0 + bh, h - 1)))
        frames.append(rects)
    return scene(h, w, frames, K)


MOVING_N, MOVING_B = 224, 12
# noise seed of every frame, 11000 + t + 100 k with the smallest k at which oracle.ftp_oracle keeps exactly two contacts in the frame: in about
# one frame in five of this scene a bridge of noise pixels above the background median joins the two components of the kept mask
MOVING_SEEDS = (11000, 11001, 11002, 11103, 11004, 11005, 11206, 11007, 11008, 11009, 11010, 11311)


def moving_bumps_frames(pkg, n=MOVING_N, count=MOVING_B, start=0, seeds=MOVING_SEEDS):
    """frames start .. start+count-1 of a scene with two Gaussian bumps (contacts_helpers.bumps_phase's phase model) on a ring of radius
    0.6 R around the ROI centre, moving about 2 px per frame in opposite directions; amplitudes 1.1 and 0.8 rad, so the rows never swap by
    themselves, sigma 0.08 n.  Frame t draws its noise from seeds[t]: a frame is the same whatever batch it is generated in."""
    cx, cy, r = pkg.synth.roi_circle(n)
    yy, xx = np.mgrid[0:n, 0:n].astype(np.float64)
    ring, sig = 0.6 * r, 0.08 * n
    frames = []
    for t in range(start, start + count):
        phi = np.zeros((n, n))
        for a0, direction, amp in ((0.2, 1.0, 1.1), (np.pi + 0.2, -1.0, 0.8)):
            ang = a0 + direction * (2.0 / ring) * t
            x0, y0 = cx + ring * np.cos(ang), cy + ring * np.sin(ang)
            phi -= amp * np.exp(-((xx - x0) ** 2 + (yy - y0) ** 2) / (2.0 * sig * sig))
        frames.append(pkg.synth._base(n, phi, np.random.default_rng(seeds[t])))
    return np.stack(frames)
