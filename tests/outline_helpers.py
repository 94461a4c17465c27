"""The contact outline read-out (include_ext/vistaf_outline.h) restated in plain Python: a single walker that follows every boundary loop edge
by edge, the hull by a monotone chain over all corners, the calipers by the header's expressions in float64.  Slow and obvious on purpose:
the kernels rank the loops by pointer jumping and build the hull from the row extremes; this does neither."""
import math

import numpy as np

NOUTLINE = 24
FIELDS = ["pixels", "pieces", "holes", "edges", "edges_all", "perimeter_mm", "enclosed_pixels", "corners", "corners_written", "hull_vertices",
          "hull_area_mm2", "solidity", "max_feret_mm", "max_feret_angle_rad", "min_feret_mm", "box_cx", "box_cy", "box_length_mm", "box_width_mm",
          "box_angle_rad"]
O = {n: i for i, n in enumerate(FIELDS)}
INT_FIELDS = ["pixels", "pieces", "holes", "edges", "edges_all", "enclosed_pixels", "corners", "corners_written", "hull_vertices"]
ANGLE_FIELDS = ["max_feret_angle_rad", "box_angle_rad"]
EXACT_DOUBLE_FIELDS = ["perimeter_mm", "hull_area_mm2", "solidity", "max_feret_mm", "min_feret_mm", "box_cx", "box_cy", "box_length_mm", "box_width_mm"]
NCONTACT, C_X0, C_Y0, C_X1, C_Y1 = 16, 9, 10, 11, 12
DX, DY = [1, 0, -1, 0], [0, 1, 0, -1]


# ---------------------------------------------------------------------------------------------------------------------------- the tracer
def fg(m, x, y):
    h, w = m.shape
    return 0 <= x < w and 0 <= y < h and bool(m[y, x])


def right_pixel(x, y, d):
    return [(x, y), (x - 1, y), (x - 1, y - 1), (x, y - 1)][d]


def left_pixel(x, y, d):
    return [(x, y - 1), (x, y), (x - 1, y), (x - 1, y - 1)][d]


def edges(m):
    """every directed boundary edge (x, y, d) of the mask: the pixel on its right is set, the one on its left is not"""
    out = set()
    for y, x in zip(*np.nonzero(m)):
        for d, (sx, sy) in enumerate([(x, y), (x + 1, y), (x + 1, y + 1), (x, y + 1)]):
            assert right_pixel(sx, sy, d) == (x, y)
            if not fg(m, *left_pixel(sx, sy, d)):
                out.add((int(sx), int(sy), d))
    return out


def succ(m, e):
    x, y, d = e
    qx, qy = x + DX[d], y + DY[d]
    if fg(m, *left_pixel(qx, qy, d)):
        nd = (d + 3) % 4
    elif fg(m, *right_pixel(qx, qy, d)):
        nd = d
    else:
        nd = (d + 1) % 4
    return (qx, qy, nd)


def loops(m):
    """the closed loops of the mask, each a list of edges from its first edge in (y, x, d) order; the loops in that order of their first edges"""
    E, seen, out = edges(m), set(), []
    for e in sorted(E, key=lambda t: (t[1], t[0], t[2])):
        if e in seen:
            continue
        L, c = [], e
        while c not in seen:
            assert c in E, (c, e)
            seen.add(c)
            L.append(c)
            c = succ(m, c)
        assert c == e
        out.append(L)
    return out


def area2(L):
    return sum(x * (y + DY[d]) - (x + DX[d]) * y for x, y, d in L)


def corners(L):
    """start vertices of the edges whose predecessor has another direction, from the loop's first edge on"""
    return [(x, y) for i, (x, y, d) in enumerate(L) if L[i - 1][2] != d]


def components(m, conn8):
    from collections import deque
    h, w = m.shape
    lab, n = -np.ones((h, w), int), 0
    nb = [(1, 0), (-1, 0), (0, 1), (0, -1)] + ([(1, 1), (1, -1), (-1, 1), (-1, -1)] if conn8 else [])
    for y in range(h):
        for x in range(w):
            if m[y, x] and lab[y, x] < 0:
                q = deque([(x, y)])
                lab[y, x] = n
                while q:
                    a, b = q.popleft()
                    for dx, dy in nb:
                        u, v = a + dx, b + dy
                        if 0 <= u < w and 0 <= v < h and m[v, u] and lab[v, u] < 0:
                            lab[v, u] = n
                            q.append((u, v))
                n += 1
    return n


# ------------------------------------------------------------------------------------------------------------------------ hull and calipers
def cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def hull(points):
    """strictly convex hull, positive shoelace (the loops' orientation, y down), from the vertex with the smallest (y, x)"""
    pts = sorted(set(points), key=lambda p: (p[1], p[0]))
    if len(pts) < 3:
        return pts

    def chain(seq):
        st = []
        for p in seq:
            while len(st) >= 2 and cross(st[-2], st[-1], p) <= 0:
                st.pop()
            st.append(p)
        return st
    return chain(pts)[:-1] + chain(pts[::-1])[:-1]


def hull_brute(points):
    """the vertex set by exclusion: a point is no vertex when it lies in the closed triangle (or on the closed segment) of three others"""
    pts = sorted(set(points))

    def inside(p, a, b, c):
        s = [cross(a, b, p), cross(b, c, p), cross(c, a, p)]
        if cross(a, b, c) == 0:                      # a degenerate triangle: on the segment spanned by the three
            if any(s):
                return False
            lo = (min(a[0], b[0], c[0]), min(a[1], b[1], c[1]))
            hi = (max(a[0], b[0], c[0]), max(a[1], b[1], c[1]))
            return lo[0] <= p[0] <= hi[0] and lo[1] <= p[1] <= hi[1]
        return all(v >= 0 for v in s) or all(v <= 0 for v in s)
    out = []
    for p in pts:
        rest = [q for q in pts if q != p]
        n = len(rest)
        if not any(inside(p, rest[i], rest[j], rest[k]) for i in range(n) for j in range(i + 1, n) for k in range(j + 1, n)):
            out.append(p)
    return set(out)


def direction(p, q):
    """atan2(p, q) folded into (-pi/2, pi/2]"""
    t = math.atan2(p, q)
    if t <= -math.pi / 2:
        t += math.pi
    elif t > math.pi / 2:
        t -= math.pi
    return t


def edge_measures(H, i):
    """(area, along, across, amin, amax, cmax, L2) of hull edge i, float64 as the header spells them"""
    m = len(H)
    (xi, yi), (xn, yn) = H[i], H[(i + 1) % m]
    ex, ey = xn - xi, yn - yi
    L2 = ex * ex + ey * ey
    a = [(x - xi) * ex + (y - yi) * ey for x, y in H]
    c = [ex * (y - yi) - ey * (x - xi) for x, y in H]
    amin, amax, cmax = min(a), max(a), max(c)
    root = np.sqrt(np.float64(L2))
    area = np.float64(amax - amin) * np.float64(cmax) / np.float64(L2)
    return area, np.float64(amax - amin) / root, np.float64(cmax) / root, amin, amax, cmax, L2


def calipers(H, s):
    """the eight caliper fields of a hull, in the record's order 12..19"""
    s, m = np.float64(s), len(H)
    meas = [edge_measures(H, i) for i in range(m)]
    best = min(range(m), key=lambda i: (meas[i][0], i))
    _, along, across, amin, amax, cmax, L2 = meas[best]
    (xi, yi), (xn, yn) = H[best], H[(best + 1) % m]
    ex, ey = xn - xi, yn - yi
    cx = np.float64(xi) + np.float64(ex * (amin + amax) - ey * cmax) / np.float64(2 * L2)
    cy = np.float64(yi) + np.float64(ey * (amin + amax) + ex * cmax) / np.float64(2 * L2)
    angle = direction(ey, ex) if along >= across else direction(ex, -ey)
    min_feret = min(v[2] for v in meas) * s
    D2, pair = -1, None
    for i in range(m):
        for j in range(i + 1, m):
            d2 = (H[j][0] - H[i][0]) ** 2 + (H[j][1] - H[i][1]) ** 2
            if d2 > D2:
                D2, pair = d2, (i, j)
    i, j = pair
    max_feret = np.sqrt(np.float64(D2)) * s
    feret_angle = direction(H[j][1] - H[i][1], H[j][0] - H[i][0])
    return [max_feret, feret_angle, min_feret, cx, cy, max(along, across) * s, min(along, across) * s, angle]


def calipers_brute(H, s):
    """the same fields with nothing shared but the hull: the box over every edge by projecting on unit vectors, Feret over all pairs"""
    P = np.array(H, dtype=np.float64)
    boxes = []
    for i in range(len(H)):
        e = P[(i + 1) % len(H)] - P[i]
        u = e / np.hypot(*e)
        n = np.array([-u[1], u[0]])
        a, c = (P - P[i]) @ u, (P - P[i]) @ n
        boxes.append(((a.max() - a.min()) * (c.max() - c.min()), a.max() - a.min(), c.max() - c.min()))
    d = np.sqrt(((P[:, None, :] - P[None, :, :]) ** 2).sum(-1))
    return {"area": min(b[0] for b in boxes), "min_feret": min(b[2] for b in boxes) * s, "max_feret": d.max() * s}


# ------------------------------------------------------------------------------------------------------------------------------- the record
def measure_mask(m, s):
    """(record [24], corner list of the principal loop) of one row's pixel mask"""
    rec = np.full(NOUTLINE, np.nan)
    Ls = loops(m)
    A = [area2(L) for L in Ls]
    rec[[0, 1, 2, 3, 4, 7, 8, 9]] = 0
    rec[O["pixels"]] = int(m.sum())
    if not Ls:
        return rec, []
    pos = [i for i, a in enumerate(A) if a > 0]
    rec[O["pieces"]], rec[O["holes"]] = len(pos), sum(a < 0 for a in A)
    rec[O["edges_all"]] = sum(len(L) for L in Ls)
    p = max(pos, key=lambda i: (A[i], -i))                        # loops() lists them by first edge: the earlier wins a tie
    P, cs = Ls[p], corners(Ls[p])
    assert cs[0] == (P[0][0], P[0][1]) and P[0][2] == 0
    rec[O["edges"]], rec[O["perimeter_mm"]], rec[O["enclosed_pixels"]], rec[O["corners"]] = len(P), np.float64(len(P)) * np.float64(s), A[p] // 2, len(cs)
    H = hull([c for i in pos for c in corners(Ls[i])])
    HA2 = sum(H[i][0] * H[(i + 1) % len(H)][1] - H[(i + 1) % len(H)][0] * H[i][1] for i in range(len(H)))
    rec[O["hull_vertices"]] = len(H)
    rec[O["hull_area_mm2"]] = np.float64(HA2) / 2 * np.float64(s) * np.float64(s)
    rec[O["solidity"]] = np.float64(m.sum()) / (np.float64(HA2) / 2)
    rec[12:20] = calipers(H, s)
    return rec, cs


def clamp_count(c, K):
    return min(max(int(c), 0), K)


def row_mask(index, row, k):
    """the pixels of row k: index == k inside the table's box clipped to the frame (csrc/contact_rows.hpp: ContactBox)"""
    h, w = index.shape
    box = [row[C_X0], row[C_Y0], row[C_X1], row[C_Y1]]
    m = np.zeros((h, w), bool)
    if not all(np.isfinite(v) and -1.0e9 <= v <= 1.0e9 for v in box):
        return m
    bx0, by0, bx1, by1 = (int(v) for v in box)
    x0, y0, x1, y1 = max(bx0, 0), max(by0, 0), min(bx1, w - 1), min(by1, h - 1)
    if x1 >= x0 and y1 >= y0:
        m[y0:y1 + 1, x0:x1 + 1] = index[y0:y1 + 1, x0:x1 + 1] == k
    return m


def reference(index, contacts, count, mm_per_px, max_vertices):
    """(outlines [B,K,24], vertices: per frame the list of (x, y) written, offsets [B,K+1]); max_vertices None: no polyline asked for"""
    B, K = contacts.shape[:2]
    out = np.full((B, K, NOUTLINE), np.nan)
    verts, offsets = [], np.zeros((B, K + 1), np.int32)
    for b in range(B):
        total, ok, vb = 0, True, []
        for k in range(K):
            if k < clamp_count(count[b], K):
                rec, cs = measure_mask(row_mask(index[b], contacts[b, k], k), mm_per_px[b])
                total += len(cs)
                ok = ok and max_vertices is not None and total <= max_vertices
                if ok:
                    vb += cs
                    rec[O["corners_written"]] = len(cs)
                out[b, k] = rec
            offsets[b, k + 1] = len(vb)
        verts.append(vb)
    return out, verts, offsets


# ---------------------------------------------------------------------------------------------------------------------------------- scenes
class Scene:
    """an int8 index plane and its table, painted label by label; the box is the painted pixels' unless one is given"""

    def __init__(self, h, w, K=8):
        self.index, self.tab, self.K, self.count = np.full((h, w), -1, np.int8), np.full((K, NCONTACT), np.nan), K, 0

    def paint(self, k, mask, box=None):
        self.index[mask] = k
        ys, xs = np.nonzero(mask)
        self.tab[k] = 0.0
        self.tab[k, C_X0:C_Y1 + 1] = box if box is not None else ([xs.min(), ys.min(), xs.max(), ys.max()] if len(xs) else [0, 0, -1, -1])
        self.count = max(self.count, k + 1)
        return self


def pack(scenes, mpp, counts=None):
    n = len(scenes)
    return {"index": np.stack([s.index for s in scenes]), "tab": np.stack([s.tab for s in scenes]),
            "count": np.array([s.count for s in scenes] if counts is None else counts, np.int32),
            "mpp": np.full(n, mpp, np.float64) if np.isscalar(mpp) else np.asarray(mpp, np.float64), "K": scenes[0].K}


def rect(h, w, x0, y0, x1, y1):
    m = np.zeros((h, w), bool)
    m[y0:y1 + 1, x0:x1 + 1] = True
    return m


def ring(h, w, cx, cy, r_out, r_in):
    yy, xx = np.mgrid[0:h, 0:w]
    d2 = (xx - cx) ** 2 + (yy - cy) ** 2
    return (d2 <= r_out * r_out) & (d2 > r_in * r_in)


def hand_made(h, w):
    """the hand-made frames of the issue at h x w, K = 8: name -> Scene list position.  Returns (names, packed case)"""
    scenes, names = [], []

    def add(name, sc):
        names.append(name)
        scenes.append(sc)
        return sc
    m = np.zeros((h, w), bool)
    m[5, 7] = True
    add("single_pixel", Scene(h, w)).paint(0, m)
    m = np.zeros((h, w), bool)
    for i in range(min(h, w) - 4):
        m[2 + i, 3 + i] = True
    add("diagonal_chain", Scene(h, w)).paint(0, m)
    add("ring", Scene(h, w)).paint(0, ring(h, w, 15, 11, 9, 4))
    m = np.zeros((h, w), bool)
    yy, xx = np.mgrid[0:6, 0:6]
    m[9:15, 4:10] = (xx + yy) % 2 == 0
    add("checkerboard", Scene(h, w)).paint(0, m)
    u = rect(h, w, 3, 2, 20, 18) & ~rect(h, w, 8, 2, 15, 12)
    add("u_shape", Scene(h, w)).paint(0, u)
    add("whole_frame", Scene(h, w)).paint(0, np.ones((h, w), bool))
    sc = add("borders_and_corners", Scene(h, w))
    sc.paint(0, rect(h, w, 0, 0, 2, 1)).paint(1, rect(h, w, w - 3, 0, w - 1, 2)).paint(2, rect(h, w, 0, h - 2, 1, h - 1))
    sc.paint(3, rect(h, w, w - 2, h - 3, w - 1, h - 1)).paint(4, rect(h, w, 10, 0, 14, 0)).paint(5, rect(h, w, 0, 8, 0, 12))
    sc.paint(6, rect(h, w, w - 1, 8, w - 1, 13)).paint(7, rect(h, w, 9, h - 1, 15, h - 1))
    sc = add("touching", Scene(h, w))
    sc.paint(0, rect(h, w, 2, 2, 6, 6)).paint(1, rect(h, w, 7, 7, 11, 10))                 # diagonal touch only
    sc.paint(2, rect(h, w, 14, 3, 18, 9)).paint(3, rect(h, w, 19, 5, 24, 12))              # a shared edge
    sc.paint(4, ring(h, w, 12, 17, 5, 2)).paint(5, rect(h, w, 11, 16, 13, 18))             # one inside the other's hole
    sc = add("two_pieces_and_empty", Scene(h, w))
    sc.paint(0, rect(h, w, 2, 2, 5, 4) | rect(h, w, 12, 9, 20, 15))                        # a label in two pieces
    sc.paint(1, np.zeros((h, w), bool), box=[3, 10, 8, 14])                                # a row whose label has no pixel
    sc.paint(2, rect(h, w, 25, 2, 29, 20), box=[25, 2, 29, 10])                            # a box that cuts its label: the box rules
    sc.paint(3, rect(h, w, 1, 17, 6, 21), box=[-5, 15, 6, 1000])                           # a box that leaves the frame
    sc = add("bad_boxes", Scene(h, w))
    sc.paint(0, rect(h, w, 2, 2, 6, 6), box=[np.nan, 2, 6, 6]).paint(1, rect(h, w, 9, 2, 12, 6), box=[9, 2, np.inf, 6])
    sc.paint(2, rect(h, w, 15, 2, 18, 6), box=[18, 2, 15, 6]).paint(3, rect(h, w, 2, 10, 9, 15))
    for name, cnt in (("count_above_K", 11), ("count_negative", -3), ("count_zero", 0)):
        sc = add(name, Scene(h, w)).paint(0, rect(h, w, 2, 2, 6, 6)).paint(1, ring(h, w, 16, 12, 6, 3))
        sc.count = cnt
    return names, pack(scenes, 0.0731)

