"""Hard masks and plain CPU references for the mask topology kernels (csrc/k_cc_dist.hip, the blob filter of csrc/k_post.hip): connected
components, the largest component, the closed-form chamfer distances and the per-component peak filter.  NumPy / SciPy only, no GPU: the
tests that use them are in tests/test_mask_kernels.py.  Everything here is integers or float32 bit patterns, so every comparison is exact."""
import numpy as np
from scipy import ndimage

HV, DG, DIST_MAX = 62587, 89738, 0x7fffffff >> 2       # cvRound(0.955 * 65536), cvRound(1.3693 * 65536), cv's DIST_MAX
G_NONE = 1 << 20                                       # row distance of a row without a zero pixel


# =======================================================================================================================================
# references

def ref_labels(mask):
    """int32 plane: the smallest linear index of the 8-connected component of every non-zero pixel, -1 elsewhere"""
    m = np.asarray(mask) != 0
    lab, n = ndimage.label(m, structure=np.ones((3, 3), np.int32))
    out = np.full(m.shape, -1, np.int32)
    if n:
        idx = np.arange(m.size, dtype=np.int64).reshape(m.shape)
        roots = np.asarray(ndimage.minimum(idx, lab, index=np.arange(1, n + 1))).astype(np.int32)
        out[m] = roots[lab[m] - 1]
    return out


def component_count(mask):
    return int(ndimage.label(np.asarray(mask) != 0, structure=np.ones((3, 3), np.int32))[1])


def component_areas(labels):
    """(roots ascending, areas) of a label plane"""
    lab = np.asarray(labels).ravel()
    return np.unique(lab[lab >= 0], return_counts=True)


def ref_largest(labels, and_static=None):
    """uint8 plane (label == winner) & and_static: the largest area wins, on a tie the smallest root; zeros for a frame without a component"""
    labels = np.asarray(labels)
    roots, areas = component_areas(labels)
    if roots.size == 0:
        return np.zeros(labels.shape, np.uint8)
    winner = roots[int(np.argmax(areas))]               # roots ascend and argmax takes the first maximum: the smallest root of a tie
    out = labels == winner
    if and_static is not None:
        out &= np.asarray(and_static).reshape(labels.shape) != 0
    return out.astype(np.uint8)


def blob_threshold(gmax, min_peak, rel_frac):
    """the float32 the peaks are compared with: max(min_peak, rel_frac * gmax) formed in float64, min_peak alone for rel_frac < 0"""
    thr = float(min_peak)
    if rel_frac >= 0.0:
        thr = max(thr, float(rel_frac) * float(np.float32(gmax)))
    return np.float32(thr)


def ref_blob(depth, cand, labels, gmax, min_peak, rel_frac):
    """(kept uint8, depth float32) of one frame: a candidate is kept when the maximum depth of its component reaches the threshold, and the
    depth of the other candidates becomes zero"""
    depth = np.asarray(depth, np.float32)
    labels = np.asarray(labels)
    cand = np.asarray(cand) != 0
    on = labels >= 0
    peak = np.full(depth.size, -np.inf, np.float32)
    np.maximum.at(peak, labels[on], depth[on])
    kept = np.zeros(depth.shape, bool)
    kept[cand] = peak[labels[cand]] >= blob_threshold(gmax, min_peak, rel_frac)
    out = depth.copy()
    out[cand & ~kept] = np.float32(0.0)
    return kept.astype(np.uint8), out


def chamfer_cap_rows(h, cap_px):
    """rows either side of a pixel the closed form looks at (launch_chamfer)"""
    return min(int((cap_px + 2) / 0.955) + 2, h)


def row_distance(zero):
    """horizontal distance of every pixel to the nearest True pixel of its row, G_NONE in a row without one"""
    h, w = zero.shape
    x = np.arange(w, dtype=np.int64)[None, :]
    last = np.maximum.accumulate(np.where(zero, x, -G_NONE), axis=1)
    nxt = np.minimum.accumulate(np.where(zero, x, 2 * G_NONE)[:, ::-1], axis=1)[:, ::-1]
    return np.minimum(np.minimum(x - last, nxt - x), G_NONE)


def closed_form_chamfer(zero, cap_px):
    """What k_chamfer_lds and k_rowdist + k_chamfer_cols compute: the minimum over the rows |dy| <= cap of HV * |g - dy| + DG * min(g, dy),
    g = the row's horizontal distance to its nearest True pixel of `zero`; DIST_MAX where no such row has one.  float32(best) / 65536."""
    zero = np.asarray(zero, bool)
    h, w = zero.shape
    cap = chamfer_cap_rows(h, cap_px)
    g = row_distance(zero)
    best = np.full((h, w), DIST_MAX, np.int64)
    for dy in range(-cap, cap + 1):
        a = abs(dy)
        lo, hi = max(0, -dy), min(h, h - dy)            # rows y with 0 <= y + dy < h
        if lo >= hi:
            continue
        gg = g[lo + dy:hi + dy]
        cost = np.where(gg >= G_NONE, DIST_MAX, HV * np.abs(gg - a) + DG * np.minimum(gg, a))
        best[lo:hi] = np.minimum(best[lo:hi], cost)
    return (best.astype(np.float32) * np.float32(1.0 / 65536.0)).astype(np.float32)


def chamfer_contract(got, ref, cap_px):
    """The promise of the closed-form tiers against the two-pass transform `ref`: the same bits wherever ref <= cap_px + 2, and beyond
    cap_px + 2 and no smaller than ref elsewhere.  Returns (problem or None, pixels in range, pixels out of range)."""
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    inr = ref <= np.float32(cap_px + 2)
    bad_in = inr & (got.view(np.uint32) != ref.view(np.uint32))
    bad_out = ~inr & ~((got > np.float32(cap_px + 2)) & (got >= ref))
    msg = None
    if bad_in.any() or bad_out.any():
        y, x = np.argwhere(bad_in | bad_out)[0]
        msg = "%d in-range and %d out-of-range pixels off, first at (%d, %d): got %r, reference %r" % (
            int(bad_in.sum()), int(bad_out.sum()), y, x, float(got[y, x]), float(ref[y, x]))
    return msg, int(inr.sum()), int((~inr).sum())


# =======================================================================================================================================
# the catalogue

def _walk(h, w, start, occupied, gap):
    """A self-avoiding one-pixel path from `start`, heading right and turning clockwise when it cannot go on.  It steps onto a free pixel n
    when the `gap` pixels behind n in the direction of travel are free (or outside) and no pixel of the 3 x 3 around n is occupied other
    than the two it came from: the path stays `gap` pixels away from what it runs towards and never touches `occupied` or itself."""
    m = np.zeros((h, w), bool)
    occ = occupied.copy()
    y, x = start
    m[y, x] = occ[y, x] = True
    dy, dx = 0, 1
    prev = [(y, x), (y, x)]
    while True:
        for _ in range(2):
            ny, nx = y + dy, x + dx
            ok = 0 <= ny < h and 0 <= nx < w and not occ[ny, nx]
            for k in range(1, gap + 1):
                ay, ax = ny + k * dy, nx + k * dx
                ok = ok and not (0 <= ay < h and 0 <= ax < w and occ[ay, ax])
            if ok:
                for qy in range(max(0, ny - 1), min(h, ny + 2)):
                    for qx in range(max(0, nx - 1), min(w, nx + 2)):
                        ok = ok and (not occ[qy, qx] or (qy, qx) in prev)
            if ok:
                break
            dy, dx = dx, -dy
        else:
            return m
        y, x = ny, nx
        m[y, x] = occ[y, x] = True
        prev = [prev[1], (y, x)]


def spiral(h, w):
    """one-pixel square spiral from the top left corner inwards, one-pixel gaps between its arms"""
    return _walk(h, w, (0, 0), np.zeros((h, w), bool), 1)


def two_spirals(h, w):
    """two interleaved one-pixel spirals: the first with three-pixel gaps, the second along the middle of those gaps"""
    a = _walk(h, w, (0, 0), np.zeros((h, w), bool), 3)
    return a | _walk(h, w, (2, 0), a, 1)


def and_static_plane(h, w):
    """the static plane of the largest-component tests: the right third of the frame is off"""
    a = np.ones((h, w), np.uint8)
    a[:, (2 * w + 2) // 3:] = 0
    return a


BAR_LEN, BAR_STARTS = 130, (0, 1, 63)
DENSITIES = (0.01, 0.41, 0.6, 0.95)                     # 0.41: next to the 8-connected percolation threshold, the most tortuous components
# the number of components a mask is built to have (the tests assert it from the reference); other masks make no such claim
COMPONENTS = {"zeros": 0, "ones": 1, "checker": 1, "comb_joined_last_row": 1, "comb_joined_first_row": 1, "serpentine": 1, "spiral": 1,
              "two_spirals": 2, "interlocked_combs": 2, "tie_equal_areas": 2, "larger_later": 2}


def hard_masks(h, w, seed):
    """name -> uint8 mask [h, w] with non-zero values 1, 2 and 255 mixed (the kernels test != 0).  A mask the shape cannot hold is left out."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    d = {}
    d["zeros"] = np.zeros((h, w), bool)
    d["ones"] = np.ones((h, w), bool)
    m = np.zeros((h, w), bool)
    m[0, 0] = m[0, w - 1] = m[h - 1, 0] = m[h - 1, w - 1] = m[h // 2, w // 2] = True
    d["corners_and_centre"] = m
    if h >= 2 and w >= 2:
        d["checker"] = (yy + xx) % 2 == 0                               # one component through diagonals only
    d["stripes_up_right"] = (xx + yy) % 3 == 0                          # held together by above-right contacts alone
    d["stripes_up_left"] = (xx - yy) % 3 == 0                           # by above-left contacts alone
    if h >= 2 and w >= 3:
        d["comb_joined_last_row"] = (xx % 2 == 0) | (yy == h - 1)       # the root travels through the joining row to every tooth
        d["comb_joined_first_row"] = (xx % 2 == 0) | (yy == 0)
    if h >= 3 and w >= 3:
        # full even rows joined alternately at the last and the first column: one component, a path of about h * w / 2
        d["serpentine"] = (yy % 2 == 0) | ((yy % 4 == 1) & (xx == w - 1)) | ((yy % 4 == 3) & (xx == 0))
    if h >= 5 and w >= 5:
        d["spiral"] = spiral(h, w)
        # teeth from the top at x % 4 == 0 and from the bottom at x % 4 == 2: every wave alternates between two roots
        d["interlocked_combs"] = (yy == 0) | ((xx % 4 == 0) & (yy <= h - 3)) | (yy == h - 1) | ((xx % 4 == 2) & (yy >= 2))
    if h >= 9 and w >= 9:
        d["two_spirals"] = two_spirals(h, w)
    if w >= BAR_STARTS[-1] + BAR_LEN:
        m = np.zeros((h, w), bool)
        for i, x0 in enumerate(BAR_STARTS):                             # runs that cross two 64-pixel boundaries, on rows 0, 2, 4
            if 2 * i < h:
                m[2 * i, x0:x0 + BAR_LEN] = True
        d["bars_130"] = m
    for p in DENSITIES:
        d["random_%g" % p] = rng.random((h, w)) < p
    if h >= 2 and w >= 5:
        # two blobs of equal area: the one with the smaller root (the last column from the top) has its other pixels after the bulk of the
        # second one (the start of row 1) in raster order
        k = min(h, w - 3)
        m = np.zeros((h, w), bool)
        m[:k, w - 1] = True
        m[1, :k] = True
        d["tie_equal_areas"] = m
        # a single pixel first, the larger component later in raster order; and_static_plane cuts the right part of that one
        m = np.zeros((h, w), bool)
        m[0, 0] = True
        m[h - max(1, h // 2):, w - max(2, w // 2):] = True
        d["larger_later"] = m
    vals = np.array([1, 2, 255], np.uint8)[rng.integers(0, 3, (h, w))]
    return {k: (v * vals).astype(np.uint8) for k, v in d.items()}


def chamfer_masks(h, w):
    """name -> uint8 mask: zero pixels where a lookup across 64-pixel words or chunks goes wrong.  A lone zero in a frame of ones (first and
    last column, x = 63, 64, w - 65: the nearest zero of a row is up to seven words away), the complements of the first two for the other
    polarity, a single zero row, a single zero column, and the combs."""
    yy, xx = np.mgrid[0:h, 0:w]
    d = {}
    y0 = h // 2
    for name, x0 in (("first_col", 0), ("last_col", w - 1), ("x63", 63), ("x64", 64), ("w_minus_65", w - 65)):
        if 0 <= x0 < w:
            m = np.ones((h, w), np.uint8)
            m[y0, x0] = 0
            d["lone_zero_" + name] = m
    d["lone_one_first_col"] = (1 - d["lone_zero_first_col"]).astype(np.uint8)
    d["lone_one_last_col"] = (1 - d["lone_zero_last_col"]).astype(np.uint8)
    d["zero_row"] = (yy != h // 3).astype(np.uint8)
    d["zero_col"] = (xx != (2 * w) // 3).astype(np.uint8)
    d["comb_joined_last_row"] = ((xx % 2 == 0) | (yy == h - 1)).astype(np.uint8)
    d["comb_joined_first_row"] = ((xx % 2 == 0) | (yy == 0)).astype(np.uint8)
    return d
