"""Inputs and references for the direct tests of the unwrap kernels (tests/test_unwrap_direct.py on the GPU, tests/test_unwrap_cases.py on the
CPU).  Everything here runs on the CPU and imports no torch.

A frame is (wrapped float32, quality float32, mask uint8) from a fixed seed, inside the contract of vistaf_ftp_test_unwrap (csrc/test_hooks.h):
quality finite and >= +0 on the mask, wrapped finite in [-pi, pi].  The references:
  oracle_reference   cvlite.unwrap_quality_guided(want_tree=True): the NaN layout, the wrap counts k = rint((u - w) / 2 pi) and the parents; and
                     the plane the kernels define from those counts, float32(float64(w) + 2 pi k);
  counts_along_tree  the counts a given tree implies under the (-pi, pi] rule of k_unwrap_tree, in float64;
  flood_py           the whole flood in Python (heapq on the reference's tuples) with that rule: the yardstick on the branch cut, where the
                     oracle's atan2f(sinf(d), cosf(d)) on the float32 difference may legitimately choose the other sign.
cut_margin is the condition under which the oracle is the yardstick (>= CUT_MARGIN = 1e-3, 100 times the kernels' own tie band): a condition on
the inputs, not a tolerance.  check_reasons restates, from the reference, why the consistency check of k_unwrap_fast.hip hands a frame to the
flood, so that a test can assert which branch a case reaches."""
import collections
import heapq
import zlib

import numpy as np

from oracle import cvlite

TWO_PI = 2.0 * np.pi
PI32 = np.float32(np.pi)
CUT_MARGIN = 1e-3           # every case compared with the oracle keeps its pixel pairs this far from the branch cut
TIE_BAND = 1e-5             # uf_c of k_unwrap_fast.hip: a pair this close to the cut sends the frame to the flood
K_MAX = 126                 # the check's int8 counts: beyond +-126 (inside a run, or absolute) the frame goes to the flood
LDS_RUNS, LDS_EDGES = 6144, 12288       # k_uf_propagate: tables up to this size are spread in LDS, larger ones in global memory

Frame = collections.namedtuple("Frame", "name wrapped quality mask")


# ---- the launcher's arithmetic, restated ------------------------------------------------------------------------------------------------
def tier_of(h, w, variant=0):
    """UnwrapTier of kernels.hpp: 0 uint16 ranks + batched flood, 1 bitmap flood, 2 generic flood"""
    en = (h + 2) * (w + 2)
    if en <= 65533:
        return 0
    return 1 if en < (1 << 26) and variant != 2 else 2


def run_cap(h):
    return min(60000, max(4096, 8 * h))


def edge_cap(h):
    return min(65000, 2 * run_cap(h))


def rng_of(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


# ---- fields: the true phase in float64, wrapped at the end ---------------------------------------------------------------------------------
def _yx(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return y.astype(np.float64), x.astype(np.float64)


def ramp(h, w, sx, sy, phase0=0.3):
    y, x = _yx(h, w)
    return sx * x + sy * y + phase0


def bump(h, w, amp=7.0, cy=None, cx=None, sigma=None):
    y, x = _yx(h, w)
    cy, cx = (0.45 * h if cy is None else cy), (0.55 * w if cx is None else cx)
    sigma = 0.2 * min(h, w) if sigma is None else sigma
    return amp * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2.0 * sigma * sigma))


def vortex(h, w, cy, cx, charge=1):
    """arctan2 about a half-pixel centre: a residue of that charge in the 2 x 2 block around it"""
    assert cy % 1 == 0.5 and cx % 1 == 0.5
    y, x = _yx(h, w)
    return charge * np.arctan2(y - cy, x - cx)


def quantised(h, w, sx, sy, levels=5):
    step = TWO_PI / levels
    return np.floor(ramp(h, w, sx, sy) / step) * step


def wrap(phi):
    return np.angle(np.exp(1j * phi)).astype(np.float32)


# ---- qualities ------------------------------------------------------------------------------------------------------------------------------
def q_constant(h, w):
    return np.full((h, w), 0.5, np.float32)


def q_two_level(h, w, rng):
    """exactly 0 (an amplitude that underflowed) or 0.75, pixel by pixel"""
    return np.where(rng.random((h, w)) < 0.5, np.float32(0.0), np.float32(0.75)).astype(np.float32)


def q_blob(h, w):
    return bump(h, w, 1.0, 0.5 * h - 0.25, 0.5 * w + 0.25, 0.3 * min(h, w)).astype(np.float32)


def q_plateaus(h, w):
    """integers 0..4"""
    return np.floor(4.999 * q_blob(h, w).astype(np.float64)).astype(np.float32)


def q_random(h, w, rng):
    return rng.random((h, w), dtype=np.float32)


# ---- masks ----------------------------------------------------------------------------------------------------------------------------------
def m_full(h, w):
    return np.ones((h, w), np.uint8)


def m_random(h, w, rng, density=0.8):
    return (rng.random((h, w)) < density).astype(np.uint8)


def m_blobs(h, w):
    """three separate discs, the smallest one last in raster order"""
    y, x = _yx(h, w)
    m = np.zeros((h, w), bool)
    for cy, cx, r in ((0.25 * h, 0.3 * w, 0.2 * min(h, w)), (0.3 * h, 0.78 * w, 0.14 * min(h, w)), (0.8 * h, 0.5 * w, 0.08 * min(h, w))):
        m |= (y - cy) ** 2 + (x - cx) ** 2 <= r * r
    return m.astype(np.uint8)


def smallest_blob_centre(h, w):
    return int(round(0.8 * h)), int(round(0.5 * w))


def m_serpentine(h, w):
    """even rows, joined by the last pixel of rows 1, 5, 9, .. and the first pixel of rows 3, 7, ..: one path, one pixel wide"""
    m = np.zeros((h, w), np.uint8)
    m[0::2] = 1
    m[1::4, w - 1] = 1
    m[3::4, 0] = 1
    if h % 2 == 0:              # the last row is an odd one: keep the path's end on an even row
        m[h - 1] = 0
    return m


def m_comb(h, w, tooth, gap):
    """row 0 is the spine, the teeth hang from it down to the last row"""
    m = np.zeros((h, w), np.uint8)
    m[:, (np.arange(w) % (tooth + gap)) < tooth] = 1
    m[0] = 1
    return m


def m_lattice(h, w):
    """runs of two pixels, shifted by two columns from row to row: every contact between rows is corner to corner"""
    m = np.zeros((h, w), np.uint8)
    c = np.arange(w) % 4
    m[0::2] = (c < 2).astype(np.uint8)
    m[1::2] = (c >= 2).astype(np.uint8)
    return m


def m_spiral(h, w):
    """a one-pixel path winding inwards with one pixel between its arms"""
    m = np.zeros((h, w), np.uint8)

    def free(y, x):
        return 0 <= y < h and 0 <= x < w and not m[y, x]

    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = 1
    while True:
        if not (free(y + dy, x + dx) and (not (0 <= y + 2 * dy < h and 0 <= x + 2 * dx < w) or not m[y + 2 * dy, x + 2 * dx])):
            dy, dx = dx, -dy
            if not (free(y + dy, x + dx) and (not (0 <= y + 2 * dy < h and 0 <= x + 2 * dx < w) or not m[y + 2 * dy, x + 2 * dx])):
                return m
        y, x = y + dy, x + dx
        m[y, x] = 1


def m_boundary_runs(h, w):
    """runs that start, end and cross columns 63 | 64 and 255 | 256 (the lanes and the chunks of the row kernels), with corner-to-corner contacts
    between the rows there; h >= 8"""
    m = np.zeros((h, w), np.uint8)

    def run(y, a, b):
        m[y, max(a, 0):min(b, w - 1) + 1] = 1

    run(0, 0, 63)                                   # ends at 63 ...
    run(1, 64, 255)                                 # ... meets this one corner to corner; it ends at 255 ...
    run(2, 256, w - 1)                              # ... and so does this one, which starts a chunk
    run(3, 60, 70); run(3, 250, 260)                # cross 63 | 64 and 255 | 256
    run(4, 0, w - 1)                                # crosses everything
    run(5, 3, 64); run(5, 66, 255); run(5, 257, w - 1)
    run(6, 63, 63); run(6, 65, 65); run(6, 255, 256); run(6, 0, 20)
    run(7, 0, 63); run(7, 65, 255); run(7, 257, w - 1)
    return m


def m_single(h, w, y, x):
    m = np.zeros((h, w), np.uint8)
    m[y, x] = 1
    return m


def m_empty(h, w):
    return np.zeros((h, w), np.uint8)


def m_row(h, w, y):
    m = np.zeros((h, w), np.uint8)
    m[y] = 1
    return m


# ---- conditions on a frame --------------------------------------------------------------------------------------------------------------------
_PAIRS = ((0, 1), (1, 0), (1, 1), (1, -1))         # right, down, down-right, down-left: every 8-adjacent pair once


def _pair_views(a, dy, dx):
    """(first, second) views of the pairs (y, x) -> (y + dy, x + dx)"""
    h, w = a.shape[:2]
    if dx >= 0:
        return a[:h - dy, :w - dx], a[dy:, dx:]
    return a[:h - dy, -dx:], a[dy:, :w + dx]


def cut_margin(wrapped, mask):
    """the smallest distance from pi (mod 2 pi) of |w[b] - w[a]| over the 8-adjacent pairs of mask pixels; inf without a pair"""
    w64, on = wrapped.astype(np.float64), mask != 0
    best = np.inf
    for dy, dx in _PAIRS:
        a, b = _pair_views(w64, dy, dx)
        ma, mb = _pair_views(on, dy, dx)
        both = ma & mb
        if both.any():
            best = min(best, float(np.abs(np.abs(b - a)[both] % TWO_PI - np.pi).min()))
    return best


def run_edge_counts(mask):
    """(R, E): the horizontal runs of the mask, and the pairs of runs of adjacent rows that touch (8-adjacency), as k_uf_count and k_uf_edges count them"""
    on = mask != 0
    left = np.zeros_like(on)
    left[:, 1:] = on[:, :-1]
    R = int((on & ~left).sum())
    U, D = on[:-1], on[1:]
    Ul, Dl = left[:-1], left[1:]
    both = U & D
    bl = np.zeros_like(both)
    bl[:, 1:] = both[:, :-1]
    E = int((both & ~bl).sum()) + int((Ul & D & ~U & ~Dl).sum()) + int((U & Dl & ~Ul & ~D).sum())
    return R, E


def run_edge_counts_plain(mask):
    """the same from the run intervals themselves, for small masks"""
    runs = []
    for row in mask != 0:
        xs = np.flatnonzero(row)
        cuts = np.flatnonzero(np.diff(xs) > 1) if len(xs) else []
        starts = [xs[0]] + [xs[i + 1] for i in cuts] if len(xs) else []
        ends = [xs[i] for i in cuts] + [xs[-1]] if len(xs) else []
        runs.append(list(zip(starts, ends)))
    E = sum(1 for up, dn in zip(runs[:-1], runs[1:]) for a in up for b in dn if a[0] - 1 <= b[1] and b[0] <= a[1] + 1)
    return sum(len(r) for r in runs), E


def wrap_count(d):
    """the integer n with d + 2 pi n in (-pi, pi]: k_unwrap_tree's float64 arithmetic (rint to even, one correction step)"""
    d = np.asarray(d, np.float64)
    k = -np.rint(d / TWO_PI)
    dd = d + TWO_PI * k
    return np.where(dd <= -np.pi, k + 1.0, np.where(dd > np.pi, k - 1.0, k)).astype(np.int64)


def first_argmax(quality, mask):
    """the seed: the largest quality on the mask, the first such pixel in raster order; -1 on an empty mask"""
    if not (mask != 0).any():
        return -1
    return int(np.argmax(np.where(mask != 0, quality, -np.inf)))


# ---- references -------------------------------------------------------------------------------------------------------------------------------
def plane_from_counts(wrapped, k, nan):
    plane = (wrapped.astype(np.float64) + TWO_PI * k.astype(np.float64)).astype(np.float32)
    plane[nan] = np.nan
    return plane


def tree_depth(parent, order):
    """the largest number of tree edges between a pixel and the seed"""
    flat_par, depth = parent.ravel().tolist(), [0] * parent.size
    best = 0
    for p in np.argsort(order.ravel(), kind="stable")[int((order < 0).sum()):].tolist():
        if flat_par[p] != p:
            depth[p] = depth[flat_par[p]] + 1
            best = max(best, depth[p])
    return best


def counts_along_tree(wrapped, parent, order):
    """the wrap counts the tree `parent` implies under wrap_count, visiting the pixels in pop order (a parent pops before its children)"""
    flat_par = parent.ravel()
    reached = np.flatnonzero(flat_par >= 0)
    inc = np.zeros(parent.size, np.int64)
    w64 = wrapped.ravel().astype(np.float64)
    inc[reached] = wrap_count(w64[reached] - w64[flat_par[reached]])
    inc_l, par_l, k = inc.tolist(), flat_par.tolist(), [0] * parent.size
    for p in reached[np.argsort(order.ravel()[reached], kind="stable")].tolist():
        if par_l[p] != p:
            k[p] = k[par_l[p]] + inc_l[p]
    return np.asarray(k, np.int32).reshape(parent.shape)


def oracle_reference(frame):
    """dict(nan, k, plane, parent, order) from the C oracle, arrays read-only"""
    u, parent, order = cvlite.unwrap_quality_guided(frame.wrapped, frame.mask, frame.quality, want_tree=True)
    nan = np.isnan(u)
    k = np.where(nan, 0.0, np.rint((np.nan_to_num(u).astype(np.float64) - frame.wrapped.astype(np.float64)) / TWO_PI)).astype(np.int32)
    ref = dict(nan=nan, k=k, plane=plane_from_counts(frame.wrapped, k, nan), parent=parent, order=order, u=u)
    for a in ref.values():
        a.setflags(write=False)
    return ref


def rule_reference(frame):
    """as oracle_reference, the counts taken along the oracle's tree (which the wrapped plane does not enter) by wrap_count instead of from the
    oracle's own float32 chain: the reference where a pair sits on the branch cut"""
    u, parent, order = cvlite.unwrap_quality_guided(frame.wrapped, frame.mask, frame.quality, want_tree=True)
    nan = np.isnan(u)
    k = counts_along_tree(frame.wrapped, parent, order)
    ref = dict(nan=nan, k=k, plane=plane_from_counts(frame.wrapped, k, nan), parent=parent, order=order, u=u)
    for a in ref.values():
        a.setflags(write=False)
    return ref


def flood_py(wrapped, quality, mask):
    """(k, nan, parent): the reference's growth loop, literally (heapq on (-q, y, x, py, px)), with wrap_count between a pixel and its parent"""
    h, w = wrapped.shape
    k = np.zeros((h, w), np.int32)
    parent = np.full((h, w), -1, np.int32)
    seed = first_argmax(quality, mask)
    if seed < 0:
        return k, parent < 0, parent
    on, q, w64 = (mask != 0).tolist(), quality.astype(np.float64).tolist(), wrapped.astype(np.float64)
    sy, sx = divmod(seed, w)
    parent[sy, sx] = seed
    heap = []

    def push(py, px):
        for ny in range(max(0, py - 1), min(h, py + 2)):
            for nx in range(max(0, px - 1), min(w, px + 2)):
                if on[ny][nx] and parent[ny, nx] < 0:
                    heapq.heappush(heap, (-q[ny][nx], ny, nx, py, px))

    push(sy, sx)
    while heap:
        _, y, x, py, px = heapq.heappop(heap)
        if parent[y, x] >= 0:
            continue
        parent[y, x] = py * w + px
        k[y, x] = k[py, px] + int(wrap_count(w64[y, x] - w64[py, px]))
        push(y, x)
    return k, parent < 0, parent


def check_reasons(frame, ref):
    """why k_unwrap_fast.hip hands the frame to the flood (the empty set: it settles the frame, need == 0), from the reference `ref`:
    "runs" / "edges"  more runs or run contacts than the check's tables (run_cap, edge_cap);
    "run_k"           a wrap count beyond +-K_MAX relative to the first pixel of a run;
    "abs_k"           a wrap count beyond +-K_MAX relative to the seed, on the seed's component;
    "tie"             a pixel pair within TIE_BAND of the branch cut;
    "residue"         a pair of the seed's component whose counts differ by something else than the wrap between them"""
    h, w = frame.mask.shape
    on, w64 = frame.mask != 0, frame.wrapped.astype(np.float64)
    out = set()
    R, E = run_edge_counts(frame.mask)
    if R > run_cap(h):
        out.add("runs")
    if E > edge_cap(h):
        out.add("edges")
    # along the rows: the running sum of the wraps, less its value at the run's first pixel
    a, b = _pair_views(w64, 0, 1)
    ma, mb = _pair_views(on, 0, 1)
    c = np.zeros((h, w), np.int64)
    c[:, 1:] = np.where(ma & mb, wrap_count(b - a), 0)
    cs = np.cumsum(c, axis=1)
    left = np.zeros_like(on)
    left[:, 1:] = on[:, :-1]
    start = on & ~left
    col = np.where(start, np.arange(w)[None, :], 0)
    first = np.maximum.accumulate(col, axis=1)
    rel = cs - np.take_along_axis(cs, first, axis=1)
    if (np.abs(rel)[on] > K_MAX).any():
        out.add("run_k")
    reached = ~ref["nan"]
    if (np.abs(ref["k"])[reached] > K_MAX).any():
        out.add("abs_k")
    if cut_margin(frame.wrapped, frame.mask) < TIE_BAND:
        out.add("tie")
    k = ref["k"].astype(np.int64)
    for dy, dx in _PAIRS:
        a, b = _pair_views(w64, dy, dx)
        ra, rb = _pair_views(reached, dy, dx)
        ka, kb = _pair_views(k, dy, dx)
        both = ra & rb
        if (both & ((kb - ka != wrap_count(b - a)) | (wrap_count(a - b) != -wrap_count(b - a)))).any():
            out.add("residue")
    return out


# ---- the frames of the cases --------------------------------------------------------------------------------------------------------------------
def _frame(name, phi, quality, mask):
    f = Frame(name, wrap(phi) if phi.dtype == np.float64 else phi, np.ascontiguousarray(quality, np.float32), np.ascontiguousarray(mask, np.uint8))
    for a in f[1:]:
        a.setflags(write=False)
    return f


def centre_vortex(h, w, sx=0.3, sy=0.2):
    return ramp(h, w, sx, sy) + vortex(h, w, h // 2 + 0.5, w // 2 - 0.5)


def frames_ties(h, w):
    """ramp and vortex under constant, two-level and plateau quality, full mask"""
    rng = rng_of("ties%dx%d" % (h, w))
    qs = (("constant", q_constant(h, w)), ("two_level", q_two_level(h, w, rng)), ("plateaus", q_plateaus(h, w)))
    fields = (("ramp", ramp(h, w, 0.9, 1.3)), ("vortex", centre_vortex(h, w)))
    return [_frame("%s_%s" % (fn, qn), phi, q, m_full(h, w)) for fn, phi in fields for qn, q in qs]


def frames_tier_edge(h, w):
    rng = rng_of("edge%dx%d" % (h, w))
    return [_frame("ramp_random", ramp(h, w, 0.8, 0.35), q_random(h, w, rng), m_full(h, w)),
            _frame("vortex_random", centre_vortex(h, w, 0.2, 0.3), q_random(h, w, rng), m_full(h, w))]


def frames_chunks(w, h=8):
    rng = rng_of("chunks%d" % w)
    phi = ramp(h, w, 1.1, 0.7)
    return [_frame("boundary_runs", phi, q_random(h, w, rng), m_boundary_runs(h, w)),
            _frame("full", phi, q_random(h, w, rng), m_full(h, w)),
            _frame("random80", phi, q_random(h, w, rng), m_random(h, w, rng)),
            _frame("one_row", phi, q_random(h, w, rng), m_row(h, w, 4)),
            _frame("quantised", quantised(h, w, 0.31, 0.17), q_random(h, w, rng), m_boundary_runs(h, w))]


def frames_combs(h=800, w=64):
    rng = rng_of("combs")
    phi = ramp(h, w, 0.9, 0.3)
    return [_frame("comb_8_runs", phi, q_random(h, w, rng), m_comb(h, w, 4, 4)),
            _frame("comb_16_runs", phi, q_random(h, w, rng), m_comb(h, w, 2, 2))]


def frames_lattice(h=6000, w=24):
    return [_frame("lattice", ramp(h, w, 0.5, 0.1), q_random(h, w, rng_of("lattice")), m_lattice(h, w))]


def frames_random_mask(h=224, w=224):
    rng = rng_of("random_mask")
    return [_frame("random80", ramp(h, w, 0.9, 1.3) + bump(h, w), q_blob(h, w), m_random(h, w, rng))]


def frames_int8():
    """(frames of 8 x 300, frames of 300 x 64, frames of 8 x 267)"""
    rng = rng_of("int8")
    q = q_random(8, 267, rng).copy()
    q[3, 0] = 2.0                                   # the seed: k falls along the row to -127 at its last pixels, and no further
    qc = q_random(300, 64, rng).copy()
    qc[0, 0] = 2.0                                  # the seed in a corner: the counts run the whole height of the frame
    return ([_frame("rows_3.0", ramp(8, 300, 3.0, 0.0), q_random(8, 300, rng), m_full(8, 300))],
            # (0.5, 2.9): the diagonal step, 3.4, is beyond pi and aliases to -2.88, so the field is inconsistent wherever a diagonal pair meets a
            # vertical one (the frame is handed on for that, and its counts stay small); (0.2, 2.9): every pair below pi, 138 wraps down the frame
            [_frame("cols_aliased", ramp(300, 64, 0.5, 2.9), q_random(300, 64, rng), m_full(300, 64)),
             _frame("cols_2.9", ramp(300, 64, 0.2, 2.9), qc, m_full(300, 64))],
            [_frame("one_row_to_-127", ramp(8, 267, -3.0, 0.0), q, m_row(8, 267, 3))])


def serpentine_vortex(h, w):
    """the ramp is gentle here: at a turn of the path three pixels of a 2 x 2 block are in the mask, and the wraps round that triangle only
    add up to 2 pi (the residue shows) while the ramp's own steps are small"""
    return ramp(h, w, 0.2, 0.1) + vortex(h, w, 0.5, w - 1.5)


def frames_serpentine(h, w):
    rng = rng_of("serp%dx%d" % (h, w))
    q = q_random(h, w, rng).copy()
    q[0, 0] = 2.0                                   # the seed at one end of the path
    m = m_serpentine(h, w)
    out = [_frame("serpentine_ramp", ramp(h, w, 2.9 if w <= 64 else 2.3, 0.2), q, m)]
    if w <= 64:
        # (2.9, 0.4): the diagonal step at a turn, 3.3, is beyond pi and aliases, so the three pixels of a turn contradict one another
        out.append(_frame("serpentine_aliased", ramp(h, w, 2.9, 0.4), q, m))
        out.append(_frame("serpentine_vortex", serpentine_vortex(h, w), q, m))
        out.append(_frame("spiral_ramp", ramp(h, w, 0.7, 0.9), q_two_level(h, w, rng), m_spiral(h, w)))
    return out


def frames_components(h, w):
    rng = rng_of("comp%dx%d" % (h, w))
    phi = ramp(h, w, 0.9, 0.6) + bump(h, w)
    q = (0.5 * q_random(h, w, rng)).astype(np.float32)
    by, bx = smallest_blob_centre(h, w)
    q[by, bx] = 0.9                                 # the best quality sits in the smallest blob: the two larger ones stay NaN
    qlast = q_two_level(h, w, rng).copy()
    qlast[qlast == qlast.max()] = 0.5
    qlast[h - 1, w - 1] = 0.75                      # the seed is the last pixel of the plane
    return [_frame("three_blobs", phi, q, m_blobs(h, w)),
            _frame("single_pixel", phi, q, m_single(h, w, h // 3, w - 1)),
            _frame("empty", phi, q, m_empty(h, w)),
            _frame("seed_last", phi, qlast, m_full(h, w))]


def frames_branch_cut(h, w):
    """two levels, the step across one column: exactly float32(pi), 5e-6 below pi, 1e-4 above pi"""
    rng = rng_of("cut%dx%d" % (h, w))
    out = []
    for name, hi in (("exact", np.float32(-1.0) + PI32), ("5e-6", np.float32(-1.0 + np.pi - 5e-6)), ("1e-4", np.float32(-1.0 + np.pi + 1e-4))):
        wr = np.full((h, w), -1.0, np.float32)
        wr[:, w // 2 + 3:] = hi
        out.append(_frame("cut_" + name, wr, q_random(h, w, rng), m_full(h, w)))
    return out


def m_disc(h, w, frac=0.3):
    y, x = _yx(h, w)
    return ((y - h // 2) ** 2 + (x - w // 2) ** 2 <= (frac * min(h, w)) ** 2).astype(np.uint8)


def frames_mixed(h, w, compact=False):
    """settled, residue, empty mask, more runs than the check's table, settled.  compact: the same on a disc round the vortex and on the upper
    half of the frame, for the frames every pop of which costs a scan of the frontier (the generic flood)"""
    rng = rng_of("mixed%dx%d" % (h, w))
    whole = m_disc(h, w) if compact else m_full(h, w)
    holes = m_random(h, w, rng)
    if compact:
        holes[h // 2:] = 0
    return [_frame("settled_blob", ramp(h, w, 0.9, 1.3), q_blob(h, w), whole),
            _frame("residue", centre_vortex(h, w), q_random(h, w, rng), whole),
            _frame("empty", ramp(h, w, 0.4, 0.2), q_random(h, w, rng), m_empty(h, w)),
            _frame("run_overflow", ramp(h, w, 0.9, 1.3), q_plateaus(h, w), holes),
            _frame("settled_blobs", ramp(h, w, 0.5, 0.7) + bump(h, w), q_blob(h, w), m_blobs(h, w))]


# name -> (frames, need[b] under variant 0, the reason asked of check_reasons per frame: a set it must EQUAL, or a string it must CONTAIN).
# The reference of every case is the oracle, the branch-cut cases apart (RULE_CASES), whose pairs sit on the cut.
Case = collections.namedtuple("Case", "frames need reasons")
_CASES = {}
RULE_CASES = ("cut_64x64", "cut_215x300")
CHUNK_WIDTHS = (63, 64, 65, 255, 256, 257, 513, 600)
NONE = frozenset()


def _build_cases():
    c = {}
    tie_need, tie_why = [0, 0, 0, 1, 1, 1], [NONE] * 3 + [{"residue"}] * 3
    for h, w in ((64, 64), (151, 203), (215, 300), (254, 254)):
        c["ties_%dx%d" % (h, w)] = Case(frames_ties(h, w), tie_need, tie_why)
    for h, w in ((921, 69), (215, 300)):
        c["edge_%dx%d" % (h, w)] = Case(frames_tier_edge(h, w), [0, 1], [NONE, {"residue"}])
    for w in CHUNK_WIDTHS:
        c["chunks_8x%d" % w] = Case(frames_chunks(w), [0] * 5, [NONE] * 5)
    c["combs_800x64"] = Case(frames_combs(), [0, 1], [NONE, {"runs"}])
    c["lattice_6000x24"] = Case(frames_lattice(), [1], [{"edges"}])
    c["random80_224x224"] = Case(frames_random_mask(), [1], ["runs"])
    rows, cols, m127 = frames_int8()
    c["int8_rows_8x300"] = Case(rows, [1], ["run_k"])
    c["int8_cols_300x64"] = Case(cols, [1, 1], [{"residue"}, {"abs_k"}])
    c["int8_m127_8x267"] = Case(m127, [1], ["run_k"])
    c["deep_64x64"] = Case(frames_serpentine(64, 64), [0, 1, 1, 0], [NONE, {"residue"}, {"residue"}, NONE])
    c["deep_254x254"] = Case(frames_serpentine(254, 254), [0], [NONE])
    for h, w in ((64, 64), (215, 300)):
        c["components_%dx%d" % (h, w)] = Case(frames_components(h, w), [0] * 4, [NONE] * 4)
        c["cut_%dx%d" % (h, w)] = Case(frames_branch_cut(h, w), [1, 1, 0], [{"tie"}, {"tie"}, NONE])
    for h, w in ((151, 203), (254, 254)):
        c["mixed_%dx%d" % (h, w)] = Case(frames_mixed(h, w, compact=h > 200), [0, 1, 0, 1, 0], [NONE, {"residue"}, NONE, "runs", NONE])
    return c


CASE_NAMES = (["ties_%dx%d" % s for s in ((64, 64), (151, 203), (215, 300), (254, 254))] + ["edge_921x69", "edge_215x300"] +
              ["chunks_8x%d" % w for w in CHUNK_WIDTHS] +
              ["combs_800x64", "lattice_6000x24", "random80_224x224", "int8_rows_8x300", "int8_cols_300x64", "int8_m127_8x267", "deep_64x64",
               "deep_254x254", "components_64x64", "cut_64x64", "components_215x300", "cut_215x300", "mixed_151x203", "mixed_254x254"])
_REFS = {}


def case(name):
    """the Case `name`; built once, shared, read-only"""
    if not _CASES:
        _CASES.update(_build_cases())
        assert sorted(_CASES) == sorted(CASE_NAMES)
    return _CASES[name]


def references(name):
    """the reference of every frame of the case, computed once"""
    if name not in _REFS:
        _REFS[name] = [(rule_reference if name in RULE_CASES else oracle_reference)(f) for f in case(name).frames]
    return _REFS[name]
