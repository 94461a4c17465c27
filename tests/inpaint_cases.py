"""Hard masks for the Telea inpaint kernels (csrc/k_inpaint*.hip, csrc/telea_common.hpp) and the CPU arithmetic that says which limit each one
crosses.  NumPy / SciPy and the C oracle only, no GPU: tests/test_inpaint_cases.py holds every case to what its name says, and
tests/test_inpaint_direct.py runs them through csrc/test_hooks.h: vistaf_ftp_test_inpaint.

A builder returns (img float32, bad uint8, range): planes [h, w], or [B, h, w] for a batch.  Contract of the hook, which every case keeps: the
image is finite, the mask is zero or non-zero (any non-zero byte is a hole pixel).

The constants below restate the kernels' capacities; tests/test_inpaint_cases.py asserts that each case sits on the side of them it is named for."""
import functools
import zlib

import numpy as np
from scipy import ndimage

from oracle import cvlite

# k_inpaint_win.hip, k_inpaint_mw.hip, k_inpaint.hip, k_inpaint_big.hip
WN_CELLS, WN_QCAP = 14464, 4096             # single-wave window, full size
WN1_CELLS, WN1_QCAP = 10752, 2048           # single-wave window, first tier
MW_CELLS, MW_FILLS, GP_MAXGEN = 10752, 4096, 32
CL2_CELLS = 3072                            # LDS window of one cluster
TQ_CAP = 6144                               # the whole-frame kernel's queue in LDS
LDS_FLAG_CELLS = 57344                      # (h + 2)(w + 2) up to which the whole-frame kernel keeps its two flag planes in LDS
MW_RANGES, CLUSTER_RANGES = (1, 2, 3, 4), (1, 2, 3, 4, 5)
TIE_RANGES = (1, 3, 4, 5, 6, 7, 12)


# =======================================================================================================================================
# mask arithmetic

def holes(bad):
    return np.asarray(bad) != 0


def _or4(m):
    """pixels with a 4-neighbour inside the frame on m"""
    out = np.zeros_like(m)
    out[1:, :] |= m[:-1, :]
    out[:-1, :] |= m[1:, :]
    out[:, 1:] |= m[:, :-1]
    out[:, :-1] |= m[:, 1:]
    return out


def _cheb(m, r):
    return ndimage.binary_dilation(m, structure=np.ones((2 * r + 1, 2 * r + 1), bool))


def band(bad):
    """known pixels 4-adjacent to a hole pixel: the seeds of both passes"""
    hole = holes(bad)
    return ~hole & _or4(hole)


def ring(bad, r):
    """the outside pass's cells: known, off the band, within Chebyshev distance r of a hole pixel (k_telea_prep)"""
    hole = holes(bad)
    return ~hole & ~_or4(hole) & _cheb(hole, r)


def seed_counts(bad, r):
    """live queue entries after the seed phase of the outside pass (ring cells 4-adjacent to the band) and of the march (hole pixels with a
    known 4-neighbour): every one of them is pushed before the first queue pop"""
    hole = holes(bad)
    return int((ring(bad, r) & _or4(band(bad))).sum()), int((hole & _or4(~hole)).sum())


def push_bounds(bad, r):
    """the pushes of a whole pass: every ring cell once, every hole pixel once"""
    return int(ring(bad, r).sum()), int(holes(bad).sum())


def bbox(bad):
    ys, xs = np.nonzero(holes(bad))
    return (int(ys.min()), int(xs.min()), int(ys.max()), int(xs.max())) if ys.size else None


def window_shape(bad, r):
    """the unclipped window of the window kernels: the bounding box of the hole pixels grown by r + 1; None for an empty mask"""
    bb = bbox(bad)
    if bb is None:
        return None
    return bb[2] - bb[0] + 1 + 2 * (r + 1), bb[3] - bb[1] + 1 + 2 * (r + 1)


def window_cells(bad, r):
    s = window_shape(bad, r)
    return 0 if s is None else s[0] * s[1]


def clusters(bad, r):
    """(labels, n): 8-connected components of the hole mask dilated by r + 1 (k_inpaint_cl.hip)"""
    return ndimage.label(_cheb(holes(bad), r + 1), structure=np.ones((3, 3), int))


def cluster_cells(bad, r):
    """window cells of every cluster, as k_cluster_list sizes them"""
    lab, n = clusters(bad, r)
    hole = holes(bad)
    return [window_cells(hole & (lab == i), r) for i in range(1, n + 1)]


def generations(img, bad, r):
    """generations of the 16-wave kernel's two FMM passes (outside pass, march), from the reference's pop log: a generation is every queue
    entry below T_head + 0.70, and whatever its pops push lies above that (k_inpaint_mw.hip), so the sorted pop sequence splits greedily"""
    _, log, tt = cvlite.inpaint_telea_pops(img, bad, float(r))
    out = []
    for p in (0, 1):
        t = tt[(log[:, 0] == p) & (tt > 0)]                 # the seeds (T = 0) are the kernel's generation 0
        n = i = 0
        while i < len(t):
            thr = np.float32(t[i]) + np.float32(0.70)
            n += 1
            while i < len(t) and t[i] < thr:
                i += 1
        out.append(n)
    return tuple(out)


def chebyshev_gap(a, b):
    """smallest Chebyshev distance between a pixel of a and a pixel of b"""
    ya, xa = np.nonzero(a)
    yb, xb = np.nonzero(b)
    return int(np.maximum(np.abs(ya[:, None] - yb[None, :]), np.abs(xa[:, None] - xb[None, :])).min())


# =======================================================================================================================================
# images

def _seed(name):
    return zlib.crc32(name.encode())


def img_random(shape, name):
    """uniform in [-5, 300): no two estimates tie, so any change of the march order changes bits"""
    return np.random.default_rng(_seed(name)).uniform(-5.0, 300.0, shape).astype(np.float32)


def img_u8(shape, name):
    return np.random.default_rng(_seed(name)).integers(0, 256, shape).astype(np.float32)


def _mask(h, w):
    return np.zeros((h, w), np.uint8)


def m_random(h, w, frac, name):
    return (np.random.default_rng(_seed("mask " + name)).random((h, w)) < frac).astype(np.uint8)


def m_checker(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((yy + xx) % 2 == 0).astype(np.uint8)


def m_lattice(h, w, pitch, first, count=None):
    """single pixels at first, first + pitch, ... on both axes (`count` of them per axis, or as many as fit)"""
    m = _mask(h, w)
    ys = np.arange(first, h, pitch)[:count]
    xs = np.arange(first, w, pitch)[:count]
    m[np.ix_(ys, xs)] = 1
    return m


def m_disc(h, w, radius):
    yy, xx = np.mgrid[0:h, 0:w]
    return (((yy - h // 2) ** 2 + (xx - w // 2) ** 2) <= radius * radius).astype(np.uint8)


def m_two_pixels(h, w, bh, bw, y0, x0):
    """two single hole pixels at opposite corners of a bh x bw bounding box: the window size is the only thing that can hand the frame back"""
    m = _mask(h, w)
    m[y0, x0] = 1
    m[y0 + bh - 1, x0 + bw - 1] = 1
    return m


# =======================================================================================================================================
# the cases

_BUILDERS = {}
FAMILY = {}


def _case(family, name):
    def deco(fn):
        _BUILDERS[name] = fn
        FAMILY.setdefault(family, []).append(name)
        return fn
    return deco


def _add(family, name, bad, r, img=None):
    bad = np.ascontiguousarray(bad, np.uint8)
    _BUILDERS[name] = lambda: (img_random(bad.shape, name) if img is None else img(bad.shape, name), bad, r)
    FAMILY.setdefault(family, []).append(name)


def _m_square33():
    m = _mask(80, 80)
    m[23:56, 23:56] = 1
    return m


def _m_plus():
    m = _mask(64, 64)
    m[30:33, 11:52] = 1
    m[11:52, 30:33] = 1
    return m


def _m_diag():
    m = _mask(64, 64)
    i = np.arange(8, 56)
    m[i, i] = 1
    return m


def _m_rowcol():
    m = _mask(48, 56)
    m[20, :] = 1
    m[:, 31] = 1
    return m


for _r in TIE_RANGES:            # ranges 1-4: the 16-wave kernel; up to 6: unrolled ring taps; 7 and up: looped taps
    _add("ties", "square33_r%d" % _r, _m_square33(), _r)
    _add("ties", "plus_r%d" % _r, _m_plus(), _r)
    _add("ties", "diag_r%d" % _r, _m_diag(), _r)
    _add("ties", "rowcol_r%d" % _r, _m_rowcol(), _r)
    _add("ties", "checker96_r%d" % _r, m_checker(96, 96), _r)


def _m_blob5(h, w, y, x):
    m = _mask(h, w)
    m[y:y + 5, x:x + 5] = 1
    return m


_add("ties", "range100_40x40", _m_blob5(40, 40, 17, 18), 100)


def _m_border4():
    m = _mask(64, 200)
    m[:2, :] = m[-2:, :] = 1
    m[:, :2] = m[:, -2:] = 1
    return m


def _m_corners():
    m = _mask(41, 53)           # 2173 pixels: no multiple of 16, the scalar bounding-box pass
    m[:6, :6] = 1
    m[-6:, -6:] = 1
    return m


def _m_lastcol():
    m = _mask(48, 40)
    m[10:31, 36:] = 1
    return m


def _m_allbutone():
    m = np.ones((24, 24), np.uint8)
    m[5, 7] = 0
    return m


_add("borders", "border4_64x200", _m_border4(), 3)
_add("borders", "corners6_41x53", _m_corners(), 3)
_add("borders", "lastcol_48x40", _m_lastcol(), 3)
_add("borders", "allhole_24x24", np.ones((24, 24), np.uint8), 3)
_add("borders", "allbutone_24x24", _m_allbutone(), 3)
_add("borders", "empty_24x24", _mask(24, 24), 3)

# range 3: window = bounding box + 8 either way.  name: (frame, bounding box, window cells, fb of variants 2, 3, 4)
CAPACITY = {
    "cap_88x104": ((96, 112), (88, 104), 10752, (0, 0, 0)),          # 96 * 112 pixels: a multiple of 16, the vector bounding-box pass
    "cap_88x105": ((95, 115), (88, 105), 10848, (1, 1, 0)),          # 10925 pixels: the scalar pass
    "cap_105x120": ((112, 128), (105, 120), 14464, (1, 1, 0)),
    "cap_105x121": ((111, 125), (105, 121), 14577, (1, 1, 1)),
}
for _n, ((_h, _w), (_bh, _bw), _cells, _fb) in CAPACITY.items():
    _add("capacity", _n, m_two_pixels(_h, _w, _bh, _bw, 3, 2), 3)


def _m_column():
    m = _mask(1500, 8)
    m[:, 3] = 1
    return m


_add("capacity", "column_1500x8", _m_column(), 3)              # window 1508 x 9: the row division at ww = 9


def _m_strip_and_corner(w):
    m = _mask(8, w)
    m[2:6, 100:400] = 1          # cluster window 12 x 308 = 3696 cells (> CL2_CELLS): the big-cluster march
    m[:3, -5:] = 1               # cluster window 11 x 13 = 143 cells: an LDS cluster, at the last column of the plane
    return m


# The big-cluster march's plane is the frame padded by r + 1 = 4: pitch w + 8 over 16 rows.  Its outside pass splits a cell into row and column
# with one multiply-high, which is exact while cell * pitch < 2^32: name: (frame width, pitch, exact).  The smallest frames either side of that edge
PLANE_EDGE = {"plane_8x16375": (16375, 16383, True), "plane_8x16376": (16376, 16384, False)}
for _n, (_w, _pitch, _exact) in PLANE_EDGE.items():
    _add("capacity", _n, _m_strip_and_corner(_w), 3)


def _m_lattice3(h, w, n):
    return m_lattice(h, w, 3, 1 + 4, n)


def _m_block(h, w, bh, bw):
    m = _mask(h, w)
    m[4:4 + bh, 4:4 + bw] = 1
    return m


_add("queues", "lattice3_small_48x48", _m_lattice3(48, 48, 10), 3)
_add("queues", "lattice3_band_112x112", _m_lattice3(112, 112, 33), 3)       # 1089 pixels, 4356 band cells (> WN_QCAP) in a window of 105 x 105
_add("queues", "fills4160_80x80", _m_block(80, 80, 65, 64), 3)              # 4160 hole pixels (> MW_FILLS) in a window of 73 x 72
_add("queues", "disc24_96x96", m_disc(96, 96, 24), 3)                       # 31 generations of the march: the last count GP_MAXGEN admits
_add("queues", "disc30_96x96", m_disc(96, 96, 30), 3)                       # 38 generations: beyond it
_add("queues", "disc10_40x40", m_disc(40, 40, 10), 3)
_add("queues", "blob5_32x32", _m_blob5(32, 32, 12, 14), 3)

# the whole-frame kernel's queue: every bounding box is the frame, so no window takes them
_add("dense", "checker_128x128", m_checker(128, 128), 3)
_add("dense", "lattice5_140x140", m_lattice(140, 140, 5, 2), 3)
_add("dense", "lattice5_224x224", m_lattice(224, 224, 5, 2), 3)
_add("dense", "rand3_224x224", m_random(224, 224, 0.03, "rand3"), 3)
_add("dense", "rand30_224x224", m_random(224, 224, 0.30, "rand30"), 3)
_add("dense", "rand10_237x237_r7", m_random(237, 237, 0.10, "rand10a"), 7)    # 239 * 239 = 57121: the last shape whose flags fit LDS
_add("dense", "rand10_237x238_r7", m_random(237, 238, 0.10, "rand10b"), 7)    # 239 * 240 = 57360: flags and queue in global memory

# cluster independence: two 3 x 3 blobs whose nearest hole pixels are d apart (Chebyshev); d = 2 r + 3 is one cluster, 2 r + 4 two
PAIR_PLACES = {"side": (0, 1), "above": (1, 0), "diag": (1, 1)}


def _m_pair(r, d, place):
    dy, dx = PAIR_PLACES[place]
    m = _mask(64, 64)
    m[10:13, 10:13] = 1
    y, x = 10 + dy * (d + 2), 10 + dx * (d + 2)
    m[y:y + 3, x:x + 3] = 1
    return m


PAIRS = {}
for _r in CLUSTER_RANGES:
    for _place in PAIR_PLACES:
        for _d, _ncl in ((2 * _r + 3, 1), (2 * _r + 4, 2)):
            _n = "pair_%s_r%d_d%d" % (_place, _r, _d)
            PAIRS[_n] = (_r, _d, _ncl)
            _add("clusters", _n, _m_pair(_r, _d, _place), _r)


def _m_blob_grid(h, w, r, rows, cols, values=(1,)):
    """3 x 3 blobs whose nearest hole pixels are 2 r + 4 apart: a period of 2 r + 6"""
    m = _mask(h, w)
    p = 2 * r + 6
    for i in range(rows):
        for j in range(cols):
            m[2 + i * p:5 + i * p, 2 + j * p:5 + j * p] = values[(i * cols + j) % len(values)]
    return m


def _m_blob_grid_big():
    m = _m_blob_grid(96, 160, 3, 6, 8)
    m[20, 100:152] = m[71, 100:152] = 1             # a 52 x 52 outline: a window of 60 x 60 = 3600 cells, above CL2_CELLS
    m[20:72, 100] = m[20:72, 151] = 1
    return m


_add("clusters", "blobs42_r1", _m_blob_grid(56, 64, 1, 6, 7), 1)
_add("clusters", "blobs42_r3", _m_blob_grid(80, 96, 3, 6, 7), 3)
_add("clusters", "blobs42_r5", _m_blob_grid(96, 112, 5, 6, 7), 5)
_add("clusters", "blobs42_bytes_r3", _m_blob_grid(80, 96, 3, 6, 7, values=(255, 7)), 3)       # non-zero bytes other than 1
_add("clusters", "blobs48_big_r3", _m_blob_grid_big(), 3)

# image content: a constant image (comes back constant: the constant is a power of two, so that every product w * c and with it the weighted
# mean sum(w c) / sum(w) of equal values is exact in float32), large and small magnitudes, integers 0..255 for the 8-bit path
CONST = np.float32(32.0)
_add("content", "const_96x96", m_random(96, 96, 0.03, "const"), 3, img=lambda s, n: np.full(s, CONST, np.float32))
_add("content", "mag1e4_96x96", m_random(96, 96, 0.03, "mag1e4"), 3, img=lambda s, n: (img_random(s, n) * np.float32(1.0e4 / 300.0)).astype(np.float32))
_add("content", "mag1em3_96x96", m_random(96, 96, 0.03, "mag1em3"), 3, img=lambda s, n: (img_random(s, n) * np.float32(1.0e-3 / 300.0)).astype(np.float32))
U8_CASES = ("u8_rand10_96x96_r7", "u8_checker_128x128_r5", "u8_disc10_40x40_r3")
_add("content", U8_CASES[0], m_random(96, 96, 0.10, "u8a"), 7, img=img_u8)
_add("content", U8_CASES[1], m_checker(128, 128), 5, img=img_u8)
_add("content", U8_CASES[2], m_disc(40, 40, 10), 3, img=img_u8)


@_case("batches", "batch5_64x200")
def _batch5():
    """an empty mask, an all-hole frame, a small blob, a frame the windows hand back (two pixels at opposite corners: 72 x 208 cells) and the
    border frame"""
    two = _mask(64, 200)
    two[0, 0] = two[63, 199] = 1
    bad = np.stack([_mask(64, 200), np.ones((64, 200), np.uint8), _m_blob5(64, 200, 30, 90), two, _m_border4()])
    return img_random(bad.shape, "batch5"), bad, 3


@_case("batches", "batch40_1500x8")
def _batch40():
    """the column case forty times, every second frame an empty mask: more frames than the retry grid's 32 workgroups"""
    bad = np.stack([_m_column() if b % 2 == 0 else _mask(1500, 8) for b in range(40)])
    return img_random(bad.shape, "batch40"), bad, 3


CASE_NAMES = tuple(_BUILDERS)
# the frames every window tier must complete (tests/test_inpaint_direct.py asserts fb == 0 for them)
MUST_COMPLETE = ("blob5_32x32", "disc10_40x40", "corners6_41x53", "square33_r3")


@functools.lru_cache(maxsize=None)
def case(name):
    img, bad, r = _BUILDERS[name]()
    img.setflags(write=False)
    bad.setflags(write=False)
    return img, bad, r


def frames(name):
    """the case as a batch: (img [B, h, w], bad [B, h, w], range)"""
    img, bad, r = case(name)
    return (img[None], bad[None], r) if img.ndim == 2 else (img, bad, r)


def reference_of(img, bad, r, u8=False):
    if u8:
        return cvlite.inpaint_telea_u8(img.astype(np.uint8), bad, float(r)).astype(np.float32)
    return cvlite.inpaint_telea(img, bad, float(r))


@functools.lru_cache(maxsize=None)
def reference(name, u8=False):
    """[B, h, w] float32: cv2.inpaint(TELEA) of every frame (oracle/cvlite.c), computed once"""
    img, bad, r = frames(name)
    out = np.stack([reference_of(img[b], bad[b], r, u8) for b in range(len(img))])
    out.setflags(write=False)
    return out


# the maps of the public temperature entry point: (map float32 with NaNs where missing, radius); the ROI is the whole frame
def temperature_maps():
    out = {}
    for name, (h, w), radius in (("t_rand10_160x160_r7", (160, 160), 7), ("t_rand10_160x160_r5", (160, 160), 5)):
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        m = (30.0 + 6.0 * np.sin(xx / 17.0) * np.cos(yy / 23.0)).astype(np.float32) + img_random((h, w), name) * np.float32(0.01)
        m[m_random(h, w, 0.10, name) != 0] = np.nan
        out[name] = (m.astype(np.float32), radius)
    m = (25.0 + img_random((128, 128), "t_checker") * np.float32(0.05)).astype(np.float32)
    m[m_checker(128, 128) != 0] = np.nan
    out["t_checker_128x128_r7"] = (m, 7)
    return out
