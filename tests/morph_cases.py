"""Structuring elements, hard masks and a plain brute-force reference for the binary dilate / erode kernels (launch_morph of csrc/k_basic.hip:
k_morph, k_row_prefix + k_morph_prefix, k_morph_bits).  NumPy only, no GPU: the tests that use them are in tests/test_morph_direct.py.

The reference restates OpenCV's semantics and nothing of the project's: the element is the array cv2.getStructuringElement returns, its anchor
is at (k // 2, k // 2), dilate is the OR (erode the AND) of the mask shifted by every set offset of the element, and a pixel outside the image
is false for the OR and true for the AND (cv::morphologyDefaultBorderValue)."""
import numpy as np

import mask_cases as M

# tiers of vistaf_ftp_test_morph (csrc/test_hooks.h)
DISPATCH, GENERIC, PREFIX, BITS, DISPATCH_NO_SCRATCH = 0, 1, 2, 3, 4

ELLIPSES = (1, 2, 3, 4, 5, 7, 8, 13, 15, 32, 33)
RECTS = ((1, 1), (3, 31), (3, 7), (127, 1), (1, 33), (127, 33), (65, 3), (4, 6))
HOURGLASSES = (3, 7, 13)        # the hook's test element (shape 2): rows that are NOT nested towards the centre, see hourglass()
ELEMENTS = [(0, k, 0) for k in ELLIPSES] + [(1, kx, ky) for kx, ky in RECTS] + [(2, k, 0) for k in HOURGLASSES]       # (shape, kx, ky) as the hook takes them
SHAPES = ((1, 70), (70, 1), (9, 40), (33, 65), (64, 64), (64, 128), (5, 129), (40, 200))


def element_id(e):
    return ("ellipse%d" % e[1]) if e[0] == 0 else ("hourglass%d" % e[1]) if e[0] == 2 else "rect%dx%d" % (e[1], e[2])


def odd_up(k):
    return k if k % 2 else k + 1


def ellipse(k):
    """cv2.getStructuringElement(cv2.MORPH_ELLIPSE, (k, k)) (morph.dispatch.cpp): uint8 [k, k]"""
    r = c = k // 2
    inv_r2 = 1.0 / (r * r) if r else 0.0
    se = np.zeros((k, k), np.uint8)
    for i in range(k):
        dy = i - r
        if abs(dy) <= r:
            dx = int(np.rint(c * np.sqrt((r * r - dy * dy) * inv_r2)))       # cvRound: half to even
            se[i, max(c - dx, 0):min(c + dx + 1, k)] = 1
    return se


def rect(kx, ky):
    """cv2.getStructuringElement(cv2.MORPH_RECT, (kx, ky)): uint8 [ky, kx]"""
    return np.ones((ky, kx), np.uint8)


def hourglass(k):
    """The hook's test element: row i spans |i - k // 2| either side of the anchor.  With an ellipse or a rectangle the rows widen towards the
    centre, so the border pixel that a clamped (replicated) read lands on is under the element anyway and an erosion that wrongly let pixels
    outside the image take part would give the same bits (test_morph_direct.py shows that on the CPU); here it does not."""
    se = np.zeros((k, k), np.uint8)
    for i in range(k):
        a = abs(i - k // 2)
        se[i, k // 2 - a:k // 2 + a + 1] = 1
    return se


def element(e):
    """the array of an ELEMENTS entry; a rectangle's sides are rounded up to odd first, as every caller of the kernels does"""
    shape, kx, ky = e
    return ellipse(kx) if shape == 0 else hourglass(kx) if shape == 2 else rect(odd_up(kx), odd_up(ky))


def symmetric(se):
    """every row of the element is a span centred on the anchor column"""
    ax = se.shape[1] // 2
    return all(np.array_equal(row, row[::-1]) and se.shape[1] == 2 * ax + 1 for row in se)


def bits_take(se, h, w):
    """where the bit-plane kernel applies: spans symmetric about the anchor and at most 63 either side, two planes of the frame within 64 KB"""
    return symmetric(se) and se.shape[1] // 2 <= 63 and h * ((w + 63) // 64) <= 4096


def expected_tier(se, h, w, tier):
    """the kernel the hook reports for `tier`, or None where it must refuse"""
    if tier in (GENERIC, PREFIX):
        return tier
    if tier == BITS:
        return BITS if bits_take(se, h, w) else None
    if bits_take(se, h, w):
        return BITS
    return PREFIX if tier == DISPATCH and se.shape[0] >= 7 else GENERIC


def morph_ref(masks, se, dilate, replicate=False):
    """masks [..., h, w] (non-zero = set) -> uint8 0 / 1 of the same shape.  replicate: NOT the operation; a pixel outside the image takes the
    value of the nearest border pixel instead, which is what a kernel that forgot the border rule on clamped addresses would compute"""
    m = np.asarray(masks) != 0
    h, w = m.shape[-2:]
    ky, kx = se.shape
    ay, ax = ky // 2, kx // 2
    pad = [(0, 0)] * (m.ndim - 2) + [(ay, ky - 1 - ay), (ax, kx - 1 - ax)]
    p = np.pad(m, pad, mode="edge") if replicate else np.pad(m, pad, constant_values=not dilate)
    out = np.zeros(m.shape, bool) if dilate else np.ones(m.shape, bool)
    for i, j in np.argwhere(se != 0):
        # out(y, x) takes src(y + i - ay, x + j - ax), which is p[y + i, x + j]
        s = p[..., i:i + h, j:j + w]
        if dilate:
            out |= s
        else:
            out &= s
    return out.astype(np.uint8)


def masks(h, w, seed=None):
    """name -> uint8 [h, w] with the set pixels drawn from {1, 2, 255}"""
    rng = np.random.default_rng(1000 * h + w if seed is None else seed)
    yy, xx = np.mgrid[0:h, 0:w]
    d = {"zeros": np.zeros((h, w), bool), "ones": np.ones((h, w), bool)}
    m = np.zeros((h, w), bool)
    for y in (0, h // 2, h - 1):
        for x in (0, w // 2, w - 1):
            if (y, x) != (h // 2, w // 2) or min(h, w) == 1:
                m[y, x] = True
    d["corners_and_mid_edges"] = m
    d["border"] = (yy == 0) | (yy == h - 1) | (xx == 0) | (xx == w - 1)
    d["border_off"] = ~d["border"]
    d["checker"] = (yy + xx) % 2 == 0
    for p in (0.02, 0.5, 0.98):
        d["random_%g" % p] = rng.random((h, w)) < p
    d["row_first"], d["row_mid"], d["row_last_off"] = yy == 0, yy == h // 2, yy != h - 1
    d["col_first"], d["col_mid"], d["col_last_off"] = xx == 0, xx == w // 2, xx != w - 1
    vals = np.array([1, 2, 255], np.uint8)[rng.integers(0, 3, (h, w))]
    out = {k: (v * vals).astype(np.uint8) for k, v in d.items()}
    hard = M.hard_masks(h, w, 7 * h + w)
    for k in ("serpentine", "comb_joined_last_row", "stripes_up_right", "bars_130"):
        if k in hard:
            out[k] = hard[k]
    return out


def gates(h, w, B, seed):
    """name -> (and_static [h, w] or None, and_frame [B, h, w] or None): each absent, each present, both present, and all-zero planes"""
    rng = np.random.default_rng(seed)
    vals = np.array([0, 0, 1, 2, 255, 255, 1], np.uint8)
    st, fr = vals[rng.integers(0, 7, (h, w))], vals[rng.integers(0, 7, (B, h, w))]
    return {"none": (None, None), "static": (st, None), "frame": (None, fr), "both": (st, fr), "static_zero": (np.zeros_like(st), None),
            "frame_zero": (None, np.zeros_like(fr)), "both_static_zero": (np.zeros_like(st), fr)}
