"""CPU references and inputs for the three binary-mask chains of a predict (csrc/k_maskchain.hip against the separate kernels): the bad-pixel
mask, the reliable mask and the contact / background masks.  The references restate oracle/ftp_oracle.py (detect_bad_pixels :223-237,
compute_reliable_mask :364-384, the contact block of process_frame :751-766) on planes of the caller, with oracle/cvlite.py for the
morphology, the labelling and the distance transform.  NumPy only, no GPU: the tests are in tests/test_mask_chains.py.  Everything is a mask,
a count or a float32 bit pattern, so every comparison is exact."""
import numpy as np

import mask_cases as M
from oracle import cvlite as cv

# where the bit-plane code can go wrong: one word per row (9 x 40, 64 x 64), a single valid bit in the last word (33 x 65), several words with
# a partial last one (96 x 80: 16 columns)
SMALL_SHAPES = [(9, 40), (64, 64), (33, 65), (96, 80)]
# structuring elements 3, 5, 7, 15 with 1 and 2 iterations, the chamfer-ball margins 1 and 6 (and none)
COMBOS = [(3, 1, 1), (3, 2, 6), (5, 1, 0), (5, 2, 1), (7, 1, 6), (7, 2, 1), (15, 1, 1), (15, 2, 6)]


def disc(h, w, inset=1):
    """the static plane (roi / valid): an ellipse that leaves the frame's corners and a border of `inset` pixels out"""
    yy, xx = np.mgrid[0:h, 0:w]
    ry, rx = max(1.0, h / 2 - inset), max(1.0, w / 2 - inset)
    return ((((yy - (h - 1) / 2) / ry) ** 2 + ((xx - (w - 1) / 2) / rx) ** 2) <= 1.0).astype(np.uint8)


def field_from_mask(mask, thr, rng, sprinkle=True):
    """float32 plane that is >= thr exactly on `mask`, some pixels equal to thr, with NaN, +inf and -inf sprinkled on both sides of it
    (sprinkle: the thresholded field is then no longer `mask` itself)"""
    on = np.asarray(mask) != 0
    mag = rng.random(on.shape).astype(np.float32) * np.float32(3.0)
    f = np.where(on, np.float32(thr) + mag, np.float32(thr) - mag - np.float32(0.125)).astype(np.float32)
    f[on & (rng.random(on.shape) < 0.05)] = np.float32(thr)
    r = rng.random(on.shape) if sprinkle else np.ones(on.shape)
    f[r < 0.01] = np.nan
    f[(r >= 0.01) & (r < 0.02)] = np.inf
    f[(r >= 0.02) & (r < 0.03)] = -np.inf
    return f


def se_of(ksize, force_odd=True):
    return cv.ellipse_se(max(3, int(ksize) | 1) if force_odd else int(ksize))


# =======================================================================================================================================
# references

def ref_bad(img, grad, valid, hi, g, ksize, iters):
    """(bad1 uint8, count)"""
    with np.errstate(invalid="ignore"):
        bad = ((img >= np.float32(hi)) | (grad >= np.float32(g))) & (valid != 0)
    if ksize > 1:
        bad = cv.dilate(bad.astype(np.uint8) * 255, se_of(ksize), int(iters)) > 0
    return bad.astype(np.uint8), int(bad.sum())


def ref_reliable(q, roi, thr, ksize, iters, margin, status_in):
    """(rel0 uint8, reliable uint8, count, status, facts) -- facts: what the largest-component step saw, for the tests' own claims"""
    roi = roi != 0
    with np.errstate(invalid="ignore"):
        rel = roi & (q >= np.float32(thr)) & np.isfinite(q)
    rel0 = rel.copy()
    facts = {"areas": np.zeros(0, np.int64), "roots": np.zeros(0, np.int64), "before_erosion": 0}
    if rel.any():
        rel = (cv.morph_close(rel.astype(np.uint8) * 255, se_of(ksize), int(iters)) > 0) & roi
    if rel.any():
        num, labels, areas = cv.cc8(rel)
        lab = M.ref_labels(rel)
        facts["roots"], facts["areas"] = M.component_areas(lab)
        if num > 1:
            best = 1 + int(np.argmax(areas[1:]))
            # OpenCV's labels ascend in raster order of the first pixel: the first maximum is the smallest root
            assert np.array_equal(labels == best, M.ref_largest(lab) != 0)
            rel = (labels == best) & roi
    facts["before_erosion"] = int(rel.sum())
    if margin > 0 and rel.any():
        rel = (cv.dist_l2_3x3(rel.astype(np.uint8) * 255) > float(margin)) & rel
    cnt = int(rel.sum())
    status = 1 if (cnt == 0 and status_in == 0) else int(status_in)
    return rel0.astype(np.uint8), rel.astype(np.uint8), cnt, status, facts


def ref_contact(res, rel, t3, rel_count, min_frac, max_frac, ksize, iters):
    """(thr_used float32, contact_d uint8, background uint8, bg_count, branch) -- branch: 'nonfinite' is added to 'in' / 'min' / 'max'"""
    rel = rel != 0
    t3 = np.asarray(t3, np.float32)
    absr = np.abs(res).astype(np.float32)

    def mask_at(t):
        with np.errstate(invalid="ignore"):
            return (absr >= np.float32(t)) & rel & np.isfinite(absr)
    thr = t3[0]
    branch = []
    if not np.isfinite(thr):
        thr = t3[1]
        branch.append("nonfinite")
    frac = float(mask_at(thr).sum()) / float(max(1, int(rel_count)))
    if frac < min_frac:
        branch.append("min")
        if np.isfinite(t3[1]):
            thr = t3[1]
    elif frac > max_frac:
        branch.append("max")
        if np.isfinite(t3[2]):
            thr = t3[2]
    else:
        branch.append("in")
    contact = mask_at(thr)
    cd = contact
    if iters > 0:
        cd = cv.dilate(contact.astype(np.uint8) * 255, se_of(ksize, False), int(iters)) > 0
    cd = cd & rel
    bg = rel & ~cd
    bgc = int(bg.sum())
    if bgc < int(0.15 * int(rel_count)):
        bg = rel.copy()
        branch.append("bg_fallback")
    return np.float32(thr), cd.astype(np.uint8), bg.astype(np.uint8), bgc, branch


# =======================================================================================================================================
# inputs

_CAT = {}


def catalogue(h, w):
    """name -> 0 / 1 mask of M.hard_masks plus two of this module's: computed once per shape, shared, never written to"""
    if (h, w) not in _CAT:
        cat = {k: (m != 0).astype(np.uint8) for k, m in M.hard_masks(h, w, 77 * h + w).items()}
        if h >= 9 and w >= 36:
            # two squares of equal area far apart (a closing leaves a square as it is): the one met first in raster order must win
            m = np.zeros((h, w), np.uint8)
            m[1:4, w - 6:w - 3] = 1
            m[h - 4:h - 1, 3:6] = 1
            cat["two_equal_squares"] = m
        for m in cat.values():
            m.setflags(write=False)
        _CAT[(h, w)] = cat
    return _CAT[(h, w)]


def big_masks(h, w, seed):
    """three masks for the one large case of each chain: next to the percolation threshold, diagonal contacts only, a comb"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    return {"random_0.41": (rng.random((h, w)) < 0.41).astype(np.uint8), "checker": ((yy + xx) % 2 == 0).astype(np.uint8),
            "comb_joined_last_row": ((xx % 2 == 0) | (yy == h - 1)).astype(np.uint8)}


def batches(names, n=3):
    names = list(names)
    out = [names[i:i + n] for i in range(0, len(names), n)]
    out[-1] = (out[-1] + names)[:n]
    return out
