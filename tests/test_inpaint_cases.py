"""CPU side of the direct inpaint tests: every case of tests/inpaint_cases.py keeps the hook's contract, has a finite and repeatable reference, and
sits on the side of each kernel capacity that its name says (so that tests/test_inpaint_direct.py reaches the branch it is about)."""
import numpy as np
import pytest
from scipy import ndimage

import inpaint_cases as C


def _frame(name, b=0):
    img, bad, r = C.frames(name)
    return img[b], bad[b], r


@pytest.mark.parametrize("name", C.CASE_NAMES)
def test_case_keeps_the_contract_and_its_reference_repeats(name):
    img, bad, r = C.frames(name)
    assert img.dtype == np.float32 and bad.dtype == np.uint8 and img.shape == bad.shape and img.ndim == 3
    assert img.shape[1] >= 8 and img.shape[2] >= 8 and 1 <= r <= 100
    assert np.isfinite(img).all(), name                                 # the hook's contract
    u8 = name in C.U8_CASES
    ref = C.reference(name, u8)
    assert ref.shape == img.shape and ref.dtype == np.float32 and np.isfinite(ref).all(), name
    for b in range(min(len(img), 5)):
        again = C.reference_of(img[b], bad[b], r, u8)
        assert np.array_equal(again.view(np.uint32), ref[b].view(np.uint32)), (name, b)
        known = ~C.holes(bad[b])
        assert np.array_equal(ref[b][known].view(np.uint32), img[b][known].view(np.uint32)), (name, b)      # known pixels untouched


def test_every_family_is_there():
    assert set(C.FAMILY) == {"ties", "borders", "capacity", "queues", "dense", "clusters", "content", "batches"}
    assert sum(len(v) for v in C.FAMILY.values()) == len(C.CASE_NAMES) == len(set(C.CASE_NAMES))
    assert len(C.FAMILY["ties"]) == 5 * len(C.TIE_RANGES) + 1 and C.TIE_RANGES == (1, 3, 4, 5, 6, 7, 12)


def test_tie_cases():
    for r in C.TIE_RANGES:
        _, bad, _ = _frame("checker96_r%d" % r)
        out, march = C.seed_counts(bad, r)
        # every known pixel is band: no outside pass at all, and the march's seed phase pushes every hole pixel
        assert (out, march, int(C.holes(bad).sum())) == (0, 4608, 4608)
        assert C.MW_FILLS < 4608 and C.WN_QCAP < march <= C.TQ_CAP
        assert (C.window_cells(bad, r) > C.WN_CELLS) == (r == 12)
        for n in ("square33", "plus", "diag", "rowcol"):
            _, bad, rr = _frame("%s_r%d" % (n, r))
            assert rr == r and C.window_cells(bad, r) <= C.WN1_CELLS and max(C.push_bounds(bad, r)) <= C.WN1_QCAP + 400
    _, bad, _ = _frame("square33_r3")
    assert bad.shape == (80, 80) and C.bbox(bad) == (23, 23, 55, 55) and C.holes(bad).sum() == 33 * 33
    _, bad, _ = _frame("rowcol_r3")
    assert C.holes(bad)[20].all() and C.holes(bad)[:, 31].all() and C.holes(bad).sum() == 48 + 56 - 1
    _, bad, _ = _frame("diag_r3")
    assert (ndimage.label(C.holes(bad))[1], C.holes(bad).sum()) == (48, 48)             # one pixel wide: 4-connected to nothing
    _, bad, r = _frame("range100_40x40")
    assert r == 100 and C.window_cells(bad, r) > C.WN_CELLS and (2 * 101 + 1) ** 2 > C.WN_CELLS       # no window of range 100 ever fits


def test_border_cases():
    _, bad, r = _frame("border4_64x200")
    hole = C.holes(bad)
    assert hole[0].all() and hole[-1].all() and hole[:, 0].all() and hole[:, -1].all() and not hole[2:-2, 2:-2].any()
    assert C.window_shape(bad, r) == (72, 208) and C.window_cells(bad, r) > C.WN_CELLS
    _, bad, r = _frame("corners6_41x53")
    assert bad.size % 16 != 0 and C.holes(bad)[:6, :6].all() and C.holes(bad)[-6:, -6:].all() and C.holes(bad).sum() == 72
    assert C.window_shape(bad, r) == (49, 61)                   # the whole frame and four cells beyond it on every side
    _, bad, r = _frame("lastcol_48x40")
    bb = C.bbox(bad)
    assert bb[3] == 39 and bb[0] > 0 and bb[1] > 0 and bb[2] < 47
    img, bad, r = _frame("allhole_24x24")
    assert C.holes(bad).all() and np.array_equal(C.reference("allhole_24x24")[0], img)          # no band: the reference returns the image
    _, bad, r = _frame("allbutone_24x24")
    assert int((~C.holes(bad)).sum()) == 1 and C.seed_counts(bad, r) == (0, 4)
    assert not C.holes(_frame("empty_24x24")[1]).any()


def test_capacity_cases():
    for name, ((h, w), (bh, bw), cells, fb) in C.CAPACITY.items():
        _, bad, r = _frame(name)
        bb = C.bbox(bad)
        assert bad.shape == (h, w) and r == 3 and C.holes(bad).sum() == 2 and (bb[2] - bb[0] + 1, bb[3] - bb[1] + 1) == (bh, bw)
        assert C.window_shape(bad, r) == (bh + 8, bw + 8) and C.window_cells(bad, r) == cells
        assert fb == (int(cells > C.MW_CELLS), int(cells > C.WN1_CELLS), int(cells > C.WN_CELLS))
    assert [c[2] for c in C.CAPACITY.values()] == [10752, 10848, 14464, 14577]
    assert sorted(h * w % 16 == 0 for (h, w), _, _, _ in C.CAPACITY.values()) == [False, False, True, True]     # both bounding-box passes
    _, bad, r = _frame("column_1500x8")
    assert C.window_shape(bad, r) == (1508, 9) and C.WN1_CELLS < C.window_cells(bad, r) == 13572 <= C.WN_CELLS
    assert C.holes(bad)[:, 3].all() and C.holes(bad).sum() == 1500 and bad.size % 16 == 0
    # the row division of the window kernels at ww = 9: umulhi(li, 2^32 / ww + 1) is li // ww for every cell index the loops form
    li = np.arange(0, 1 << 16, dtype=np.uint64)
    assert np.array_equal((li * np.uint64((1 << 32) // 9 + 1)) >> np.uint64(32), li // np.uint64(9))
    # the big-cluster march's padded plane either side of cell * pitch = 2^32, where its outside pass can no longer split a cell into row and
    # column with one multiply-high
    assert [v[2] for v in C.PLANE_EDGE.values()] == [True, False]
    for name, (w, pitch, exact) in C.PLANE_EDGE.items():
        _, bad, r = _frame(name)
        assert bad.shape == (8, w) and r == 3 and pitch == w + 2 * (r + 1)
        assert (pitch * pitch * (8 + 2 * (r + 1)) < 1 << 32) == exact
        assert C.holes(bad)[2:6, 100:400].all() and C.holes(bad)[:3, -5:].all() and C.holes(bad).sum() == 4 * 300 + 3 * 5
        assert C.cluster_cells(bad, r) == [3696, 143] and 143 <= C.CL2_CELLS < 3696          # the strip: big-cluster march; the corner: an LDS cluster
    assert 16383 * 16383 * 16 < 1 << 32 <= 16384 * 16384 * 16


def test_queue_cases():
    _, bad, r = _frame("lattice3_small_48x48")
    assert C.holes(bad).sum() == 100 and C.band(bad).sum() == 400 and max(C.push_bounds(bad, r)) < C.WN1_QCAP // 2
    _, bad, r = _frame("lattice3_band_112x112")
    out, march = C.seed_counts(bad, r)
    assert C.holes(bad).sum() == 1089 and C.band(bad).sum() == 4356 > C.WN_QCAP and out == 4488 > C.WN_QCAP and march == 1089
    assert C.window_shape(bad, r) == (105, 105) and C.WN1_CELLS < 11025 <= C.WN_CELLS and max(out, march) <= C.TQ_CAP
    _, bad, r = _frame("fills4160_80x80")
    assert C.holes(bad).sum() == 4160 > C.MW_FILLS and C.window_cells(bad, r) == 73 * 72 <= C.MW_CELLS
    # generations of the 16-wave kernel: generation 0 is the seeds, and the pass gives up when a generation beyond number GP_MAXGEN - 1 is due
    for name, want in (("disc24_96x96", (5, 31)), ("disc30_96x96", (5, 38)), ("disc10_40x40", (5, 12))):
        img, bad, r = _frame(name)
        assert C.generations(img, bad, r) == want, name
        assert C.window_cells(bad, r) <= C.WN1_CELLS and C.holes(bad).sum() <= C.MW_FILLS
    assert 12 < 31 <= C.GP_MAXGEN - 1 < 38
    for name in C.MUST_COMPLETE:
        _, bad, r = _frame(name)
        assert r == 3 and C.window_cells(bad, r) <= C.WN1_CELLS and max(C.push_bounds(bad, r)) <= C.WN1_QCAP


# name: hole pixels, live entries after the seed phase of the outside pass and of the march (the regular masks' counts follow from their pitch)
DENSE = {
    "checker_128x128": (8192, 0, 8192),
    "lattice5_140x140": (784, 6272, 784),
    "lattice5_224x224": (2025, 16110, 2025),
    "rand3_224x224": (1552, 9531, 1552),
    "rand30_224x224": (15100, 7930, 14975),
    "rand10_237x237_r7": (5800, 18861, 5799),
    "rand10_237x238_r7": (5621, 18881, 5621),
}


def test_dense_cases_outgrow_the_lds_queue_of_the_whole_frame_kernel():
    assert set(DENSE) == set(C.FAMILY["dense"])
    for name, want in DENSE.items():
        _, bad, r = _frame(name)
        out, march = C.seed_counts(bad, r)
        assert (int(C.holes(bad).sum()), out, march) == want, name
        assert max(out, march) > C.TQ_CAP, name                          # more live entries than the LDS queue holds
        assert C.window_cells(bad, r) > C.WN_CELLS, name                 # no window tier takes the frame
        h, w = bad.shape
        assert ((h + 2) * (w + 2) <= C.LDS_FLAG_CELLS) == (name != "rand10_237x238_r7")
    assert 239 * 239 == 57121 <= C.LDS_FLAG_CELLS < 239 * 240
    _, bad, r = _frame("u8_checker_128x128_r5")
    assert C.seed_counts(bad, r)[1] == 8192 > C.TQ_CAP
    for name, (m, radius) in C.temperature_maps().items():
        assert max(C.seed_counts(~np.isfinite(m), radius)) > C.TQ_CAP, name
        assert np.isfinite(m).any() and 0.05 < np.mean(~np.isfinite(m)) <= 0.5


def test_cluster_cases():
    assert len(C.PAIRS) == 30
    for name, (r, d, ncl) in C.PAIRS.items():
        _, bad, rr = _frame(name)
        lab, n = ndimage.label(C.holes(bad))
        assert rr == r and n == 2 and C.holes(bad).sum() == 18 and d == 2 * r + 2 + ncl
        assert C.chebyshev_gap(lab == 1, lab == 2) == d, name           # the nearest hole pixels of the two blobs
        assert C.clusters(bad, r)[1] == ncl, name
    for name, r in (("blobs42_r1", 1), ("blobs42_r3", 3), ("blobs42_r5", 5), ("blobs42_bytes_r3", 3)):
        _, bad, rr = _frame(name)
        lab, n = ndimage.label(C.holes(bad))
        assert rr == r and n == 42 and C.clusters(bad, r)[1] == 42 and max(C.cluster_cells(bad, r)) <= C.CL2_CELLS
        assert C.chebyshev_gap(lab == 1, lab == 2) == 2 * r + 4 and C.chebyshev_gap(lab == 1, lab == 8) == 2 * r + 4       # right and below
    assert sorted(np.unique(_frame("blobs42_bytes_r3")[1]).tolist()) == [0, 7, 255]
    _, bad, r = _frame("blobs48_big_r3")
    cells = C.cluster_cells(bad, r)
    assert len(cells) == 49 and sorted(cells)[-2:] == [(3 + 8) ** 2, 60 * 60] and 60 * 60 > C.CL2_CELLS


def test_batch_and_content_cases():
    img, bad, r = C.frames("batch5_64x200")
    hole = C.holes(bad)
    assert len(bad) == 5 and not hole[0].any() and hole[1].all() and hole[2].sum() == 25 and hole[3].sum() == 2
    assert C.window_cells(bad[3], r) == 72 * 208 > C.WN_CELLS and np.array_equal(bad[4], C.case("border4_64x200")[1])
    img, bad, r = C.frames("batch40_1500x8")
    assert len(bad) == 40 > 32 and all(C.holes(bad[b]).any() == (b % 2 == 0) for b in range(40))
    assert np.array_equal(bad[0], C.case("column_1500x8")[1]) and len(np.unique(img[::2].reshape(20, -1), axis=0)) == 20
    img, bad, r = _frame("const_96x96")
    assert (img == C.CONST).all() and (C.reference("const_96x96") == C.CONST).all()       # comes back constant
    assert 3e3 < np.abs(_frame("mag1e4_96x96")[0]).max() <= 1.0e4 and 3e-4 < np.abs(_frame("mag1em3_96x96")[0]).max() <= 1.0e-3
    for name in C.U8_CASES:
        img = _frame(name)[0]
        assert np.array_equal(img, np.rint(img)) and img.min() >= 0 and img.max() <= 255
        ref = C.reference(name, True)
        assert np.array_equal(ref, np.rint(ref)) and ref.min() >= 0 and ref.max() <= 255
