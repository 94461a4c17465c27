"""The Telea inpaint kernels launched directly (csrc/test_hooks.h: vistaf_ftp_test_inpaint, the production launchers on planes of the caller's) on
the masks of tests/inpaint_cases.py: ties in T, holes on the frame's borders, windows either side of each tier's capacity, queues and lists
either side of theirs, masks whose band outgrows the whole-frame kernel's LDS queue, clusters either side of the independence distance, and
batches that mix them.

The reference is oracle/cvlite.inpaint_telea (OpenCV's photo/inpaint.cpp restated) and the bar is the project's own for every Telea tier:
np.array_equal on the whole plane, which also shows that no known pixel was touched.  The 8-bit cases compare with cvlite.inpaint_telea_u8,
cvlite's restatement of OpenCV's uchar path: its docstring says that its parity with OpenCV itself is unpinned (no file of the reference holds
an output of that call), and so it is here -- these tests pin the kernel to the restatement, not to OpenCV.

Variants (test_hooks.h): 0 a session's dispatch, 1 the whole-frame kernel alone, 2 / 3 / 4 one window tier alone (16 waves, single wave at
first-tier capacity, single wave at full size), 5 / 6 the cluster front end with the big-cluster march's queue in LDS / in global memory.
  * variants 0, 1, 5, 6 complete every frame: bits equal to the reference, status 0;
  * variants 2-4, frame by frame: fb == 0 -> bits equal to the reference; fb == 1 -> the plane is bit-identical to the input (a tier that
    hands a frame on has written nothing back);
  * fb is asserted wherever the kernels' constants decide it (derived_fb); where it depends on run-time counts it is only recorded (OBSERVED_FB).

tests/test_inpaint_cases.py asserts on the CPU that each case crosses the limit it is named for."""
import ctypes

import numpy as np
import pytest

import inpaint_cases as C

E_INVALID = -1
UNTOUCHED = -7

# fb where it depends on run-time counts (queue lengths, generations): what the MI355X gave when each case first ran.  An OBSERVATION, not
# an expectation -- the tests print the value and assert only "fb == 0 -> reference, fb == 1 -> input".  name: {variant: fb}; under variants
# 0, 5 and 6, fb == 1 says that the whole-frame kernel took the frame.
#   * the 96 x 96 checkerboard pushes its 4608 hole pixels in the march's seed phase: beyond WN_QCAP = 4096, so the full-size window hands it
#     on, and so does the big-cluster march with its queue in global memory (variant 6), whose slice at this size is 2048 entries;
#   * the 3-pixel lattice has 4488 live entries after the outside pass's seed phase: the same two hand-backs;
#   * the radius-24 disc needs 31 generations of the march, which is the last count the 16-wave kernel admits: it completes; the radius-30
#     disc needs 38;
#   * a frame that is all hole but one pixel is handed on by the 16-wave kernel and completed by every other tier.
OBSERVED_FB = {
    "lattice3_small_48x48": {0: 0, 2: 0, 3: 0, 4: 0, 5: 0, 6: 0},
    "lattice3_band_112x112": {0: 1, 4: 1, 5: 0, 6: 1},
    "fills4160_80x80": {0: 0, 3: 0, 4: 0, 5: 0, 6: 0},
    "disc24_96x96": {0: 0, 2: 0, 3: 0, 4: 0, 5: 0, 6: 0},
    "disc30_96x96": {0: 0, 2: 1, 3: 0, 4: 0, 5: 0, 6: 0},
    "border4_64x200": {5: 0, 6: 0},
    "lastcol_48x40": {0: 0, 2: 0, 3: 0, 4: 0, 5: 0, 6: 0},
    "allhole_24x24": {0: 0, 2: 0, 3: 0, 4: 0, 5: 0, 6: 0},
    "allbutone_24x24": {0: 0, 2: 1, 3: 0, 4: 0, 5: 0, 6: 0},
    "checker96_r1": {0: 1, 3: 1, 4: 1, 5: 0, 6: 1},
    "checker96_r3": {0: 1, 4: 1, 5: 0, 6: 1},
    "checker96_r4": {0: 1, 4: 1, 5: 0, 6: 1},
    "checker96_r5": {0: 1, 4: 1, 5: 0, 6: 1},
    "checker96_r6": {0: 1, 4: 1},
    "checker96_r7": {0: 1, 4: 1},
    "blobs48_big_r3": {0: 0, 4: 0, 5: 0, 6: 0},
    "column_1500x8": {0: 0, 5: 0, 6: 0},
}


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def run_inpaint(pkg, img, bad, r, variant, round_u8=0):
    """planes [B, h, w] -> (inpainted [B, h, w], fb [B], status [B]); fb keeps UNTOUCHED where the variant does not write it"""
    import torch
    n, h, w = img.shape
    d_img, d_bad = _dev(img), _dev(bad)
    fb = torch.full((n,), UNTOUCHED, dtype=torch.int32, device="cuda")
    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    lib = pkg._lib.load()
    rc = lib.vistaf_ftp_test_inpaint(_ptr(d_img), _ptr(d_bad), r, round_u8, _ptr(fb), _ptr(status), n, h, w, variant, None)
    assert rc == 0, (rc, lib.vistaf_ftp_last_error())
    return d_img.cpu().numpy(), fb.cpu().numpy(), status.cpu().numpy()


def variants_for(r, want=(0, 1, 2, 3, 4, 5, 6)):
    return tuple(v for v in want if not (v == 2 and r not in C.MW_RANGES) and not (v in (5, 6) and r not in C.CLUSTER_RANGES))


def derived_fb(name, bad, r, variant):
    """fb[b] of one frame where the kernels' constants decide it, else None"""
    nh, cells = int(C.holes(bad).sum()), C.window_cells(bad, r)
    if variant == 1:
        return UNTOUCHED
    if nh == 0:
        return 0                                                # nothing to inpaint: no tier hands the frame on
    if variant in (0, 4) and cells > C.WN_CELLS:
        return 1                                                # variant 0: no window took it, the whole-frame kernel did
    if variant == 3 and cells > C.WN1_CELLS:
        return 1
    if variant == 2 and (cells > C.MW_CELLS or nh > C.MW_FILLS):
        return 1
    if name in C.CAPACITY and variant in (2, 3, 4):
        return C.CAPACITY[name][3][variant - 2]
    if name == "column_1500x8" and variant == 4:
        return 0                                                # 13572 cells, a band of two columns: the full-size tier completes it
    if name in C.MUST_COMPLETE:
        return 0
    return None


def _same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _diff(got, want):
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    y, x = bad[0]
    return "%d pixels differ, first at (%d, %d): got %r, want %r" % (len(bad), y, x, got[y, x], want[y, x])


def check_planes(name, variant, img, bad, r, ref, out, fb, status, frame_names=None):
    seen_before = OBSERVED_FB.get(name, {}).get(variant)
    print("%s variant %d: fb %s status %s%s" % (name, variant, fb.tolist(), status.tolist(), "" if seen_before is None else " (first observed: %d)" % seen_before))
    assert (status == 0).all(), (name, variant, status.tolist())
    for b in range(len(img)):
        tag = (name, variant, b)
        want_fb = derived_fb(frame_names[b] if frame_names else name, bad[b], r, variant)
        if want_fb is not None:
            assert fb[b] == want_fb, (tag, int(fb[b]), want_fb)
        assert fb[b] in ((0, 1) if variant != 1 else (UNTOUCHED,)), tag
        if variant in (2, 3, 4) and fb[b] == 1:
            assert _same(out[b], img[b]), (tag, "handed on, but written to", _diff(out[b], img[b]))
        else:
            assert _same(out[b], ref[b]), (tag, _diff(out[b], ref[b]))


def check_case(pkg, name, variants=(0, 1, 2, 3, 4, 5, 6)):
    img, bad, r = C.frames(name)
    ref = C.reference(name)
    seen = {}
    for variant in variants_for(r, variants):
        out, fb, status = run_inpaint(pkg, img, bad, r, variant)
        check_planes(name, variant, img, bad, r, ref, out, fb, status)
        seen[variant] = fb
    return seen


# ---- ties in T: the stable queue's order through every tier, ranges on both sides of the 16-wave kernel and of the unrolled ring taps ----------
@pytest.mark.gpu
@pytest.mark.parametrize("name", C.FAMILY["ties"])
def test_ties_pop_in_the_stable_queue_order(pkg, name):
    check_case(pkg, name)


# ---- the frame's borders: the unclipped window's BORDER cells, OpenCV's index shifts at the first and last row and column ------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", C.FAMILY["borders"])
def test_holes_on_the_frame_borders(pkg, name):
    check_case(pkg, name)


# ---- window capacity: two hole pixels, so that the window's size is the only reason for a hand-back -----------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", C.FAMILY["capacity"])
def test_windows_either_side_of_each_tiers_capacity(pkg, name):
    if name in C.PLANE_EDGE:                                    # the padded plane of the big-cluster march either side of cell * pitch = 2^32
        check_case(pkg, name, (1, 5, 6))
        return
    seen = check_case(pkg, name)
    if name in C.CAPACITY:
        assert tuple(int(seen[v][0]) for v in (2, 3, 4)) == C.CAPACITY[name][3]
        assert seen[0][0] == C.CAPACITY[name][3][2]             # a session: the full-size retry takes what variant 4 takes


# ---- queue and list capacity --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", C.FAMILY["queues"])
def test_queues_and_lists_either_side_of_their_capacity(pkg, name):
    check_case(pkg, name)


# ---- the whole-frame kernel's queue -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", C.FAMILY["dense"])
def test_dense_masks_through_the_whole_frame_kernel(pkg, name):
    """more live queue entries than TQ_CAP = 6144 (tests/test_inpaint_cases.py: DENSE): the kernel has to take its queue to global memory and
    still complete the frame, through a session's dispatch, on its own, and behind the cluster front end"""
    seen = check_case(pkg, name, (0, 1, 5, 6))
    assert seen[0][0] == 1                                       # no window took the frame: the whole-frame kernel did


# ---- cluster independence -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", C.FAMILY["clusters"])
def test_clusters_either_side_of_the_independence_distance(pkg, name):
    """blobs 2 r + 3 apart (one cluster) and 2 r + 4 apart (two): marched apart they give the bits of the one queue of the reference"""
    check_case(pkg, name)


# ---- image content -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", C.FAMILY["content"])
def test_image_content(pkg, name):
    check_case(pkg, name)
    img, bad, r = C.frames(name)
    if name == "const_96x96":
        assert (run_inpaint(pkg, img, bad, r, 0)[0] == C.CONST).all()
    if name in C.U8_CASES:                                       # the temperature path: 8-bit semantics, cvlite's restatement of OpenCV's uchar path
        out, fb, status = run_inpaint(pkg, img, bad, r, 1, round_u8=1)
        ref = C.reference(name, True)
        print("%s round_u8: status %s" % (name, status.tolist()))
        assert (status == 0).all() and (fb == UNTOUCHED).all()
        assert _same(out[0], ref[0]), (name, _diff(out[0], ref[0]))


# ---- batches ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_mixed_batch_equals_its_frames_run_alone(pkg):
    """an empty mask, an all-hole frame, a small blob, a frame the windows hand back and the border frame in one launch"""
    name = "batch5_64x200"
    img, bad, r = C.frames(name)
    ref = C.reference(name)
    frame_names = [None, None, "blob5_32x32", None, None]       # the small blob must complete in every window tier, here too
    for variant in variants_for(r):
        out, fb, status = run_inpaint(pkg, img, bad, r, variant)
        check_planes(name, variant, img, bad, r, ref, out, fb, status, frame_names)
        for b in range(len(img)):
            o1, fb1, st1 = run_inpaint(pkg, img[b:b + 1], bad[b:b + 1], r, variant)
            assert _same(o1[0], out[b]) and fb1[0] == fb[b] and st1[0] == 0, (name, variant, b)


@pytest.mark.gpu
def test_batch_beyond_the_retry_grid(pkg):
    """forty frames, every second one an empty mask, the others the 1508 x 9 window that only the full-size tier takes: a session's retry grid of
    32 workgroups strides over the batch"""
    name = "batch40_1500x8"
    img, bad, r = C.frames(name)
    ref = C.reference(name)
    for variant in (0, 4):
        out, fb, status = run_inpaint(pkg, img, bad, r, variant)
        check_planes(name, variant, img, bad, r, ref, out, fb, status, ["column_1500x8"] * 40)
        assert (fb == 0).all()


# ---- every tier completes frames of its own ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("variant", (2, 3, 4, 5, 6))
def test_every_tier_completes_named_cases_itself(pkg, variant):
    """so that "fb == 1 -> untouched" is never all a tier is held to: the small blob, the radius-10 disc, the corner holes and the 33 x 33 square
    complete under every variant without a hand-back"""
    assert len(C.MUST_COMPLETE) >= 3
    for name in C.MUST_COMPLETE:
        img, bad, r = C.frames(name)
        out, fb, status = run_inpaint(pkg, img, bad, r, variant)
        assert fb[0] == 0 and status[0] == 0 and _same(out[0], C.reference(name)[0]), (name, variant, fb.tolist())
        assert not _same(out[0], img[0])


# ---- the public temperature entry point --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(C.temperature_maps()))
def test_temperature_map_with_scattered_missing_pixels(pkg, name):
    """inpaint_temperature_map over a whole-frame ROI whose missing pixels are scattered: the whole-frame kernel with more live queue entries than
    its LDS queue holds, where a user meets it.  Equal to the oracle restatement, NaN for NaN"""
    from oracle import temp_oracle as T
    m, radius = C.temperature_maps()[name]
    roi = np.ones(m.shape, bool)
    want = T.inpaint_temperature_map(m, roi, radius)
    got = pkg.tempseg.inpaint_temperature_map(m, roi, radius)
    assert np.isfinite(want).all()
    assert np.array_equal(got, want, equal_nan=True), "%d pixels differ, %d not finite" % (int((got != want).sum()), int((~np.isfinite(got)).sum()))


# ---- the hook's argument checks (no GPU needed: a refused call makes no HIP call) ------------------------------------------------------------------------------
def test_inpaint_hook_refuses_bad_arguments(pkg):
    lib = pkg._lib.load()
    buf = [np.zeros(256, np.int32) for _ in range(4)]
    p = [ctypes.c_void_p(b.ctypes.data) for b in buf]

    def call(img=p[0], bad=p[1], fb=p[2], status=p[3], r=3, u8=0, B=1, h=8, w=8, variant=0):
        return lib.vistaf_ftp_test_inpaint(img, bad, r, u8, fb, status, B, h, w, variant, None)

    for kw in (dict(img=None), dict(bad=None), dict(fb=None), dict(status=None), dict(B=0), dict(B=-2), dict(h=7), dict(w=7), dict(h=0), dict(w=-3),
               dict(r=0), dict(r=101), dict(r=-1), dict(variant=-1), dict(variant=7), dict(h=65536, w=65536)):
        assert call(**kw) == E_INVALID, kw
    for variant in (0, 2, 3, 4, 5, 6):                          # 8-bit semantics: the whole-frame kernel alone
        assert call(u8=1, variant=variant) == E_INVALID, variant
    for r in (5, 6, 100):                                       # the 16-wave kernel takes ranges 1..4
        assert call(r=r, variant=2) == E_INVALID, r
    for r in (6, 7, 100):                                       # the cluster kernels take ranges 1..5
        assert call(r=r, variant=5) == E_INVALID and call(r=r, variant=6) == E_INVALID, r
    assert lib.vistaf_ftp_last_error()
