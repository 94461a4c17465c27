"""The unwrap kernels launched directly (csrc/test_hooks.h: vistaf_ftp_test_unwrap, the production launch_unwrap on planes of the caller's) on the
frames of tests/unwrap_cases.py: ties in quality, masks of many runs, holes, corridors and components, runs across the lane and chunk
boundaries of the row kernels, wrap counts beyond int8, trees as deep as the mask, pixel pairs on the branch cut, batches that mix settled,
flooded and empty frames, and the two sides of the uint16 rank range.

Every case runs under variant 0 (as a session: the consistency check first), 1 (the floods only) and 2 (the bitmap flood hands every frame to
the generic one) and asserts, per frame, against the CPU oracle (tests/unwrap_cases.py: oracle_reference; rule_reference on the branch cut):
the tier the launcher reports, need[b], a zero status, the NaN layout and the wrap counts exactly, the plane within one float32 ulp of
float32(float64(w) + 2 pi k), the parents exactly wherever a flood grew the frame (and an untouched parent plane where the check settled it),
and the three variants' planes bit for bit.  tests/test_unwrap_cases.py asserts on the CPU that each case is what its name says (run and edge
counts, largest count, tree depth, distance from the branch cut, why the check hands it on).

Where a case differs from what a first reading of the kernels suggests:
  * a ramp of (2.9, 0.4) or (0.5, 2.9) rad / pixel steps by more than pi along one diagonal, which aliases: such a field contradicts itself
    wherever a diagonal pair meets a vertical one, the check hands it on for THAT (need == 1, also on the serpentine, whose turns hold three
    pixels of a 2 x 2 block), and its counts stay small.  The cases keep those ramps and add (2.9, 0.2) and (0.2, 2.9), below pi on every
    pair, for "deep and settled" and for "absolute count beyond 126";
  * more run contacts than the edge table (E > ecap) with no more runs than the run table cannot happen at 800 x 64: two adjacent rows of a and
    b runs touch in at most a + b - 1 pairs, so E <= 2 R - (h - 1) < 2 rcap = ecap.  It takes ecap's own ceiling of 65000, i.e. h > 4062: the
    case is a 6000 x 24 lattice of two-pixel runs that meet corner to corner (R = 36000 <= 48000, E = 65989);
  * an empty mask is settled by the check (nothing on it contradicts): need == 0, as the hook's comment states;
  * the masks of more pixels than the bitmap flood holds (1 228 800) are left to variant 2, which takes the same hand-back path on masks that
    do fit: a full mask of 1120 x 1120 under variant 1, timed once on the MI355X, took 9.7 s in the launch alone (1.25 million dependent pops
    on one wave of the generic flood; layout, counts and parents equal to the oracle's), which with its reference is past 10 s for one test.
  * the largest batch of floods on one wave, mixed_254x254, keeps its full-frame masks to a disc and to the upper half of the frame: every pop
    of the generic flood scans the frontier, and the case is about the per-frame skips and strides, not about the size of a flood."""
import ctypes

import numpy as np
import pytest

import unwrap_cases as U

E_INVALID = -1
UNTOUCHED = -7
# the flood of each shape: 0 uint16 ranks + batched flood ((h + 2)(w + 2) <= 65533: 921 x 69 is the last such frame), 1 bitmap flood (215 x 300,
# 65534, is the first); under variant 2 the frames of tier 1 report 2, the generic flood
SHAPE_TIER = {(64, 64): 0, (151, 203): 0, (224, 224): 0, (921, 69): 0, (800, 64): 0, (300, 64): 0, (8, 300): 0, (8, 267): 0,
              (215, 300): 1, (254, 254): 1, (6000, 24): 1}
SHAPE_TIER.update({(8, w): 0 for w in U.CHUNK_WIDTHS})


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def run_unwrap(pkg, frames, variant):
    """frames -> (unwrapped [B, h, w], parent, need [B], status [B], tier); the planes the hook does not write keep UNTOUCHED"""
    import torch
    n = len(frames)
    h, w = frames[0].mask.shape
    dw, dq, dm = (_dev(np.stack([getattr(f, k) for f in frames])) for k in ("wrapped", "quality", "mask"))
    uw = torch.full((n, h, w), float(UNTOUCHED), dtype=torch.float32, device="cuda")
    par = torch.full((n, h, w), UNTOUCHED, dtype=torch.int32, device="cuda")
    need = torch.full((n,), UNTOUCHED, dtype=torch.int32, device="cuda")
    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    lib = pkg._lib.load()
    tier = lib.vistaf_ftp_test_unwrap(_ptr(dw), _ptr(dq), _ptr(dm), _ptr(uw), _ptr(par), _ptr(need), _ptr(status), n, h, w, variant, None)
    assert tier >= 0, lib.vistaf_ftp_last_error()
    return uw.cpu().numpy(), par.cpu().numpy(), need.cpu().numpy(), status.cpu().numpy(), tier


def _first_diff(got, want):
    bad = np.argwhere(got != want)
    y, x = bad[0]
    return "%d pixels differ, first at (%d, %d): got %r, want %r" % (len(bad), y, x, got[y, x], want[y, x])


def assert_frame(tag, frame, ref, uw, par, flooded):
    nan = np.isnan(uw)
    assert np.array_equal(nan, ref["nan"]), (tag, "NaN layout", _first_diff(nan, ref["nan"]))
    k = np.where(nan, 0.0, np.rint((np.nan_to_num(uw).astype(np.float64) - frame.wrapped.astype(np.float64)) / U.TWO_PI)).astype(np.int32)
    assert np.array_equal(k, ref["k"]), (tag, "wrap counts", _first_diff(k, ref["k"]))
    want = ref["plane"]
    err = np.abs(uw.astype(np.float64) - want.astype(np.float64))[~nan]
    ulp = np.spacing(np.abs(want[~nan])).astype(np.float64)
    assert (err <= ulp).all(), (tag, "plane", float((err / ulp).max()))
    if flooded:
        assert np.array_equal(par, ref["parent"]), (tag, "parents", _first_diff(par, ref["parent"]))
    else:                                           # the check settled the frame: no flood ran, the parent plane is as it was passed
        assert (par == UNTOUCHED).all(), tag


def check_case(pkg, name, variants=(0, 1, 2)):
    c, refs = U.case(name), U.references(name)
    h, w = c.frames[0].mask.shape
    planes = {}
    for variant in variants:
        uw, par, need, status, tier = run_unwrap(pkg, c.frames, variant)
        want_tier = 2 if variant == 2 and SHAPE_TIER[(h, w)] == 1 else SHAPE_TIER[(h, w)]
        print("%s variant %d: tier %d need %s" % (name, variant, tier, need.tolist()))
        assert tier == want_tier, (name, variant, tier, want_tier)
        assert (status == 0).all(), (name, variant, status)
        if variant == 0:
            assert need.tolist() == list(c.need), (name, need.tolist(), c.need)
        else:
            assert (need == UNTOUCHED).all(), (name, variant)
        for b, (f, r) in enumerate(zip(c.frames, refs)):
            assert_frame((name, f.name, variant), f, r, uw[b], par[b], variant != 0 or need[b] == 1)
        planes[variant] = uw
    for v in variants[1:]:
        assert np.array_equal(planes[v].view(np.uint32), planes[variants[0]].view(np.uint32)), (name, v)
    return planes


# ---- ties in quality: the heap order (-q, y, x, py, px) through every tier ---------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ties_64x64", "ties_151x203", "ties_215x300", "ties_254x254"])
def test_ties_in_quality_follow_the_heap_order(pkg, name):
    """constant, two-level (exact zeros) and plateau quality: on the ramps the order shows in the parents, on the vortices it decides the plane
    (need == 1 there, from the case table)"""
    c = U.case(name)
    assert [f.name.split("_")[0] for f in c.frames] == ["ramp"] * 3 + ["vortex"] * 3 and list(c.need) == [0, 0, 0, 1, 1, 1]
    for f in c.frames:
        assert len(np.unique(f.quality)) <= 5                  # ties, and nothing but ties
    check_case(pkg, name)


# ---- the two sides of the uint16 rank range ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["edge_921x69", "edge_215x300"])
def test_last_uint16_frame_and_first_bitmap_frame(pkg, name):
    h, w = U.case(name).frames[0].mask.shape
    assert (h + 2) * (w + 2) == (65533 if name == "edge_921x69" else 65534)
    check_case(pkg, name)


# ---- lanes and chunks of the row kernels ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("w", U.CHUNK_WIDTHS)
def test_runs_across_lane_and_chunk_boundaries_settle(pkg, w):
    """h = 8: runs that start, end and cross columns 63 | 64 and 255 | 256 and touch corner to corner there, on residue-free fields with wraps
    inside the runs: the check settles every frame (need == 0) and its plane is the flood's"""
    assert list(U.case("chunks_8x%d" % w).need) == [0] * 5
    check_case(pkg, "chunks_8x%d" % w)


# ---- many runs: the propagation in global memory, the table overflows --------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["combs_800x64", "lattice_6000x24", "random80_224x224"])
def test_many_runs_and_table_overflows(pkg, name):
    """combs_800x64: 6393 runs (beyond the 6144 the propagation holds in LDS, within rcap = 6400) settle, 12785 runs go to the flood;
    lattice_6000x24: more contacts than ecap; random80_224x224: more runs than rcap = 4096"""
    check_case(pkg, name)


# ---- wrap counts beyond int8 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["int8_rows_8x300", "int8_cols_300x64", "int8_m127_8x267"])
def test_wrap_counts_beyond_int8_go_to_the_flood(pkg, name):
    """more than 126 wraps inside a run; small runs whose absolute count passes 126; a single run whose count ends at exactly -127, the value
    the check keeps for "never reached" (no vertical neighbour would catch a plane that took it)"""
    assert all(n == 1 for n in U.case(name).need)
    check_case(pkg, name)


# ---- deep trees --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["deep_64x64", "deep_254x254"])
def test_trees_as_deep_as_the_mask(pkg, name):
    c, refs = U.case(name), U.references(name)
    for f, r in zip(c.frames, refs):
        if f.name.startswith("serpentine"):
            assert U.tree_depth(r["parent"], r["order"]) >= int((f.mask != 0).sum()) // 2
    check_case(pkg, name)


# ---- components and degenerate masks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["components_64x64", "components_215x300"])
def test_components_single_pixel_empty_mask_and_last_pixel_seed(pkg, name):
    c, refs = U.case(name), U.references(name)
    reached = [int((~r["nan"]).sum()) for r in refs]
    on = [int((f.mask != 0).sum()) for f in c.frames]
    assert 1 < reached[0] < on[0] // 4 and reached[1:3] == [1, 0] and on[1:3] == [1, 0] and reached[3] == on[3] == c.frames[3].mask.size
    assert U.first_argmax(c.frames[3].quality, c.frames[3].mask) == c.frames[3].mask.size - 1
    check_case(pkg, name)


# ---- the branch cut ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", U.RULE_CASES)
def test_pairs_on_the_branch_cut_follow_the_half_open_rule(pkg, name):
    """a step of exactly float32(pi), of pi - 5e-6 and of pi + 1e-4 across one column: the first two are ties for the check (need == 1), the third
    is not; every plane is the (-pi, pi] rule's, from the float64 restatement along the reference's tree"""
    c = U.case(name)
    assert name in U.RULE_CASES and list(c.need) == [1, 1, 0]
    step = [float(np.ptp(f.wrapped.astype(np.float64))) for f in c.frames]
    assert step[0] == float(U.PI32) and 4e-6 < np.pi - step[1] < 6e-6 and 0.9e-4 < step[2] - np.pi < 1.1e-4
    check_case(pkg, name)


# ---- mixed batches ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mixed_151x203", "mixed_254x254"])
def test_mixed_batch_equals_its_frames_run_alone(pkg, name):
    """settled, residue, empty mask, run-table overflow, settled in one launch: need == [0, 1, 0, 1, 0], and every frame bit-equal to the same
    frame run alone (the need[b] skips and the per-frame scratch strides)"""
    c = U.case(name)
    assert list(c.need) == [0, 1, 0, 1, 0]
    variants = (0, 1, 2) if name == "mixed_151x203" else (2,)       # 254 x 254: the hand-back to the generic flood, frame by frame
    planes = check_case(pkg, name, variants)
    for variant in variants[::2]:
        for b, f in enumerate(c.frames):
            uw, par, need, status, _ = run_unwrap(pkg, [f], variant)
            assert np.array_equal(uw[0].view(np.uint32), planes[variant][b].view(np.uint32)), (name, variant, f.name)
            assert status[0] == 0 and (variant != 0 or need[0] == c.need[b])


# ---- the hook's argument checks (no GPU needed: a refused call makes no HIP call) ------------------------------------------------------------------
def test_unwrap_hook_refuses_bad_arguments(pkg):
    lib = pkg._lib.load()
    buf = [np.zeros(256, np.int32) for _ in range(7)]
    p = [ctypes.c_void_p(b.ctypes.data) for b in buf]
    ok = dict(B=1, h=8, w=8, variant=0)
    for bad in (dict(B=0), dict(B=-1), dict(h=7), dict(w=7), dict(h=0), dict(w=-5), dict(variant=3), dict(variant=-1), dict(h=65536, w=65536),
                dict(h=32768), dict(w=65536)):
        a = dict(ok, **bad)
        assert lib.vistaf_ftp_test_unwrap(*p, a["B"], a["h"], a["w"], a["variant"], None) == E_INVALID, bad
    for i in range(7):                              # a null plane; `need` (5) may be null under variants 1 and 2 only
        args = list(p)
        args[i] = None
        assert lib.vistaf_ftp_test_unwrap(*args, 1, 8, 8, 0, None) == E_INVALID, i
        if i != 5:
            assert lib.vistaf_ftp_test_unwrap(*args, 1, 8, 8, 1, None) == E_INVALID, i
    assert b"variant 0" in lib.vistaf_ftp_last_error() or b"bad argument" in lib.vistaf_ftp_last_error()
