"""The scratch layouts of the seven stages that cut one device buffer into planes, read out by a counting pass of the very function each
launcher carves with (vistaf_ftp_test_scratch_regions, csrc/test_hooks.h).  Arithmetic only: no HIP call, no GPU.

A handle sizes every buffer for `max_batch` and carves it at the call's batch, so besides the layout's own consistency the regions of
every smaller batch must end inside the buffer of the larger one."""
import ctypes

import pytest

STAGES = ("unwrap", "telea", "inpaint_big", "inpaint_cl", "inpaint_win", "big", "tstats")
RANGED = ("inpaint_big",)                       # the stages whose layout depends on the inpaint radius (padding range + 1)
SHAPES = [(8, 8), (64, 64), (224, 224), (253, 254), (253, 255), (512, 512), (1182, 1182)]
BATCHES = (1, 3, 8, 64)
RANGES = (1, 3, 5)
HUGE = (8200, 8200)                             # EN >= 2^26: the generic flood's layout, beyond any GPU test
CAP = 32


def regions(lib, stage, B, h, w, rng=3):
    names = ctypes.create_string_buffer(32 * CAP)
    off, size, align = ((ctypes.c_size_t * CAP)() for _ in range(3))
    total = ctypes.c_size_t()
    n = lib.vistaf_ftp_test_scratch_regions(stage.encode(), B, h, w, rng, CAP, names, off, size, align, ctypes.byref(total))
    assert n > 0, (stage, n)
    return [(names.raw[32 * i:32 * i + 32].split(b"\0")[0].decode(), off[i], size[i], align[i]) for i in range(n)], total.value


def cases():
    for h, w in SHAPES:
        for B in BATCHES:
            yield B, h, w
    yield (1,) + HUGE


def ranges_of(stage):
    return RANGES if stage in RANGED else (3,)


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg._lib.load()


@pytest.mark.parametrize("stage", STAGES)
def test_regions_are_aligned_ordered_and_disjoint(lib, stage):
    for B, h, w in cases():
        for rng in ranges_of(stage):
            regs, total = regions(lib, stage, B, h, w, rng)
            assert all(name for name, *_ in regs) and len({name for name, *_ in regs}) == len(regs)
            end = 0
            for name, off, size, align in regs:
                where = (stage, B, h, w, rng, name)
                assert align >= 16 and align & (align - 1) == 0 and off % align == 0, where
                # ascending and disjoint: the read-out lists memory only, the aliases a struct documents are pointers into these regions
                assert off >= end and size > 0, where
                end = off + size
            assert end <= total, (stage, B, h, w, rng)


@pytest.mark.parametrize("stage", STAGES)
def test_a_smaller_batch_stays_inside_the_buffer_of_a_larger_one(lib, stage):
    for h, w in SHAPES:
        for rng in ranges_of(stage):
            ends = {}
            for B in range(1, max(BATCHES) + 1):
                regs, total = regions(lib, stage, B, h, w, rng)
                ends[B] = max(off + size for _, off, size, _ in regs)
                if B in BATCHES:
                    assert max(ends.values()) <= total, (stage, B, h, w, rng)
    # the big-cluster planes are sized at the widest padding and carved at the call's: every radius fits the buffer of radius 5
    for h, w in SHAPES:
        for B in BATCHES:
            widest = regions(lib, "inpaint_big", B, h, w, 5)[1]
            for rng in RANGES:
                assert regions(lib, "inpaint_big", B, h, w, rng)[1] <= widest


def test_floors_from_the_shapes_alone(lib):
    for B, h, w in cases():
        P, EN = h * w, (h + 2) * (w + 2)
        size = {name: s for name, _, s, _ in regions(lib, "unwrap", B, h, w)[0]}
        assert size["state"] >= B * P
        # five uint32 planes of EN per frame: two pairs that stay contiguous, and the padded parents
        assert size["sort_a"] >= 2 * B * EN * 4 and size["sort_b"] >= 2 * B * EN * 4 and size["ppar"] >= B * EN * 4
        assert size["rank"] >= B * EN * (2 if EN <= 65533 else 4)
        assert min(size["seed"], size["nmask"], size["need_generic"]) >= 4 * B
        assert size["check.kk"] >= B * P and size["check.rowbase"] >= 4 * B * (h + 1) and size["check.seedkey"] >= 8 * B

        size = {name: s for name, _, s, _ in regions(lib, "telea", B, h, w)[0]}
        assert size["T"] >= B * EN * 4 and size["flags"] >= B * EN * 2 and size["queue"] >= B * EN * 8 and size["nbad"] >= 4 * B

        size = {name: s for name, _, s, _ in regions(lib, "inpaint_cl", B, h, w)[0]}
        # six int32 planes (the box planes in pairs, one memset each) and three byte planes of B * P, and B counters
        assert size["labels"] >= B * P * 4 and size["list"] >= B * P * 4
        assert size["xmin_ymin"] >= 2 * B * P * 4 and size["xmax_ymax"] >= 2 * B * P * 4
        assert min(size["dil"], size["big"], size["bad_big"]) >= B * P and size["count"] >= 4 * B

        for rng in RANGES:
            M = rng + 1
            en = (h + 2 * M) * (w + 2 * M)
            size = {name: s for name, _, s, _ in regions(lib, "inpaint_big", B, h, w, rng)[0]}
            assert size["T"] >= B * en * 4 and size["im"] >= B * en * 4 and size["f"] >= B * en and size["gq"] >= B * 4 * 1024 * 8

        assert regions(lib, "inpaint_win", B, h, w)[0][0][2] >= 5 * B * 4
        size = {name: s for name, _, s, _ in regions(lib, "tstats", 1, h, w)[0]}
        assert size["vals"] >= P * 4 and size["sel"] >= P


# What vistaf_ftp_create and the temperature session allocated per stage before the layouts had one definition each, evaluated by running
# that revision's size functions (`*_bytes_per_frame(h, w) * max_batch + K` and the rest) for the benchmark's two workloads.  "inpaint" is the
# buffer the whole-frame and the big-cluster march share.
BEFORE = {
    (224, 224, 256): {"inpaint": 229249024, "inpaint_cl": 346834944, "inpaint_win": 5376, "unwrap": 337093632, "big": 9075712, "tstats": 252928},
    (1182, 1182, 8): {"inpaint": 169762848, "inpaint_cl": 301781344, "inpaint_win": 416, "unwrap": 293227488, "big": 763264, "tstats": 6994944},
}


@pytest.mark.parametrize("shape", sorted(BEFORE))
def test_no_growth_against_the_hand_written_sizes(lib, shape):
    """A stage may exceed its earlier total by at most 256 bytes per region: the worst case of aligning every region."""
    h, w, B = shape
    for stage, before in BEFORE[shape].items():
        if stage == "inpaint":
            layouts = [regions(lib, "telea", B, h, w), regions(lib, "inpaint_big", B, h, w, 5)]
            regs, total = max(layouts, key=lambda rt: rt[1])
        else:
            regs, total = regions(lib, stage, 1 if stage == "tstats" else B, h, w)
        print(shape, stage, "before", before, "now", total, "regions", len(regs))
        assert total <= before + 256 * len(regs), (stage, before, total)


def test_unknown_stage_is_refused(lib):
    total = ctypes.c_size_t()
    buf = ctypes.create_string_buffer(32 * CAP)
    arr = (ctypes.c_size_t * CAP)()
    assert lib.vistaf_ftp_test_scratch_regions(b"nope", 1, 8, 8, 3, CAP, buf, arr, arr, arr, ctypes.byref(total)) < 0
    assert lib.vistaf_ftp_test_scratch_regions(b"unwrap", 1, 8, 8, 3, 2, buf, arr, arr, arr, ctypes.byref(total)) < 0      # 16 regions, cap 2
