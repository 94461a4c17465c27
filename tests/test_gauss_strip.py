"""The long Gaussian blurs in one launch (csrc/k_basic.hip: k_gauss_strip; session hook "gauss_strip", csrc/test_hooks.h) against the row and the
column kernel they stand in for, and the sessions around them.

Main bar: the dispatch (variant 0) and the strip kernel (variant 2) equal tests/kernel_refs.blur_ref32 AND the two kernels (variant 1) BIT FOR
BIT -- the strip kernel runs the same taps in the same order per output and rounds its LDS intermediate to float as the intermediate plane is.
Shapes sit on the kernel's edges: a strip is 32 output columns (seams at 31 | 32, 63 | 64, 95 | 96, a partial last strip), the row pass takes
32 rows per chunk (seams at 31 | 32, 63 | 64; the 15 | 16 seam of a 16-row chunk is kept too), the column pass 8 rows per thread and 64 rows per
round, frames narrower or lower than the radius reflect repeatedly, and batches that are no multiple of eight exercise the block remap.  dst is
pre-filled with a sentinel so that an unwritten pixel shows.  The sessions (scaled and shipped constants, pair mode, no frontier band) run with
the tier on, off and on again; they also cover the plane that the second distance transform lands in when the fused compose runs."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import kernel_refs as R
import test_kernels_direct as KD
from oracle import cvlite

pytestmark = pytest.mark.gpu
_dev, _ptr = KD._dev, KD._ptr
TWO, STRIP, TILE = 1, 2, 3            # GaussTier of csrc/kernels.hpp
SENTINEL = 777.0
# sigma -> taps: 17 the first long kernel; 19 and 23 a last refill of 2 and of 2 + 4 taps; 69 the workload's; 73
SIGMA_TAPS = [(2.0, 17), (2.25, 19), (2.75, 23), (8.5, 69), (9.0, 73)]
WIDTHS = (1, 8, 31, 32, 33, 63, 65, 100)
HEIGHTS = (1, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65)


def pitch_of(taps):
    """gs_pitch of kernels.hpp: the chunk's row pitch, an odd multiple of four floats"""
    return 4 * (((32 + 2 * (taps // 2) + 3) // 4) | 1)


def max_height(taps):
    """the largest h with (h * 32 + 32 * pitch + 2 * 104) * 4 <= 48 KB (gauss_strip_lds: the plane, the chunk, two copies of the taps)"""
    return (48 * 1024 // 4 - 2 * 104) // 32 - pitch_of(taps)


def gauss(pkg, src, sigma, variant):
    B, h, w = src.shape
    ds = _dev(src)
    dst = torch.full((B, h, w), SENTINEL, dtype=torch.float32, device="cuda")
    rc = pkg._lib.load().vistaf_ftp_test_gauss_variant(_ptr(ds), _ptr(dst), float(sigma), B, h, w, variant, None)
    return rc, dst.cpu().numpy()


def inputs(h, w, seed):
    """the kinds of test_kernels_direct.blur_inputs, the impulses on both sides of every strip and chunk seam the frame has and in the corners"""
    rng = np.random.default_rng(seed)
    noise = rng.standard_normal((h, w)).astype(np.float32)
    imp = np.zeros((h, w), np.float32)
    for y in (0, h - 1, 15, 16, 31, 32, 63, 64):
        for x in (0, w - 1, 31, 32, 63, 64, 95, 96):
            if y < h and x < w:
                imp[y, x] = 1.0 + 0.25 * ((y + 3 * x) % 7)
    wide = (10.0 ** rng.uniform(-30, 30, (h, w)) * rng.choice([-1.0, 1.0], (h, w))).astype(np.float32)
    bad = noise.copy()
    bad[h // 2, w // 3] = np.nan
    bad[h // 4, (2 * w) // 3] = np.inf
    bad[h - 1, w - 1] = -np.inf
    return np.stack([noise, imp, wide]), bad[None]


def same_bits(tag, got, exp):
    ndiff = int((R.bits(got) != R.bits(exp)).sum())
    assert ndiff == 0, (tag, ndiff)


def check_shape(pkg, sigma, taps, h, w, seeds=(0,)):
    """variants 0, 1 and 2 on 3 x len(seeds) finite planes and on one plane with NaN and +-Inf"""
    fits = max_height(taps) >= h
    planes = [inputs(h, w, 1000 * taps + 31 * h + w + 7919 * s) for s in seeds]
    src, bad = np.concatenate([p[0] for p in planes]), planes[0][1]
    exp = np.stack([R.blur_ref32(p, sigma) for p in src])
    exp_bad = R.blur_ref32(bad[0], sigma)
    fin = np.isfinite(exp_bad)
    for variant, tier in ((0, STRIP if fits else TWO), (1, TWO), (2, STRIP)):
        rc, got = gauss(pkg, src, sigma, variant)
        if variant == 2 and not fits:
            assert rc == -1 and (got == SENTINEL).all(), (taps, h, w, "variant 2 must refuse before any launch")
            continue
        assert rc == tier, (taps, h, w, variant, rc)
        same_bits((taps, h, w, variant), got, exp)
        rc, got = gauss(pkg, bad, sigma, variant)
        assert rc == tier
        got = got[0]
        assert np.array_equal(np.isnan(got), np.isnan(exp_bad)) and np.array_equal(np.isposinf(got), np.isposinf(exp_bad)) and \
            np.array_equal(np.isneginf(got), np.isneginf(exp_bad)), (taps, h, w, variant, "classes of the NaN / Inf plane")
        assert (R.bits(got)[fin] == R.bits(exp_bad)[fin]).all(), (taps, h, w, variant, "finite part of the NaN / Inf plane")


# =======================================================================================================================================
# what a blur takes

def test_the_hooks_have_matching_signatures(pkg):
    """csrc/test_hooks_gauss.h against _lib.GAUSS_STRIP_SIGNATURES: the same functions, and a pointer where the header has one"""
    text = open(os.path.join(os.path.dirname(pkg.__file__), "csrc", "test_hooks_gauss.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    protos = {name: [p.strip() for p in params.split(",")] for name, params in re.findall(r"\bint\s+(vistaf_\w+)\s*\(([^()]*)\)\s*;", text)}
    table = pkg._lib.GAUSS_STRIP_SIGNATURES
    assert sorted(protos) == sorted(table) and len(protos) == 2
    for name, params in protos.items():
        restype, argtypes = table[name]
        assert restype is ctypes.c_int and len(argtypes) == len(params), name
        for p, a in zip(params, argtypes):
            if "*" in p:
                assert a is ctypes.c_void_p, (name, p)
            else:
                assert a is (ctypes.c_double if p.startswith("double") else ctypes.c_int), (name, p)


def test_what_a_blur_takes(pkg):
    fits = pkg._lib.load().vistaf_ftp_test_gauss_strip_fits
    assert fits(224, 224, 69) == 1 and fits(224, 224, 73) == 1 and fits(224, 224, 21) == 1 and fits(224, 224, 49) == 1
    assert fits(224, 224, 15) == 0 and fits(224, 224, 97) == 1 and fits(224, 224, 99) == 0          # the tile's kernels; two loads per lane and row
    assert fits(1182, 1182, 69) == 0 and fits(1, 1, 17) == 1
    for _, taps in SIGMA_TAPS:
        hmax = max_height(taps)
        assert fits(hmax, 40, taps) == 1 and fits(hmax + 1, 40, taps) == 0, taps
    assert (pitch_of(69), max_height(69)) == (100, 277) and (pitch_of(73), max_height(73)) == (108, 269) and (pitch_of(17), max_height(17)) == (52, 325)
    assert fits(0, 4, 17) < 0 and fits(4, 4, 16) < 0
    for sigma, taps in SIGMA_TAPS:
        assert cvlite.gaussian_ksize(sigma) == taps


def test_short_kernels_keep_the_tile(pkg):
    """15 taps: the dispatch takes the one-kernel tile, variant 1 the two kernels, variant 2 refuses"""
    src, _ = inputs(33, 65, 5)
    exp = np.stack([R.blur_ref32(p, 1.75) for p in src])
    for variant, tier in ((0, TILE), (1, TWO)):
        rc, got = gauss(pkg, src, 1.75, variant)
        assert rc == tier
        same_bits(("15 taps", variant), got, exp)
    rc, got = gauss(pkg, src, 1.75, 2)
    assert rc == -1 and (got == SENTINEL).all()
    assert gauss(pkg, src, 1.75, 3)[0] == -1


# =======================================================================================================================================
# the kernels

@pytest.mark.parametrize("sigma,taps", SIGMA_TAPS)
def test_strip_seams_chunk_seams_and_small_frames(pkg, sigma, taps):
    """every width against every height: strip seams, a partial last strip, chunk seams, frames narrower and lower than the radius (r = 34 and
    36 against w = 1, 8, 31 and h = 1, 8, ..: the reflection repeats)"""
    for h in HEIGHTS:
        for w in WIDTHS:
            check_shape(pkg, sigma, taps, h, w)


@pytest.mark.parametrize("sigma,taps", SIGMA_TAPS)
def test_largest_height_and_one_more(pkg, sigma, taps):
    """the largest height gauss_strip_fits takes at the tap count (several chunks, several rounds of the column pass, a partial last chunk),
    and one row more: the dispatch runs the two kernels, variant 2 refuses"""
    hmax = max_height(taps)
    check_shape(pkg, sigma, taps, hmax, 33)
    check_shape(pkg, sigma, taps, hmax + 1, 33)


@pytest.mark.parametrize("nseed", [1, 3])
def test_batches_off_the_block_remap(pkg, nseed):
    """batches of 3 and 9 planes (and the single NaN / Inf plane: a batch of 1), 1 to 4 strips each: block counts that are no multiple of eight"""
    for sigma, taps in ((2.0, 17), (8.5, 69)):
        for h, w in ((17, 8), (33, 65), (40, 100)):
            check_shape(pkg, sigma, taps, h, w, seeds=tuple(range(nseed)))


def test_the_workloads_frame(pkg):
    """224 x 224 at 69 taps, three planes: the benchmark's illumination blur"""
    check_shape(pkg, 8.5, 69, 224, 224)


# =======================================================================================================================================
# sessions

def _outputs(out):
    return {k: v.cpu().numpy().copy() for k, v in out.items()}


def _planes(sensor, nb):
    return {name: sensor.intermediate(name, nb, torch.float32).cpu().numpy().copy() for name in ("iw", "hmap", "unitless")}


@pytest.mark.parametrize("n", [224, 200])
@pytest.mark.parametrize("mode", ["scaled", "shipped", "pairs", "no_band"])
def test_sessions_give_the_same_bytes_with_and_without_the_tier(pkg, n, mode):
    """4 frames of n x n (200: a partial last strip) with gauss_strip 1, 0 and 1 again: outputs, scalars, status and the planes iw, hmap and
    unitless byte for byte.  scaled: the illumination blur (69 taps at 224) is the only long one; shipped: quality, reliable-only and
    unreliable-region blurs are long too and the kernel sequence composes; pairs: predict_pairs; no_band: frontier_zero_band_px = 0, the fused
    compose without the distance pair"""
    g = os.path.join(os.path.dirname(__file__), "golden")
    model, neg = pkg.load_calibration(os.path.join(g, "calibration_phase_to_height.json"))
    fm = pkg.load_force_calibration(os.path.join(g, "calibration_height_to_force.json"))["best_model"]
    nb = 4
    cfg = pkg.FtpConfig.as_shipped() if mode == "shipped" else pkg.FtpConfig.scaled(n)
    if mode == "no_band":
        cfg.frontier_zero_band_px = 0
    circle = pkg.synth.roi_circle(n)
    if mode == "pairs":
        periods = [pkg.synth.NATIVE_PERIOD_PX * n / pkg.synth.NATIVE_CROP, 11.3]
        refs = np.stack([pkg.synth._base(n, 0.0, np.random.default_rng(770000 + b), periods[b % 2]) for b in range(nb)])
        defs = np.stack([pkg.synth.deformed_frame(n, 5100 + b, config=3, period=periods[b % 2], amp_scale=1.0 + 0.5 * (b % 3)) for b in range(nb)])
        sensor = pkg.FtpSensor(None, circle, cfg, model, neg, fm, max_batch=nb, frame_shape=(n, n))
        run = lambda: sensor.predict_pairs(refs, defs)
    else:
        ref = pkg.synth.reference_frame(n, config=3)
        frames = pkg.synth.deformed_batch(n, 600, nb, config=3)
        sensor = pkg.FtpSensor(ref, circle, cfg, model, neg, fm, max_batch=nb)
        run = lambda: sensor.predict_batch(frames)
    res = []
    for tier in (1, 0, 1):
        sensor._test_set("gauss_strip", tier)
        out = _outputs(run())
        torch.cuda.synchronize()
        out.update({"plane:" + k: v for k, v in _planes(sensor, nb).items()})
        res.append(out)
    sensor.close()
    assert {"height_map_mm", "output_reliable", "scalars", "status"} <= set(res[1])
    for other in (res[0], res[2]):
        assert set(other) == set(res[1])
        for key, want in res[1].items():
            assert other[key].tobytes() == want.tobytes(), (n, mode, key)
