"""The load, reduce-and-solve and residual-plane phases of the column IRLS fit (csrc/k_fit.hip, robust_polyfit_col_body), launched directly
on small batches: the production instance <56, 4> at its own size and at a size with dead rows and columns, and the runtime-groups instance,
each with order 1 (the step that accumulates and reduces nine sums) and order 2 (twenty-one), with six iterations and with one (no
medians at all).  Bars and launcher are those of tests/test_kernels_direct.py.

Not compared here: the streaming chain (variant 2).  It takes planes of 262144 pixels and more, the column instances end at 64 rows per
thread of a 1024-thread workgroup, so no shape reaches both and the chain's coefficients cannot be set against a column instance's bit for
bit; the tests only record that the chain refuses these shapes.  What pins "same bits" for the sums an order-1 step no longer forms is the
comparison of whole benchmark outputs between builds (profiles/README.md), not a test of this file: the float64 bars below are four times
the float32 reference's own error, which a reassociated sum would still meet."""
import functools

import numpy as np
import pytest

import kernel_refs as R
from test_kernels_direct import FIT_FLOOR_ULPS, FIT_MULT, gpu_polyfit

pytestmark = pytest.mark.gpu

C = 4.685
# (h, w) -> instance: cols_pad = w rounded up to 64, groups = min(1024 / cols_pad, h), rows per thread = ceil(h / groups)
SHAPES = [((224, 224), "col56_g4"),       # 256, 4, 56: the production instance
          ((222, 200), "col56_g4"),       # 256, 4, 56 with h % groups != 0 and 56 dead columns
          ((96, 80), "col16")]            # 128, 8, 12: runtime row groups


@functools.lru_cache(maxsize=None)
def phase_inputs(h, w):
    """frame 0: disc with holes, whole rows and a whole 64-column span (one wave per row group) without a sample, NaN and inf inside the mask, finite z outside it;
    frame 1: the holes alone, z quantised to 1/64 (ties in both medians);  frame 2: 150 mask pixels (fewer than 200 fitted samples)"""
    rng = np.random.default_rng(1000 * h + w)
    yy, xx = np.indices((h, w))
    xn, yn = (xx - (w - 1) / 2) / ((w - 1) / 2), (yy - (h - 1) / 2) / ((h - 1) / 2)
    disc = (xn * 1.05) ** 2 + (yn * 1.05) ** 2 <= 1.0
    holes = np.ones((h, w), bool)
    for _ in range(6):
        cy, cx, rr = rng.integers(0, h), rng.integers(0, w), max(2, min(h, w) // 9)
        holes &= (yy - cy) ** 2 + (xx - cx) ** 2 > rr * rr
    zs, ms = [], []
    for i in range(3):
        cf = rng.uniform(-2, 2, 6)
        z = cf[0] * xn + cf[1] * yn + 3.0 * cf[2] + cf[3] * xn * xn + cf[4] * xn * yn + cf[5] * yn * yn + 0.02 * rng.standard_normal((h, w))
        o = rng.random((h, w)) < 0.05
        z[o] += rng.choice([-1.0, 1.0], int(o.sum())) * rng.uniform(2, 6, int(o.sum()))
        if i == 1:
            z = np.round(z * 64) / 64
        z = z.astype(np.float32)
        if i == 0:
            m = disc & holes
            m[h // 3:h // 3 + 5] = False                   # five whole rows (more than one row group's worth) ...
            m[:, 64:128] = False                            # ... and the 64 columns of every row group's second wave without a sample
            z[rng.random((h, w)) < 0.03] = np.nan
            z[rng.random((h, w)) < 0.002] = np.inf
        elif i == 1:
            m = holes.copy()
        else:
            m = np.zeros((h, w), bool)
            m.flat[rng.permutation(h * w)[:150]] = True
        zs.append(z)
        ms.append(m.astype(np.uint8))
    z, m = np.stack(zs), np.stack(ms)
    z.setflags(write=False)
    m.setflags(write=False)
    return z, m


@functools.lru_cache(maxsize=None)
def phase_refs(h, w, order, iters):
    z, mask = phase_inputs(h, w)
    return [(R.polyfit_ref32(z[b], mask[b], order, iters, C), R.polyfit_ref64(z[b], mask[b], order, iters, C)) for b in range(2)]


def eval_resid32(z, coef, order, fitted):
    """z - fit in float32 with eval_poly2d's operation order, from float32 coefficients (z itself where the frame was not fitted)"""
    h, w = z.shape
    f = np.float32
    cx, cy = f((w - 1) / 2.0), f((h - 1) / 2.0)
    xn = ((np.arange(w, dtype=f) - cx) / cx)[None, :]
    yn = ((np.arange(h, dtype=f) - cy) / cy)[:, None]
    c = coef.astype(f)
    with np.errstate(all="ignore"):
        if not fitted:
            return z - f(0)
        fit = (c[0] * xn + c[1] * yn) + c[2]
        if order >= 2:
            fit = fit + (c[3] * xn) * xn
            fit = fit + (c[4] * xn) * yn
            fit = fit + (c[5] * yn) * yn
        return (z - fit).astype(f)


def same_plane(got, exp):
    nan = np.isnan(exp)
    return np.array_equal(np.isnan(got), nan) and (R.bits(got)[~nan] == R.bits(exp)[~nan]).all()


@pytest.mark.parametrize("iters", [6, 1])
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("shape,expect", SHAPES)
def test_fit_phases_against_float64_and_own_coefficients(pkg, shape, expect, order, iters):
    h, w = shape
    z, mask = phase_inputs(h, w)
    coef, resid, inst = gpu_polyfit(pkg, z, mask, order, 0, iters=iters)
    assert inst == expect
    refs = phase_refs(h, w, order, iters)
    for b in range(2):
        (c32, r32), (c64, r64) = refs[b]
        fin = np.isfinite(z[b])
        zmax = float(np.abs(z[b][fin]).max())
        assert np.array_equal(np.isfinite(resid[b]), fin), "residual plane finite exactly where z is"
        e32 = max(float(np.abs(r32[fin] - r64[fin]).max()), float(np.abs(c32 - c64).max()))
        dg = max(float(np.abs(resid[b][fin] - r64[fin]).max()), float(np.abs(coef[b] - c64).max()))
        bar = max(FIT_MULT * e32, FIT_FLOOR_ULPS * 2.0 ** -23 * zmax)
        print("fit %4dx%-4d %-9s order %d iters %d frame %d: e32 %.3e  gpu %.3e  bar %.3e  max|z| %.2f" % (h, w, inst, order, iters, b, e32, dg, bar, zmax))
        assert bar <= 1e-5 * zmax, "the bar itself stays far below the end-to-end 1e-4 of peak"
        assert dg <= bar, (h, w, inst, order, iters, b, dg, bar)
        if order == 1:
            assert not coef[b, 3:].any()
    # every pixel of every frame, fitted or not: z - fit of the returned coefficients, bit for bit
    for b in range(3):
        assert same_plane(resid[b], eval_resid32(z[b], coef[b], order, fitted=b < 2)), (h, w, order, iters, b)
    # frame 2: fewer than 200 fitted samples
    assert int(((mask[2] != 0) & np.isfinite(z[2])).sum()) < 200 and not coef[2].any()
    # the streaming chain refuses every shape a column instance takes (see the module docstring)
    with pytest.raises(ValueError):
        gpu_polyfit(pkg, z, mask, order, 2, iters=iters)


@pytest.mark.parametrize("shape,expect", SHAPES)
def test_fit_phases_ramp_gate_returns_z(pkg, shape, expect):
    """between 200 and 500 mask pixels under min_mask_count = 500, order 1: zero coefficients and z back, bit for bit; without the gate
    the same planes are fitted"""
    h, w = shape
    z, _ = phase_inputs(h, w)
    rng = np.random.default_rng(h + w)
    mask = np.zeros((3, h, w), np.uint8)
    for b, cnt in enumerate((200, 350, 499)):
        mask[b].flat[rng.permutation(h * w)[:cnt]] = 1
    z = np.where(np.isfinite(z), z, np.float32(0.5)).astype(np.float32)
    z[0, 0, 0] = np.float32(-0.0)
    for iters in (6, 1):
        coef, resid, inst = gpu_polyfit(pkg, z, mask, 1, 0, iters=iters, min_mask_count=500)
        assert inst == expect and not coef.any() and (R.bits(resid) == R.bits(z)).all()
    coef, resid, _ = gpu_polyfit(pkg, z, mask, 1, 0, min_mask_count=0)
    assert coef[:, :3].any(axis=1).all()
    for b in range(3):
        assert same_plane(resid[b], eval_resid32(z[b], coef[b], 1, fitted=True))
