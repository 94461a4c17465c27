"""The selection, IRLS fit and Gaussian kernels launched directly (csrc/test_hooks.h: vistaf_ftp_test_select / _polyfit / _gauss) on inputs
no fringe image produces, against the plain references of tests/kernel_refs.py; and the three fused blur chains through a session at every
tap count from 3 to 17.  Every figure a bar applies to is printed before it is asserted (run with -s to see them)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import kernel_refs as R
from oracle import cvlite
from oracle import ftp_oracle as O

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


# =======================================================================================================================================
# selection

QS = [0.0, 8.0, 25.0, 50.0, 92.0, 99.7, 99.9, 100.0, R.MEDIAN]
REQ_TRIPLES = [QS[0:3], QS[3:6], QS[6:9]]           # three requests per call (the k_big.hip chain takes at most four)
KEY_LO, KEY_HI = 0x90000000, 0xD0000000             # positive normal floats; the key range 2^30 needs 31 bits
HIST_BITS = {1: 13, 2: 11}                          # histogram digits per refinement level: select.hpp SEL_BITS, k_big.hip SB_BITS


def boundary_keys(hist_bits):
    """(first, later): the key just below a bucket boundary of the first refinement level (bucket width 2^(31 - bits)) and just below a
    boundary of the second level (width 2^(31 - 2 bits)) that lies inside a first-level bucket, not on its edge"""
    s1, s2 = 31 - hist_bits, 31 - 2 * hist_bits
    j1 = (1 << (30 - s1)) - 96                      # a first-level bucket near the top of the range: 4000 of 4096, 928 of 1024
    first = KEY_LO + (j1 << s1) - 1
    later = KEY_LO + (j1 << s1) + (((1 << hist_bits) * 3 // 8 + 1) << s2) - 1
    assert (later + 1 - KEY_LO) % (1 << s2) == 0 and (later + 1 - KEY_LO) % (1 << s1) != 0 and KEY_LO < later < KEY_HI
    return first, later


def gpu_select(pkg, vals, mask, mask_stride, le_thr, use_abs, reqs, variant):
    """vals [B, P] float32, mask [P] (stride 0) or [B, P] uint8, le_thr [B] or None -> (out [B, nreq] float32, counts [B])"""
    B, P = vals.shape
    dv, dm = _dev(vals), _dev(mask)
    dl = _dev(np.asarray(le_thr, np.float32)) if le_thr is not None else None
    dr = _dev(np.array([R.request_value(q) for q in reqs], np.float32))
    out = torch.full((B, len(reqs)), 12345.0, dtype=torch.float32, device="cuda")
    cnt = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    rc = pkg._lib.load().vistaf_ftp_test_select(_ptr(dv), _ptr(dm), mask_stride, _ptr(dl), int(use_abs), _ptr(dr), len(reqs), _ptr(out), _ptr(cnt),
                                                B, P, variant, None)
    pkg._lib.check(rc)
    return out.cpu().numpy(), cnt.cpu().numpy()


def _rank_of(n, q):
    return (n - 1) // 2 if q is R.MEDIAN else min(n - 1, int(np.floor((n - 1) * q / 100.0)))


def _keys_around(n, k, a_key, b_key, rng):
    """n keys in [KEY_LO, KEY_HI] with exactly k keys below a_key, then a_key at rank k and b_key at rank k + 1; half of the others crowd the
    2^17 keys next to the pair (more than 1024 of them as soon as n allows, so the refinement cannot stop at a candidate sort early)"""
    def draw(cnt, lo, hi, near_lo, near_hi, pin):
        if cnt <= 0:
            return np.empty(0, np.uint32)
        far = rng.integers(lo, hi, cnt // 2, dtype=np.int64, endpoint=True)
        near = rng.integers(max(lo, near_lo), min(hi, near_hi), cnt - cnt // 2, dtype=np.int64, endpoint=True)
        out = np.concatenate([far, near])
        out[0] = pin                       # the end of the key range: fixes the histogram's origin and width
        return out.astype(np.uint32)
    below = draw(k, KEY_LO, a_key - 1, a_key - (1 << 17), a_key - 1, KEY_LO)
    above = draw(n - k - 2, b_key + 1, KEY_HI, b_key + 1, b_key + (1 << 17), KEY_HI)
    mid = np.array([a_key, b_key][:max(0, min(2, n - k))], np.uint32)
    keys = np.concatenate([below, mid, above])[:n]
    return keys


def selection_inputs(P, seed, hist_bits=13):
    """name -> float32[P].  The rank-targeted ones aim at the lower rank of the median / 50th percentile and of the 92nd percentile of a
    plane whose elements are all valid; under a mask, abs or a threshold they are simply further inputs.  (At P = 1 and 2 there is no room
    for the ends of the key range next to the pair, so the boundary inputs are plain two-element planes there.)"""
    rng = np.random.default_rng(seed)
    normal = rng.standard_normal(P).astype(np.float32)
    d = {}
    d["all_equal"] = np.full(P, 1.25, np.float32)
    d["all_negative_zero"] = np.full(P, -0.0, np.float32)
    for q in (50.0, 92.0):
        k = _rank_of(P, q)
        t = min(1500, max(1, P // 3))                                                    # copies of each of the two values
        v = np.concatenate([-1.0 - rng.random(max(0, k + 1 - t)), np.full(min(t, k + 1), 0.5), np.full(min(t, P), 0.75), 2.0 + rng.random(P)])[:P]
        d["ties_at_rank_q%g" % q] = rng.permutation(v.astype(np.float32))
        d["two_values_split_q%g" % q] = rng.permutation(np.where(np.arange(P) <= k, np.float32(-2.5), np.float32(7.0)).astype(np.float32))
        for level, a_key in zip(("first", "later"), boundary_keys(hist_bits)):
            d["bucket_boundary_%s_q%g" % (level, q)] = R.key2f(rng.permutation(_keys_around(P, k, a_key, a_key + 1, rng)))
    z = rng.choice(np.array([-0.0, 0.0, -1e-3, 1e-3], np.float32), P, p=[0.4, 0.4, 0.1, 0.1])
    d["signed_zeros"] = z.astype(np.float32)
    d["denormals"] = (rng.integers(1, 0x7FFFFF, P, dtype=np.uint32) | (rng.integers(0, 2, P, dtype=np.uint32) << np.uint32(31))).view(np.float32)
    d["span_3e38"] = rng.uniform(-3e38, 3e38, P).astype(np.float32)
    d["sorted"] = np.sort(normal)
    d["reversed"] = np.sort(normal)[::-1].copy()
    d["sawtooth"] = ((np.arange(P) % 37) * np.float32(0.25) - np.float32(4.0)).astype(np.float32)
    nf = normal.copy()
    bad = rng.random(P)
    nf[bad < 0.08] = np.nan
    nf[(bad >= 0.08) & (bad < 0.14)] = np.inf
    nf[(bad >= 0.14) & (bad < 0.2)] = -np.inf
    d["nan_inf_scattered"] = nf
    return d


def _count_mask(P, n_valid, rng):
    m = np.zeros(P, np.uint8)
    m[rng.permutation(P)[:min(P, n_valid)]] = 1
    return m


_REF_CACHE = {}


def _check_select(pkg, P, variant, B, seed):
    """every input of selection_inputs (plus planes with 0, 1 and 2 valid elements) in batches of B frames, all request triples, abs on and
    off, threshold given and null, one mask for the batch and one per frame; results bit-equal (kernel_refs.same_result), counts exact"""
    rng = np.random.default_rng(seed + 1)
    inputs = selection_inputs(P, seed, HIST_BITS[variant])
    names = list(inputs)
    frames = [inputs[k] for k in names]
    # every input runs with all of its elements valid ("full": the rank-targeted inputs are built for that) and under a random mask ("own")
    masks = [(rng.random(P) < 0.7).astype(np.uint8) for _ in frames]
    full = [np.ones(P, np.uint8) for _ in frames]
    for nv in (0, 1, 2):                          # 0, 1, 2 valid elements: through the mask, and through NaN under a full mask
        names.append("valid_%d_by_mask" % nv)
        frames.append(inputs["sorted"])
        masks.append(_count_mask(P, nv, rng))
        full.append(masks[-1])
        names.append("valid_%d_by_nan" % nv)
        f = np.full(P, np.nan, np.float32)
        f[rng.permutation(P)[:min(P, nv)]] = np.float32(-3.5)
        frames.append(f)
        masks.append(np.ones(P, np.uint8))
        full.append(masks[-1])
    while len(frames) % B:
        names.append(names[len(frames) % 7] + "_again")
        frames.append(frames[len(frames) % 7])
        masks.append(masks[len(masks) % 7])
        full.append(full[len(full) % 7])
    shared = {"shared_full": np.ones(P, np.uint8), "shared_70pct": (rng.random(P) < 0.7).astype(np.uint8), "shared_0": _count_mask(P, 0, rng), "shared_1": _count_mask(P, 1, rng),
              "shared_2": _count_mask(P, 2, rng)}
    # thresholds: the median of each frame's finite |values| (keeps about half), computed once
    les = []
    for f in frames:
        fin = np.abs(f[np.isfinite(f)])
        les.append(np.float32(np.median(fin)) if fin.size else np.float32(0.0))
    nbad, ncases, worst = 0, 0, []
    for g0 in range(0, len(frames), B):
        sl = slice(g0, g0 + B)
        vals = np.stack(frames[sl])
        for mname, mask, stride in [("full", np.stack(full[sl]), P), ("own", np.stack(masks[sl]), P)] + [(k, v, 0) for k, v in shared.items()]:
            for use_abs in (False, True):
                for use_le in (False, True):
                    if stride == 0 and mname not in ("shared_70pct", "shared_full") and (use_abs or use_le):
                        continue
                    le = np.array(les[sl], np.float32) if use_le else None
                    for reqs in REQ_TRIPLES:
                        out, cnt = gpu_select(pkg, vals, mask, stride, le, use_abs, reqs, variant)
                        for b in range(vals.shape[0]):
                            mb = mask if stride == 0 else mask[b]
                            key = (P, seed, variant, names[g0 + b], mname, use_abs, use_le, tuple(reqs))
                            if key not in _REF_CACHE:
                                _REF_CACHE[key] = R.select_ref(vals[b], mb, reqs, use_abs, le[b] if use_le else None)
                            exp, n, nbrs = _REF_CACHE[key]
                            ncases += 1
                            ok = int(cnt[b]) == n and all(R.same_result(out[b, j], exp[j]) for j in range(len(reqs)))
                            if not ok:
                                nbad += 1
                                if len(worst) < 12:
                                    worst.append((names[g0 + b], mname, "abs" if use_abs else "", "le=%r" % (le[b] if use_le else None), reqs,
                                                  "got", [hex(x) for x in R.bits(out[b])], "exp", [hex(x) for x in R.bits(exp)],
                                                  "count", int(cnt[b]), n, "rank, s[k-1], s[k], s[k+1]", nbrs))
    print("select P=%d variant=%d B=%d: %d frame-calls, %d wrong" % (P, variant, B, ncases, nbad))
    for wv in worst[:4]:
        print("  wrong:", wv)
    assert nbad == 0, worst


@pytest.mark.parametrize("P", [1, 2, 1023, 1024, 1025, 8191, 8192, 8193, 50176, 262143])
def test_select_per_frame_kernel(pkg, P):
    """k_select (variant 1) at plane sizes around the thread count, the 8192-element pass unit and just below the chain's threshold."""
    _check_select(pkg, P, 1, 3, 1000 + P % 997)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("P", [262144, 300001])
def test_select_streaming_chain(pkg, P, B):
    """launch_select_big (variant 2).  No valid element: the specified result is the quiet NaN 0x7fc00000 and count 0, as for k_select
    (block_percentile / block_median return it; the reference's nanpercentile_safe returns the caller's fallback there)."""
    _check_select(pkg, P, 2, B, 2000 + P % 997)
    if B == 3:
        _REF_CACHE.clear()          # B = 1 ran before with the same frames: the references are shared between the two


def test_select_production_dispatch_and_refusals(pkg):
    """variant 0 takes the per-frame kernel below 262144 pixels and the chain from there on; both give the reference's bits.  variant 2 is
    refused where the chain does not apply."""
    for P in (50176, 262144):
        rng = np.random.default_rng(P)
        vals = rng.standard_normal((2, P)).astype(np.float32)
        mask = (rng.random((2, P)) < 0.6).astype(np.uint8)
        out, cnt = gpu_select(pkg, vals, mask, P, None, True, [8.0, 92.0, R.MEDIAN], 0)
        for b in range(2):
            exp, n, _ = R.select_ref(vals[b], mask[b], [8.0, 92.0, R.MEDIAN], True)
            assert int(cnt[b]) == n and all(R.same_result(out[b, j], exp[j]) for j in range(3))
    with pytest.raises(ValueError):
        gpu_select(pkg, np.zeros((1, 1024), np.float32), np.ones(1024, np.uint8), 0, None, False, [50.0], 2)


# =======================================================================================================================================
# IRLS fit

FITV = ["big", "generic", "generic_div", "col16", "col32", "col48", "col56", "col64", "col48_g4", "col56_g4", "col64_g4"]     # kernels.hpp: FitVariant
# (h, w) -> the instance production dispatch (variant 0) takes; worked from polyfit_variant: cols_pad = w rounded up to 64,
# groups = min(1024 / cols_pad, h), need = ceil(h / groups)
LADDER = [((128, 128), "col16"),        # cols_pad 128, groups 8, need 16
          ((160, 160), "col32"),        # 192, 5, 32
          ((140, 300), "col48"),        # 320, 3, 47
          ((165, 300), "col56"),        # 320, 3, 55
          ((190, 300), "col64"),        # 320, 3, 64
          ((151, 203), "col48_g4"),     # 256, 4, 38
          ((224, 224), "col56_g4"),     # 256, 4, 56
          ((256, 256), "col64_g4"),     # 256, 4, 64
          ((320, 320), "generic"),      # 320, 3, 107 > 64
          ((512, 512), "big")]          # 262144 pixels: the k_big.hip chain
FIT_MULT = 4.0        # the GPU's distance from the float64 fit may be this many times the float32 LAPACK path's own (direct kernel tests)
FIT_FLOOR_ULPS = 4.0  # ... and never needs to be below this many float32 ulps of max|z| (the residual plane is a float32 difference)


def gpu_polyfit(pkg, z, mask, order, variant, iters=6, c=4.685, min_count=200, min_mask_count=0):
    B, h, w = z.shape
    dz, dm = _dev(z), _dev(mask)
    coef = torch.full((B, 6), 777.0, dtype=torch.float32, device="cuda")
    resid = torch.full((B, h, w), 777.0, dtype=torch.float32, device="cuda")
    rc = pkg._lib.load().vistaf_ftp_test_polyfit(_ptr(dz), _ptr(dm), order, iters, c, min_count, min_mask_count, _ptr(coef), _ptr(resid), B, h, w, variant, None)
    if rc < 0:
        pkg._lib.check(rc)
    return coef.cpu().numpy(), resid.cpu().numpy(), FITV[rc]


def fit_inputs(h, w, seed):
    """three frames: disc mask, smooth quadratic + noise + 5 % gross outliers; mask with holes, the same quantised to 1/64 (tied residuals
    in both medians); disc with holes and NaN inside the mask"""
    rng = np.random.default_rng(seed)
    yy, xx = np.indices((h, w))
    xn, yn = (xx - (w - 1) / 2) / max(1.0, (w - 1) / 2), (yy - (h - 1) / 2) / max(1.0, (h - 1) / 2)
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
        m = [disc, holes, disc & holes][i].copy()
        if i == 2:
            z[rng.random((h, w)) < 0.03] = np.nan
            z[rng.random((h, w)) < 0.002] = np.inf
        zs.append(z)
        ms.append(m.astype(np.uint8))
    return np.stack(zs), np.stack(ms)


def _fit_case(pkg, h, w, variant, seed, orders=(1, 2)):
    z, mask = fit_inputs(h, w, seed)
    inst = None
    for order in orders:
        coef, resid, inst = gpu_polyfit(pkg, z, mask, order, variant)
        for b in range(z.shape[0]):
            c32, r32 = R.polyfit_ref32(z[b], mask[b], order, 6, 4.685)
            c64, r64 = R.polyfit_ref64(z[b], mask[b], order, 6, 4.685)
            fin = np.isfinite(z[b])
            zmax = float(np.abs(z[b][fin]).max())
            assert np.array_equal(np.isfinite(resid[b]), fin), "residual plane finite exactly where z is"
            e32 = max(float(np.abs(r32[fin] - r64[fin]).max()), float(np.abs(c32 - c64).max()))
            dg = max(float(np.abs(resid[b][fin] - r64[fin]).max()), float(np.abs(coef[b] - c64).max()))
            bar = max(FIT_MULT * e32, FIT_FLOOR_ULPS * 2.0 ** -23 * zmax)
            print("fit %4dx%-4d %-9s variant %d order %d frame %d: e32 %.3e  gpu %.3e  bar %.3e  max|z| %.2f" % (h, w, inst, variant, order, b, e32, dg, bar, zmax))
            assert bar <= 1e-5 * zmax, "the bar itself stays far below the end-to-end 1e-4 of peak"
            assert dg <= bar, (h, w, inst, order, b, dg, bar)
            if order == 1:
                assert not coef[b, 3:].any()
    return inst


@pytest.mark.parametrize("shape,expect", LADDER)
def test_polyfit_ladder_production_dispatch(pkg, shape, expect):
    assert _fit_case(pkg, shape[0], shape[1], 0, 31 * shape[0] + shape[1]) == expect


def test_polyfit_generic_kernel_plain_division(pkg):
    """h * w * w = 2^32: the generic kernel's row index is a plain division (magic = 0); coordinate tables still fit (w + h <= 4096)"""
    assert _fit_case(pkg, 1024, 2048, 1, 77, orders=(2,)) == "generic_div"


def test_polyfit_chain_against_per_frame_512(pkg):
    z, mask = fit_inputs(512, 512, 5)
    assert _fit_case(pkg, 512, 512, 2, 5) == "big"
    assert _fit_case(pkg, 512, 512, 1, 5) == "generic"
    for order in (1, 2):
        c1, r1, _ = gpu_polyfit(pkg, z, mask, order, 1)
        c2, r2, _ = gpu_polyfit(pkg, z, mask, order, 2)
        fin = np.isfinite(z)
        peak = float(np.abs(r1[fin]).max())
        d = float(np.abs(r1[fin] - r2[fin]).max())
        print("512x512 order %d: chain vs per-frame %.3e of peak" % (order, d / peak))
        assert d <= 1e-6 * peak and np.abs(c1 - c2).max() <= 1e-6 * max(1.0, np.abs(c1).max())
    with pytest.raises(ValueError):
        gpu_polyfit(pkg, z[:, :128, :128].copy(), mask[:, :128, :128].copy(), 2, 2)


@pytest.mark.parametrize("shape,variant", [((128, 128), 0), ((256, 256), 0), ((190, 300), 0), ((320, 320), 0), ((512, 512), 1), ((512, 512), 2),
                                           ((1, 150), 0), ((150, 1), 0)])
def test_polyfit_degenerate_inputs_give_zero_coefficients_and_z_back(pkg, shape, variant):
    """Specified (robust_polyfit2d's first test; the session's 500-mask-pixel gate of the ramp removal): fewer than min_count fitted pixels,
    or fewer than min_mask_count mask pixels, give six zero coefficients and the residual plane z - 0: z's own bits, NaN where z is NaN."""
    h, w = shape
    rng = np.random.default_rng(h * 7 + w)
    z = (rng.standard_normal((3, h, w)) * 3).astype(np.float32)
    z[0].flat[::7] = np.nan
    mask = np.zeros((3, h, w), np.uint8)
    P = h * w
    mask[0].flat[rng.permutation(P)[:min(P, 1400)]] = 1            # frame 0: enough mask pixels ...
    z[0][mask[0] != 0] = np.where(np.arange(int(mask[0].sum())) < 199, z[0][mask[0] != 0], np.nan)     # ... but 199 finite ones at most
    z[0][(mask[0] != 0) & ~np.isfinite(z[0])] = np.nan
    mask[1].flat[rng.permutation(P)[:min(P, 150)]] = 1             # frame 1: 150 mask pixels
    #                                                                frame 2: empty mask
    coef, resid, _ = gpu_polyfit(pkg, z, mask, 2, variant)
    assert int((np.isfinite(z[0]) & (mask[0] != 0)).sum()) < 200
    assert not coef.any()
    fin = np.isfinite(z)
    assert np.array_equal(np.isnan(resid), ~fin) and (R.bits(resid)[fin] == R.bits(z)[fin]).all()
    if P >= 1000:                                                  # 400 fitted pixels pass min_count = 200 but not min_mask_count = 500
        mask[:] = 0
        z = np.nan_to_num(z, nan=0.5)
        for b in range(3):
            mask[b].flat[rng.permutation(P)[:400]] = 1
        coef, resid, _ = gpu_polyfit(pkg, z, mask, 1, variant, min_mask_count=500)
        assert not coef.any() and (R.bits(resid) == R.bits(z)).all()
        coef, resid, _ = gpu_polyfit(pkg, z, mask, 1, variant, min_mask_count=0)
        assert coef[:, :3].any(axis=1).all()                       # the same planes without the gate are fitted


def test_polyfit_every_instance_is_reached(pkg):
    """production dispatch (variant 0) over the ladder reaches all ten kernels, and variant 1 the generic kernel's plain-division form, which
    production only takes for batches of more than 192 large frames.  Empty masks: the launch is the real one, the fit is skipped."""
    seen = set()
    for (h, w), expect in LADDER:
        inst = gpu_polyfit(pkg, np.zeros((1, h, w), np.float32), np.zeros((1, h, w), np.uint8), 2, 0)[2]
        assert inst == expect, ((h, w), inst, expect)
        seen.add(inst)
    assert seen == set(FITV) - {"generic_div"}, seen
    assert gpu_polyfit(pkg, np.zeros((1, 1024, 2048), np.float32), np.zeros((1, 1024, 2048), np.uint8), 2, 1)[2] == "generic_div"


# =======================================================================================================================================
# plain Gaussian blur

SIGMA_TAPS = [(0.25, 3), (0.5, 5), (0.75, 7), (1.0, 9), (1.25, 11), (1.5, 13), (1.75, 15), (2.0, 17), (2.5, 21), (6.0, 49), (9.0, 73)]
BLUR_SHAPES = [(h, w) for h in (8, 9, 31, 32, 33) for w in (8, 63, 64, 65, 129)] + [(200, 200), (224, 224), (151, 203)]


def gpu_gauss(pkg, src, sigma):
    B, h, w = src.shape
    ds = _dev(src)
    dst = torch.full((B, h, w), 777.0, dtype=torch.float32, device="cuda")
    pkg._lib.check(pkg._lib.load().vistaf_ftp_test_gauss(_ptr(ds), _ptr(dst), float(sigma), B, h, w, None))
    return dst.cpu().numpy()


def blur_inputs(h, w, seed):
    rng = np.random.default_rng(seed)
    noise = rng.standard_normal((h, w)).astype(np.float32)
    imp = np.zeros((h, w), np.float32)
    for y in (0, h - 1, 31, 32):
        for x in (0, w - 1, 63, 64):
            if y < h and x < w:
                imp[y, x] = 1.0                # corners, and both sides of every tile seam the frame has
    wide = (10.0 ** rng.uniform(-30, 30, (h, w)) * rng.choice([-1.0, 1.0], (h, w))).astype(np.float32)
    bad = noise.copy()
    bad[h // 2, w // 3] = np.nan
    bad[h // 4, (2 * w) // 3] = np.inf
    bad[h - 1, w - 1] = -np.inf
    return np.stack([noise, imp, wide]), bad[None]


@pytest.mark.parametrize("sigma,taps", SIGMA_TAPS)
def test_gauss_blur_bit_equal_to_cvlite(pkg, sigma, taps):
    """3 to 15 taps: the one-kernel LDS tile in both radius classes (7 and 9 taps: a one-tap and a three-tap last refill of the row pass);
    17, 21, 49, 73: the row and the column kernel.  Frames narrower than a tile and, for the long kernels, than the radius (cvlite reflects
    repeatedly for len <= r: tests/test_kernel_refs.py)."""
    assert cvlite.gaussian_ksize(sigma) == taps
    for h, w in BLUR_SHAPES:
        src, bad = blur_inputs(h, w, 1000 * taps + h * 31 + w)
        got = gpu_gauss(pkg, src, sigma)
        for b, name in enumerate(("noise", "impulses", "1e-30..1e30")):
            exp = R.blur_ref32(src[b], sigma)
            ndiff = int((R.bits(got[b]) != R.bits(exp)).sum())
            assert ndiff == 0, (taps, h, w, name, ndiff, float(np.abs(got[b] - exp).max()))
        got = gpu_gauss(pkg, bad, sigma)[0]
        exp = R.blur_ref32(bad[0], sigma)
        assert np.array_equal(np.isnan(got), np.isnan(exp)) and np.array_equal(np.isposinf(got), np.isposinf(exp)) and np.array_equal(np.isneginf(got), np.isneginf(exp))
        fin = np.isfinite(exp)
        assert fin.any() or taps > min(h, w)
        assert (R.bits(got)[fin] == R.bits(exp)[fin]).all(), (taps, h, w, "finite part of the NaN / Inf plane")


# =======================================================================================================================================
# the three fused chains through a session, every tap count 3 .. 17

CHAIN_SIGMAS = [s for s, t in SIGMA_TAPS if t <= 17]
HMAP_MULT = 4.0       # as FIT_MULT: the smoothed map sits downstream of the fits


@pytest.fixture(scope="module")
def cal(pkg):
    import test_gpu_parity
    model, neg = pkg.load_calibration(os.path.join(G, "calibration_phase_to_height.json"))
    fm = pkg.load_force_calibration(os.path.join(G, "calibration_height_to_force.json"))["best_model"]
    test_gpu_parity._FORCE_MODEL[0] = fm
    return model, neg, fm


def _scene(pkg, which):
    if which == "224":
        n = 224
        return pkg.synth.reference_frame(n, config=3), pkg.synth.deformed_batch(n, 910, 2, config=3), pkg.synth.roi_circle(n), (n, n)
    import test_config_surface as S
    return S._ref_odd(), np.stack([S._odd(1), S._odd_multi(2)]), S.C151, (151, 203)


def _session(pkg, cal, cfg, ref, circle, frames, fused):
    sensor = pkg.FtpSensor(ref, circle, cfg, cal[0], cal[1], cal[2], max_batch=len(frames))
    sensor._test_set("fused_chains", fused)
    out = sensor.predict_batch(frames)
    torch.cuda.synchronize()
    res = {k: out[k].detach().cpu().numpy().copy() for k in ("height_map_mm", "output_reliable", "scalars", "status")}
    for name, dt in (("iw", torch.float32), ("hmap", torch.float32), ("unitless", torch.float32), ("kept", torch.uint8)):
        res["plane:" + name] = sensor.intermediate(name, len(frames), dt).cpu().numpy().copy()
    res["plane:mu"] = sensor.intermediate("mu", len(frames), torch.float32).cpu().numpy().ravel()[:len(frames)].copy()
    sensor.close()
    return out, res


@pytest.mark.parametrize("which", ["224", "151x203"])
@pytest.mark.parametrize("sigma", CHAIN_SIGMAS)
def test_chains_at_every_tap_count(pkg, cal, which, sigma):
    """pre-blur, reliable-only smoothing and unreliable-region smoothing all at `sigma`: 3 and 5 taps take the small radius class of each
    chain (k_compose_finalize_mm<GF_RSMALL> among them), 7 to 15 the large one, 17 the kernel sequence."""
    import test_gpu_parity
    taps = cvlite.gaussian_ksize(sigma)
    assert taps == dict(SIGMA_TAPS)[sigma] and 3 <= taps <= 17
    ref, frames, circle, (h, w) = _scene(pkg, which)
    cfg = pkg.FtpConfig.scaled(224 if which == "224" else 160)
    cfg.pre_blur_sigma_px = cfg.reliable_smooth_sigma_px = cfg.unreliable_smooth_sigma_px = sigma
    out, a = _session(pkg, cal, cfg, ref, circle, frames, 1)
    _, b = _session(pkg, cal, cfg, ref, circle, frames, 0)
    for k in a:                                                   # fused against the kernel sequence: byte for byte
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (k, taps)
    rs = O.make_reference_state(ref, *circle, cfg)
    orig = O.robust_polyfit2d

    def fit64(z, mask, order=2, iters=6, c=4.685):
        c64, r64 = R.polyfit_ref64(z, mask, order, iters, c)
        nc = 6 if order >= 2 else 3
        if not c64.any():
            return np.zeros(nc, np.float32), np.zeros_like(z, np.float32)
        return c64[:nc].astype(np.float32), (np.asarray(z, np.float32).astype(np.float64) - r64).astype(np.float32)

    problems = []
    for f in range(len(frames)):
        o = O.process_frame(frames[f], rs, cfg, *cal, keep_intermediates=True)
        test_gpu_parity._check_frame(out, f, o, w)
        rel = o["reliable"]
        # the session's iw plane is kept before the median is taken off (the DFT kernel subtracts mu on the fly): subtract it as the oracle does
        iw_g = a["plane:iw"].reshape(-1, h, w)[f] - np.float32(a["plane:mu"].ravel()[f])
        iw_o = o["inter"]["demod"]["inter"]["iw"]
        nd = int((R.bits(iw_g)[rel] != R.bits(iw_o)[rel]).sum())
        print("%s taps %2d frame %d: iw differs from the oracle in %d of %d reliable pixels (max %.3e; mu gpu %r oracle %r)" % (which, taps, f, nd, int(rel.sum()), float(np.abs(iw_g - iw_o)[rel].max()), float(a["plane:mu"].ravel()[f]), o["inter"]["demod"]["inter"]["mu"]))
        if nd:
            problems.append(("iw", taps, f, nd))
        # hmap: downstream of three IRLS fits, so the bar comes from the oracle's own float32-LAPACK error: the same frame with the fits in float64
        O.robust_polyfit2d = fit64
        try:
            o64 = O.process_frame(frames[f], rs, cfg, *cal, keep_intermediates=True)
        finally:
            O.robust_polyfit2d = orig
        hg, h32, h64 = a["plane:hmap"].reshape(-1, h, w)[f], o["inter"]["height_smooth"], o64["inter"]["height_smooth"]
        both = rel & o64["reliable"]
        peak = float(np.abs(h32[rel]).max())
        e32 = float(np.abs(h32 - h64)[both].max()) if o64["flipped"] == o["flipped"] else float("nan")
        dg = float(np.abs(hg - h32)[rel].max())
        bar = max(HMAP_MULT * e32, FIT_FLOOR_ULPS * 2.0 ** -23 * peak)
        print("%s taps %2d frame %d: hmap gpu-oracle %.3e, oracle32-oracle64 %.3e, bar %.3e, peak %.3f, bit-equal %s" % (which, taps, f, dg, e32, bar, peak, bool((R.bits(hg)[rel] == R.bits(h32)[rel]).all())))
        if not (np.isfinite(hg[rel]).all() and bar <= 1e-5 * peak and dg <= bar):
            problems.append(("hmap", taps, f, dg, bar, peak))
    assert not problems, problems
