"""The IRLS fits' window kernel and chained launch (csrc/k_fit.hip: k_robust_polyfit_colwin, k_robust_polyfit_col_retry; session hook "fit_window",
csrc/test_hooks.h; direct hooks csrc/test_hooks_fit.h) against the plain column kernels they stand in for.

The reference is the plain kernel (variant 2 of the hooks), which tests/test_kernels_direct.py ties to the float64 fit.  The comparison is on BIT
PATTERNS of the coefficients and of the whole residual plane, NaN layout included: a thread of the window kernel owns the same rows of the same
column in the same lane and adds its finite samples in the same order, so every sum and every order statistic is the plain kernel's.  Outputs are
filled with a sentinel before every call.  Frames are launched in batches of three with fitting and non-fitting frames mixed.

Geometry (polyfit_variant of k_fit.hip): cols_pad = w rounded up to 64, groups = min(1024 / cols_pad, h), a thread (column x, group g) owns the rows
g + groups * k, k < need = ceil(h / groups).  The window instance keeps RP slots from the thread's first mask row on; a frame is flagged when some
thread's mask rows span more than RP slots (`flags` below restates the rule)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import kernel_refs as R
import test_kernels_direct as KD

pytestmark = pytest.mark.gpu
_dev, _ptr = KD._dev, KD._ptr
SENTINEL = 777.0
FITV = KD.FITV + ["win16", "win32", "win48", "win56", "win32_g4", "win48_g4", "win56_g4"]        # kernels.hpp: FitVariant
# (h, w): groups, rows of a unit, slots of the plain instance, slots of the window instance, window instance
GEOM = {(224, 224): (4, 56, 56, 48, "win48_g4"), (165, 300): (3, 55, 56, 48, "win48"), (151, 203): (4, 38, 48, 32, "win32_g4")}


PLAIN_OF = {"win48_g4": "col56_g4", "win48": "col56", "win32_g4": "col48_g4"}       # the plain instance a window instance stands in for


def flags(mask, groups, rp):
    """[B] 1 where some thread's mask rows span more than rp slots: per column and row group, last slot - first slot + 1 over the mask pixels"""
    out = []
    for m in mask:
        over = False
        for g in range(groups):
            sub = m[g::groups] != 0                       # [slots, w]
            has = sub.any(axis=0)
            first = sub.argmax(axis=0)
            last = sub.shape[0] - 1 - sub[::-1].argmax(axis=0)
            over |= bool(((last - first + 1)[has] > rp).any())
        out.append(int(over))
    return np.array(out, np.int32)


def polyfit(pkg, z, mask, order, variant, min_mask_count=0):
    B, h, w = z.shape
    dz, dm = _dev(z), _dev(mask)
    coef = torch.full((B, 6), SENTINEL, dtype=torch.float32, device="cuda")
    resid = torch.full((B, h, w), SENTINEL, dtype=torch.float32, device="cuda")
    need = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    rc = pkg._lib.load().vistaf_ftp_test_polyfit_window(_ptr(dz), _ptr(dm), order, 6, 4.685, 200, min_mask_count, _ptr(coef), _ptr(resid), B, h, w, variant,
                                                        _ptr(need), None)
    if rc < 0:
        pkg._lib.check(rc)
    return FITV[rc], coef.cpu().numpy(), resid.cpu().numpy(), need.cpu().numpy()


def chain(pkg, z, mask, orders, gates, variant):
    B, h, w = z.shape
    dz, dm = _dev(z), _dev(mask)
    coef = torch.full((B, 6), SENTINEL, dtype=torch.float32, device="cuda")
    r1 = torch.full((B, h, w), SENTINEL, dtype=torch.float32, device="cuda")
    r2 = torch.full((B, h, w), SENTINEL, dtype=torch.float32, device="cuda")
    need = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    rc = pkg._lib.load().vistaf_ftp_test_polyfit_chain(_ptr(dz), _ptr(dm), orders[0], orders[1], 6, 4.685, 200, gates[0], gates[1], _ptr(coef), _ptr(r1), _ptr(r2),
                                                       B, h, w, variant, _ptr(need), None)
    if rc < 0:
        pkg._lib.check(rc)
    return FITV[rc], coef.cpu().numpy(), r1.cpu().numpy(), r2.cpu().numpy(), need.cpu().numpy()


def same_bits(tag, got, exp):
    assert got.shape == exp.shape and np.array_equal(R.bits(got), R.bits(exp)), (tag, int((R.bits(got) != R.bits(exp)).sum()))


def surface(h, w, seed):
    """a smooth quadratic + noise + 5 % gross outliers, finite everywhere"""
    rng = np.random.default_rng(seed)
    yy, xx = np.indices((h, w))
    xn, yn = (xx - (w - 1) / 2) / ((w - 1) / 2), (yy - (h - 1) / 2) / ((h - 1) / 2)
    cf = rng.uniform(-2, 2, 6)
    z = cf[0] * xn + cf[1] * yn + 3.0 * cf[2] + cf[3] * xn * xn + cf[4] * xn * yn + cf[5] * yn * yn + 0.02 * rng.standard_normal((h, w))
    o = rng.random((h, w)) < 0.05
    z[o] += rng.choice([-1.0, 1.0], int(o.sum())) * rng.uniform(2, 6, int(o.sum()))
    return z.astype(np.float32)


def rows_mask(h, w, lo, hi):
    m = np.zeros((h, w), np.uint8)
    m[lo:hi + 1] = 1
    return m


def disc_rows(n, lo, hi):
    """a disc of n x n whose rows are exactly lo..hi"""
    yy, xx = np.indices((n, n))
    cy, r = (lo + hi) / 2.0, (hi - lo) / 2.0 + 0.25
    return (((yy - cy) ** 2 + (xx - (n - 1) / 2.0) ** 2) <= r * r).astype(np.uint8)


def frames_224():
    """[(name, z, mask)] at 224 x 224: four groups, 56 rows per unit, the window keeps 48"""
    n = 224
    out = []
    disc = disc_rows(n, 17, 207)                                # 191 rows: every central thread has extent 48
    assert disc.any(axis=1).nonzero()[0][[0, -1]].tolist() == [17, 207]
    for s in range(4):                                          # the groups start at different slots
        out.append(("disc+%d" % s, surface(n, n, 10 + s), np.roll(disc, s, axis=0)))
    extra = disc.copy()
    extra[13, 111] = 1                                          # group 1 of column 111: rows 13, 17, ..., 205 = 49 slots; no other thread changes
    out.append(("extent49", surface(n, n, 20), extra))
    zs, ms = KD.fit_inputs(n, n, 5)                             # holes, quantised values, NaN and Inf inside the window
    for i in range(3):
        out.append(("kind%d" % i, zs[i], ms[i] & disc))
    band = np.zeros((n, n), np.uint8)                           # the first row moves by one row every six columns: u0 differs across a wave
    for x in range(n):
        band[10 + x // 6:10 + x // 6 + 185, x] = 1
    out.append(("band", surface(n, n, 21), band))
    out.append(("rows40..223", surface(n, n, 22), rows_mask(n, n, 40, 223)))      # first slot 10 > need - RP = 8: the window would run past the last row
    z = surface(n, n, 23)                                       # NaN under the mask at a unit's first and last mask row
    for x in (60, 111, 112, 170):
        ys = disc[:, x].nonzero()[0]
        z[ys[0], x] = np.nan
        z[ys[-1], x] = np.nan
        z[ys[1], x] = np.inf
    out.append(("nan_ends", z, disc))
    out.append(("full", surface(n, n, 24), np.ones((n, n), np.uint8)))            # extent 56 everywhere
    out.append(("empty", surface(n, n, 25), np.zeros((n, n), np.uint8)))
    few = np.zeros((n, n), np.uint8)
    few[100:110, 50:65] = 1                                     # 150 fitted pixels: below min_count
    out.append(("few150", surface(n, n, 26), few))
    right = np.zeros((n, n), np.uint8)
    right[40:201, 192:] = 1                                     # only columns >= 192: the half-empty wave of every group
    out.append(("cols>=192", surface(n, n, 27), right))
    tall = np.zeros((n, n), np.uint8)
    tall[:, 100:103] = 1                                        # a non-fitting frame whose mask is small
    out.append(("tall", surface(n, n, 28), tall))
    return out


def frames_other(h, w, seed):
    groups, need, _, rp, _ = GEOM[(h, w)]
    fit_rows = groups * (rp - 1)                                # rows lo .. lo + fit_rows - 1 span at most rp slots in every group
    lo = 2 * groups + 1
    fit = rows_mask(h, w, lo, lo + fit_rows - 1)
    zs, ms = KD.fit_inputs(h, w, seed)
    return [("fit", surface(h, w, seed + 1), fit), ("full", surface(h, w, seed + 2), np.ones((h, w), np.uint8)), ("holes_nan", zs[2], ms[2] & fit)]


def check_frames(pkg, h, w, frames, min_mask_count=0):
    groups, _, _, rp, inst_name = GEOM[(h, w)]
    seen = set()
    for k in range(0, len(frames), 3):
        part = frames[k:k + 3]
        names = [f[0] for f in part]
        z, mask = np.stack([f[1] for f in part]), np.stack([f[2] for f in part])
        want_need = flags(mask, groups, rp)
        seen |= set(want_need.tolist())
        for order in (1, 2):
            inst, cref, rref, nref = polyfit(pkg, z, mask, order, 2, min_mask_count)
            assert inst == PLAIN_OF[inst_name], (names, inst)
            assert (nref == -1).all(), "the plain kernel writes no flags"
            assert (cref != SENTINEL).all() and (rref != SENTINEL).all()
            inst, c0, r0, n0 = polyfit(pkg, z, mask, order, 0, min_mask_count)
            assert inst == inst_name, (names, inst)
            assert np.array_equal(n0, want_need), (names, n0, want_need)
            same_bits((names, order, "dispatch coef"), c0, cref)
            same_bits((names, order, "dispatch resid"), r0, rref)
            inst, c1, r1, n1 = polyfit(pkg, z, mask, order, 1, min_mask_count)
            assert inst == inst_name and np.array_equal(n1, want_need), (names, n1, want_need)
            for b, name in enumerate(names):
                if want_need[b]:
                    assert (c1[b] == SENTINEL).all() and (r1[b] == SENTINEL).all(), (name, "a flagged frame's outputs stay untouched")
                else:
                    same_bits((name, order, "window coef"), c1[b], cref[b])
                    same_bits((name, order, "window resid"), r1[b], rref[b])
    return seen


# =======================================================================================================================================
# the hooks

def test_the_hooks_have_matching_signatures(pkg):
    """csrc/test_hooks_fit.h against _lib.FIT_WINDOW_SIGNATURES: the same functions, and a pointer where the header has one"""
    text = open(os.path.join(os.path.dirname(pkg.__file__), "csrc", "test_hooks_fit.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    protos = {name: [p.strip() for p in params.split(",")] for name, params in re.findall(r"\bint\s+(vistaf_\w+)\s*\(([^()]*)\)\s*;", text)}
    table = pkg._lib.FIT_WINDOW_SIGNATURES
    assert sorted(protos) == sorted(table) and len(protos) == 3
    for name, params in protos.items():
        restype, argtypes = table[name]
        assert restype is ctypes.c_int and len(argtypes) == len(params), name
        for p, a in zip(params, argtypes):
            if "*" in p:
                assert a is ctypes.c_void_p, (name, p)
            else:
                assert a is (ctypes.c_float if p.startswith("float") else ctypes.c_int), (name, p)


def test_the_flag_rule_on_hand_made_masks():
    """`flags` itself: 48 slots pass, 49 do not, and one pixel decides"""
    m = np.zeros((1, 224, 224), np.uint8)
    m[0, 17:208, 5] = 1
    assert flags(m, 4, 48).tolist() == [0]
    m[0, 13, 5] = 1
    assert flags(m, 4, 48).tolist() == [1] and flags(m, 4, 56).tolist() == [0]
    assert flags(np.zeros((2, 8, 8), np.uint8), 4, 1).tolist() == [0, 0]


# =======================================================================================================================================
# the window kernel, alone and with the kernel behind it

def test_window_224(pkg):
    frames = frames_224()
    by_name = {f[0]: f for f in frames}
    groups, _, _, rp, _ = GEOM[(224, 224)]
    want = {f[0]: int(flags(f[2][None], groups, rp)[0]) for f in frames}
    assert [n for n, v in want.items() if v] == ["extent49", "full", "tall"], want
    # mixed batches: a flagged frame sits among fitting ones in three of the six launches
    order = ["disc+0", "extent49", "disc+1", "disc+2", "full", "disc+3", "kind0", "kind1", "kind2", "band", "tall", "rows40..223", "nan_ends", "empty", "few150",
             "cols>=192"]
    assert sorted(order) == sorted(by_name)
    assert check_frames(pkg, 224, 224, [by_name[n] for n in order]) == {0, 1}


def test_window_224_mask_count_gate(pkg):
    """min_mask_count = 500 with 400 and with 600 mask pixels (and a frame the window does not take)"""
    n = 224
    m400, m600 = np.zeros((n, n), np.uint8), np.zeros((n, n), np.uint8)
    m400[60:80, 100:120] = 1
    m600[60:80, 100:130] = 1
    frames = [("400", surface(n, n, 40), m400), ("full", surface(n, n, 41), np.ones((n, n), np.uint8)), ("600", surface(n, n, 42), m600)]
    check_frames(pkg, n, n, frames, min_mask_count=500)
    z, mask = np.stack([f[1] for f in frames]), np.stack([f[2] for f in frames])
    _, coef, resid, _ = polyfit(pkg, z, mask, 1, 0, 500)
    assert not coef[0].any() and np.array_equal(R.bits(resid[0]), R.bits(z[0])) and coef[2, :3].any() and coef[1, :3].any()


@pytest.mark.parametrize("shape", [(165, 300), (151, 203)])
def test_window_other_ladder_steps(pkg, shape):
    """three groups with the runtime row stride (<56,0> -> <48,0>) and the four-group step <48,4> -> <32,4>: a fitting mask, a non-fitting one, one
    with holes and NaN"""
    h, w = shape
    assert check_frames(pkg, h, w, frames_other(h, w, 7 * h + w)) == {0, 1}


def test_no_window_at_128(pkg):
    """128 x 128 takes the 16-slot kernel, the smallest step: no window instance, no flags, the same bits"""
    assert FITV[pkg._lib.load().vistaf_ftp_test_polyfit_window_instance(3, 128, 128)] == "col16"
    for (h, w), (_, _, _, _, name) in GEOM.items():
        assert FITV[pkg._lib.load().vistaf_ftp_test_polyfit_window_instance(3, h, w)] == name
    z, mask = KD.fit_inputs(128, 128, 3)
    for order in (1, 2):
        inst, cref, rref, _ = polyfit(pkg, z, mask, order, 2)
        assert inst == "col16"
        inst, c0, r0, n0 = polyfit(pkg, z, mask, order, 0)
        assert inst == "col16" and (n0 == -1).all()
        same_bits("128 coef", c0, cref)
        same_bits("128 resid", r0, rref)
    with pytest.raises(ValueError):
        polyfit(pkg, z, mask, 2, 1)


# =======================================================================================================================================
# the chained launch

def _chain_case(pkg, tag, z, mask, gates=(500, 0), orders=(1, 2), two_calls=False):
    h, w = z.shape[1:]
    groups, _, _, rp, inst_name = GEOM[(h, w)]
    want_need = flags(mask, groups, rp)
    _, cref, r1ref, r2ref, _ = chain(pkg, z, mask, orders, gates, 2)
    assert (r1ref != SENTINEL).all() and (r2ref != SENTINEL).all()
    if two_calls:                                      # variant 2 of the chain hook is two plain launches: spelled out once
        _, ca, ra, _ = polyfit(pkg, z, mask, orders[0], 2, gates[0])
        _, cb, rb, _ = polyfit(pkg, ra, mask, orders[1], 2, gates[1])
        same_bits((tag, "two calls r1"), r1ref, ra)
        same_bits((tag, "two calls r2"), r2ref, rb)
        same_bits((tag, "two calls coef"), cref, cb)
    inst, c0, r10, r20, n0 = chain(pkg, z, mask, orders, gates, 0)
    assert inst == inst_name and np.array_equal(n0, want_need), (tag, inst, n0, want_need)
    same_bits((tag, "coef"), c0, cref)
    same_bits((tag, "resid1"), r10, r1ref)
    same_bits((tag, "resid2"), r20, r2ref)
    inst, c1, r11, r21, n1 = chain(pkg, z, mask, orders, gates, 1)
    assert np.array_equal(n1, want_need)
    for b in range(z.shape[0]):
        if want_need[b]:
            assert (c1[b] == SENTINEL).all() and (r11[b] == SENTINEL).all() and (r21[b] == SENTINEL).all(), tag
        else:
            same_bits((tag, b, "window coef"), c1[b], cref[b])
            same_bits((tag, b, "window resid1"), r11[b], r1ref[b])
            same_bits((tag, b, "window resid2"), r21[b], r2ref[b])
    return r1ref, r2ref, cref


def test_chain_against_two_plain_launches(pkg):
    n = 224
    fr = {f[0]: f for f in frames_224()}
    pick = lambda names: (np.stack([fr[k][1] for k in names]), np.stack([fr[k][2] for k in names]))
    _chain_case(pkg, "fitting", *pick(["disc+0", "kind2", "band"]), two_calls=True)
    _chain_case(pkg, "non-fitting", *pick(["full", "extent49", "tall"]))
    _chain_case(pkg, "mixed", *pick(["nan_ends", "full", "rows40..223"]))
    _chain_case(pkg, "mixed, orders (2, 1)", *pick(["disc+1", "extent49", "kind1"]), orders=(2, 1))
    # the first fit gated off (400 mask pixels < 500) and on (600), beside an empty mask: the second fit runs on z itself / on z - plane
    m400, m600 = np.zeros((n, n), np.uint8), np.zeros((n, n), np.uint8)
    m400[60:80, 100:120] = 1
    m600[60:80, 100:130] = 1
    z = np.stack([surface(n, n, 50), surface(n, n, 51), surface(n, n, 52)])
    r1, r2, coef = _chain_case(pkg, "gates", z, np.stack([m400, m600, np.zeros((n, n), np.uint8)]))
    assert np.array_equal(R.bits(r1[0]), R.bits(z[0])) and not np.array_equal(R.bits(r1[1]), R.bits(z[1])) and coef[0].any() and coef[1].any() and not coef[2].any()


def test_chain_sample_that_the_first_fit_turns_into_inf(pkg):
    """|z| near FLT_MAX under the mask, the rest of the plane at -1e33: z - fit overflows, the second fit drops the sample as a reload would"""
    n = 224
    disc = disc_rows(n, 17, 207)
    z = (surface(n, n, 60).astype(np.float64) * 1e30 - 1e33).astype(np.float32)
    z[100, 100] = np.finfo(np.float32).max               # + 1e33 rounds to Inf: half an ulp of FLT_MAX is 1e31
    z[101, 140] = np.finfo(np.float32).max
    zz = np.stack([z, surface(n, n, 61), z])
    mask = np.stack([disc, disc, np.ones((n, n), np.uint8)])
    r1, r2, _ = _chain_case(pkg, "inf", zz, mask, gates=(500, 0))
    assert np.isfinite(zz).all() and np.isposinf(r1[0, 100, 100]) and np.isposinf(r1[0, 101, 140]) and np.isposinf(r2[0, 100, 100])
    assert np.isfinite(r2[0][disc != 0]).sum() == int(disc.sum()) - 2


# =======================================================================================================================================
# sessions

def _session(pkg, n, plane_order=None, nb=8):
    g = os.path.join(os.path.dirname(__file__), "golden")
    model, neg = pkg.load_calibration(os.path.join(g, "calibration_phase_to_height.json"))
    fm = pkg.load_force_calibration(os.path.join(g, "calibration_height_to_force.json"))["best_model"]
    cfg = pkg.FtpConfig.scaled(n)
    if plane_order is not None:
        cfg.plane_order_for_removal = plane_order
    ref = pkg.synth.reference_frame(n, config=3)                    # the benchmark's frames
    frames = pkg.synth.deformed_batch(n, 0, nb, config=3)
    sensor = pkg.FtpSensor(ref, pkg.synth.roi_circle(n), cfg, model, neg, fm, max_batch=nb)
    res = []
    for tier in (1, 0, 1):
        sensor._test_set("fit_window", tier)
        out = {k: v.cpu().numpy().copy() for k, v in sensor.predict_batch(frames).items()}
        torch.cuda.synchronize()
        for name in ("hmap", "unitless"):
            out["plane:" + name] = sensor.intermediate(name, nb, torch.float32).cpu().numpy().copy()
        out["plane:coef"] = sensor.intermediate("coef", nb, torch.float32).cpu().numpy().copy()
        if len(res) == 0:
            need = sensor.intermediate("fit_need", nb, torch.int32).cpu().numpy().copy()
        res.append(out)
    sensor.close()
    for other in (res[0], res[2]):
        assert set(other) == set(res[1]) and {"height_map_mm", "scalars", "status"} <= set(other)
        for key, want in res[1].items():
            assert other[key].tobytes() == want.tobytes(), (n, key)
    return need


@pytest.mark.parametrize("n", [224, 200])
def test_sessions_give_the_same_bytes_with_and_without_the_tier(pkg, n):
    """eight benchmark frames with fit_window 1, 0 and 1 again: every output byte for byte, and no frame took the kernel behind the window"""
    need = _session(pkg, n)
    print("fit_need", need.tolist())
    assert (need == 0).all()


def test_session_without_the_ramp_removal(pkg):
    """plane_order_for_removal = 0: no chained launch, so no window kernel: the copy and one plain launch per fit as before"""
    assert (_session(pkg, 224, plane_order=0, nb=4) == -1).all()
