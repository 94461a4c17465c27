"""The register-resident selection kernel (csrc/k_select.hip: k_select_resident) at the plane sizes where its slot bookkeeping can go wrong,
the streaming kernel forced at small sizes, the chained form (a threshold and the median of the elements up to it in one launch) and the
`select_resident` tier through sessions in flight.  Every comparison is bit-equal (kernel_refs.same_result against NumPy, raw bits between
two GPU paths); counts are exact."""
import numpy as np
import pytest
import torch

import kernel_refs as R
import test_kernels_direct as D

gpu = pytest.mark.gpu

# kernels.hpp: SelectVariant
SELV = {"big": 0, "stream": 1, "res16": 2, "res32": 3, "res49": 4, "res64": 5}
# (P, the instance variant 1 takes).  Slot boundaries of the ladder 16 / 32 / 49 / 64 slots of 1024 elements: the 16-slot instance AT its
# boundary (16384) and the 32-slot one just above it (16385); the 32-slot instance just BELOW its boundary (32767) and the 49-slot one just
# above it (32769); the 49-slot instance's boundary is 50176 (test_kernels_direct runs it), just ABOVE it (50177) is the 64-slot one with
# a single element in its 50th slot; the 64-slot instance below, at and above its boundary, the last being the streaming kernel's.
# 1025 has one element in the second slot and fourteen empty slots.
RESIDENT_SIZES = [(1025, "res16"), (16384, "res16"), (16385, "res32"), (32767, "res32"), (32769, "res49"), (50177, "res64"),
                  (65535, "res64"), (65536, "res64"), (65537, "stream")]


def _b(x):
    return int(R.bits(x).ravel()[0])


def _instance(pkg, B, P, nreq, variant):
    return pkg._lib.load().vistaf_ftp_test_select_instance(B, P, nreq, variant)


@gpu
@pytest.mark.parametrize("P,inst", RESIDENT_SIZES)
def test_resident_kernel_at_slot_boundaries(pkg, P, inst):
    assert _instance(pkg, 3, P, 3, 1) == SELV[inst]
    D._check_select(pkg, P, 1, 3, 3000 + P % 997)


@gpu
@pytest.mark.parametrize("P", [1023, 8193])
def test_streaming_kernel_forced_at_small_sizes(pkg, P):
    """variant 3: k_select whatever the size, so the kernel of planes beyond 65536 pixels stays covered where a reference is cheap"""
    assert _instance(pkg, 3, P, 3, 3) == SELV["stream"] and _instance(pkg, 3, P, 3, 1) == SELV["res16"]
    D.HIST_BITS.setdefault(3, D.HIST_BITS[1])           # _check_select aims its bucket-boundary inputs by variant: 3 has variant 1's histogram
    D._check_select(pkg, P, 3, 3, 4000 + P % 997)


# =======================================================================================================================================
# chained form

CHAIN_QS = [8.0, 50.0, 92.0]


def chain_cases(P, seed):
    """[(name, vals float32[P], mask uint8[P])]: every selection_inputs plane under a full and under a random mask (signed_zeros puts the
    50th percentile on a zero, all_equal makes every element equal the threshold, ties_at_rank_* put it inside a run of equal values), and
    planes with 0, 1 and 2 valid elements (the empty one hands a NaN threshold to the second request)"""
    rng = np.random.default_rng(seed + 7)
    inputs = D.selection_inputs(P, seed)
    cases = []
    for name, v in inputs.items():
        cases.append((name + "/full", v, np.ones(P, np.uint8)))
        cases.append((name + "/own", v, (rng.random(P) < 0.7).astype(np.uint8)))
    for nv in (0, 1, 2):
        cases.append(("valid_%d_by_mask" % nv, inputs["sorted"], D._count_mask(P, nv, rng)))
        f = np.full(P, np.nan, np.float32)
        f[rng.permutation(P)[:nv]] = np.float32(-3.5)
        cases.append(("valid_%d_by_nan" % nv, f, np.ones(P, np.uint8)))
    return cases


def chain_ref(vals, mask, q, use_abs):
    """(threshold, median of the elements <= threshold, count of the first selection): the reference pair"""
    first, n, _ = R.select_ref(vals, mask, [q], use_abs)
    second, _, _ = R.select_ref(vals, mask, [R.MEDIAN], use_abs, first[0])
    return first[0], second[0], n


def gpu_select_chained(pkg, vals, mask, use_abs, reqs):
    """vals [B, P], mask [B, P] -> (out [nreq, B] float32, counts [B], instance)"""
    B, P = vals.shape
    dv, dm = D._dev(vals), D._dev(mask)
    dr = D._dev(np.array([R.request_value(q) for q in reqs], np.float32))
    out = torch.full((len(reqs), B), 12345.0, dtype=torch.float32, device="cuda")
    cnt = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    rc = pkg._lib.load().vistaf_ftp_test_select_chained(D._ptr(dv), D._ptr(dm), P, int(use_abs), D._ptr(dr), len(reqs), D._ptr(out), D._ptr(cnt),
                                                        B, P, None)
    if rc < 0:
        pkg._lib.check(rc)
    return out.cpu().numpy(), cnt.cpu().numpy(), rc


@pytest.mark.parametrize("P", [1025, 8193])
def test_chain_reference_pair_runs_on_every_case(P):
    """no GPU: the reference pair is defined on every case, the NaN threshold of an empty plane included, and the cases hold what they claim"""
    cases = chain_cases(P, 5000 + P)
    hit_zero = hit_all = hit_nan = 0
    for name, v, m in cases:
        for q in CHAIN_QS:
            for use_abs in (False, True):
                thr, med, n = chain_ref(v, m, q, use_abs)
                comp = R.select_compact(v, m, use_abs)
                assert n == comp.size and (n > 0 or np.isnan(thr))
                if np.isnan(thr):
                    hit_nan += 1
                    assert np.isnan(med)
                else:
                    kept = comp[comp <= thr]
                    assert np.isnan(med) == (kept.size == 0)
                    hit_zero += int(thr == 0 and name.startswith("signed_zeros"))
                    hit_all += int(name.startswith("all_equal") and kept.size == n and n > 0)
    assert hit_zero and hit_all and hit_nan


@gpu
@pytest.mark.parametrize("P", [1025, 8193])
def test_chained_pair_against_reference_and_two_launches(pkg, P):
    B = 3
    cases = chain_cases(P, 5000 + P)
    while len(cases) % B:
        cases.append(cases[len(cases) % 5])
    nbad, ncases, worst = 0, 0, []
    for g0 in range(0, len(cases), B):
        vals = np.stack([c[1] for c in cases[g0:g0 + B]])
        mask = np.stack([c[2] for c in cases[g0:g0 + B]])
        for q in CHAIN_QS:
            for use_abs in (False, True):
                out, cnt, inst = gpu_select_chained(pkg, vals, mask, use_abs, [q, R.MEDIAN])
                assert inst == SELV["res16"]
                thr2, cnt2 = D.gpu_select(pkg, vals, mask, P, None, use_abs, [q], 1)
                med2, _ = D.gpu_select(pkg, vals, mask, P, thr2[:, 0], use_abs, [R.MEDIAN], 1)
                for b in range(B):
                    thr, med, n = chain_ref(vals[b], mask[b], q, use_abs)
                    ncases += 1
                    ok = int(cnt[b]) == n and int(cnt2[b]) == n and R.same_result(out[0, b], thr) and R.same_result(out[1, b], med)
                    ok = ok and _b(out[0, b]) == _b(thr2[b, 0]) and _b(out[1, b]) == _b(med2[b, 0])
                    if not ok:
                        nbad += 1
                        worst.append((cases[g0 + b][0], q, "abs" if use_abs else "", "chained", [hex(int(x)) for x in R.bits(out[:, b])],
                                      "two launches", hex(_b(thr2[b, 0])), hex(_b(med2[b, 0])),
                                      "reference", hex(_b(thr)), hex(_b(med)), "count", int(cnt[b]), int(cnt2[b]), n))
    print("chained P=%d: %d frame-calls, %d wrong" % (P, ncases, nbad))
    for wv in worst[:4]:
        print("  wrong:", wv)
    assert nbad == 0, worst[:12]


@gpu
def test_chained_hook_refuses_planes_beyond_the_largest_instance(pkg):
    """65537 pixels: no resident instance; the hook launches nothing and says so (a session then runs one launch per request)"""
    P = 65537
    assert _instance(pkg, 1, P, 2, 1) == SELV["stream"]
    with pytest.raises(ValueError):
        gpu_select_chained(pkg, np.zeros((1, P), np.float32), np.ones((1, P), np.uint8), False, [50.0, R.MEDIAN])


# =======================================================================================================================================
# the tier through sessions

@gpu
def test_select_resident_tier_gives_the_same_bits_with_sessions_in_flight(pkg):
    """three sessions in flight at 224 x 224 (batch 4, each on its own stream) with the resident kernel and the chained core pair, and with
    the streaming kernel and one launch per selection: same outputs, same thresholds"""
    import test_gpu_parity as T
    import os
    n, nb = 224, 4
    model, neg = pkg.load_calibration(os.path.join(T.G, "calibration_phase_to_height.json"))
    fm = pkg.load_force_calibration(os.path.join(T.G, "calibration_height_to_force.json"))["best_model"]
    cfg = pkg.FtpConfig.scaled(n)
    frames = [torch.from_numpy(pkg.synth.deformed_batch(n, 700 + 100 * k, nb, config=3)).cuda() for k in range(3)]
    streams = [torch.cuda.Stream() for _ in range(3)]
    res = {}
    for tier in (1, 0):
        sensors = [T._sensor(pkg, (model, neg, fm), n, cfg, nb, config=3)[1] for _ in range(3)]
        for s in sensors:
            s._test_set("select_resident", tier)
        outs = [None] * 3
        for rnd in range(2):
            for k in range(3):
                with torch.cuda.stream(streams[k]):
                    outs[k] = sensors[k].predict_batch(frames[k], outs[k])
        torch.cuda.synchronize()
        got = []
        for k in range(3):
            assert (outs[k]["status"].cpu().numpy() == 0).all()
            d = {key: outs[k][key].cpu().numpy().copy() for key in ("height_map_mm", "scalars", "output_reliable")}
            for name in ("core_thr", "core_med"):
                d[name] = sensors[k].intermediate(name, nb, torch.float32).cpu().numpy().ravel()[:nb].copy()
            got.append(d)
            sensors[k].close()
        res[tier] = got
    for k in range(3):
        for key in res[1][k]:
            assert res[1][k][key].tobytes() == res[0][k][key].tobytes(), (k, key)
        assert np.isfinite(res[1][k]["core_thr"]).all() and np.isfinite(res[1][k]["core_med"]).all()
