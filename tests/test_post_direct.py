"""The back end of a predict launched directly (csrc/test_hooks_post.h): the reliable-only smoothing, the sign flip, the hole stage's glue, the
frontier taper / composition / mm curve, the blob filter with the force tail and the output copy, and the three force tails, each production
launcher on the hand-made planes of tests/post_cases.py against the NumPy references there (the oracle's own stage functions in the order of
process_frame).

Exact by bit pattern: unitless, hmap, masks, counts, labels, kept, gmax, area, max depth, every index and flag.  Two outputs cannot be:
  depth   float64 exp on the device against NumPy's, then one cast: got == float32(r), or |got - r| <= 1/2 ulp32(r) (1 + 2^-20) for the float64
          reference r (post_cases.within_depth_rule); cand must then be roi & finite(got) & got > 0 and gmax the largest of those;
  volume  the kernels round a float64 sum once to float32: the float32 behind S[0] is the correctly rounded exact sum (math.fsum) or its
          neighbour; S[0] itself is that float32 through the kernels' own expression, bit for bit; the force is predict_force_from_volume at the
          kernel's own volume under the depth rule.
The CPU tests (unmarked) pin every restatement of post_cases.py to the oracle's function and assert that each case reaches the branch it is
named after."""
import ctypes
import os
import re

import numpy as np
import pytest

import mask_cases as M
import post_cases as C
from oracle import cvlite
from oracle import ftp_oracle as O

E_INVALID = -1
NSCAL = 16
SENTINEL = -12345.0


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _full(shape, value, dtype):
    import torch
    return torch.full(shape, value, dtype=dtype, device="cuda")


def _diff32(got, want):
    bad = np.argwhere(C.bits32(got) != C.bits32(want))
    i = tuple(bad[0])
    return "%d elements differ, first at %r: got %r (%08x), want %r (%08x)" % (len(bad), i, got[i], C.bits32(got)[i], want[i], C.bits32(want)[i])


def assert_bits32(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(C.bits32(got), C.bits32(want)), (what, _diff32(got, want))


def assert_equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        i = tuple(bad[0])
        raise AssertionError((what, "%d elements differ, first at %r: got %r, want %r" % (len(bad), i, got[i], want[i])))


_CACHE = {}


def cached(key, make):
    """a reference computed once, shared by the tests, never written to"""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# =======================================================================================================================================
# CPU: the curve and the tail restatements against the oracle, and what the tail frames reach

def test_curve_restatement_equals_the_oracle_models():
    v = np.array([0.0, -0.0, 1e-9, 0.015625, 0.4375, 0.5, 1.0, 2.75, 11.0, -3.0], np.float64)
    for cv in C.CURVES:
        model = C.curve_model(*cv)
        for x in v:
            assert C.bits64(C.ref_curve(*cv, x)) == C.bits64(O.predict_force_from_volume(model, float(x))), (cv, x)
    hs = np.array([[0.0, -0.0, -0.5, 0.25, np.nan, np.inf, -np.inf, -3.0, -1e-30]], np.float32)
    for cv in C.CURVES[4:]:
        for use_neg in (False, True):
            with np.errstate(over="ignore", invalid="ignore"):
                want = O.height_unitless_to_depth_mm(hs, C.curve_model(*cv), use_neg)
                got = C.ref_to_mm(hs, cv, use_neg).astype(np.float32)
            assert_bits32(got, want, (cv, use_neg))


def base_of(kind):
    return kind.rstrip("0123456789")


def tail_catalogue(P):
    """name -> (height, roi_frame, unitless, {mode: reference}) at P pixels; modes: `full` (isfinite ROI, unitless), `roi` (the frame's own ROI, no
    unitless)"""
    def make():
        rs = C.tail_roi_static(P)
        cat = {}
        for kind in C.tail_kinds(P):
            h, rf, u = C.tail_frame(kind, P)
            for a in (h, rf, u):
                a.setflags(write=False)
            cat[kind] = (h, rf, u, {"full": C.ref_tail(h, None, u, rs), "roi": C.ref_tail(h, rf, None, rs)})
        return rs, cat
    return cached(("tail", P), make)


def test_tail_restatement_equals_the_oracle_volume():
    for P in C.TAIL_P[:-1]:
        rs, cat = tail_catalogue(P)
        for kind, (h, rf, u, refs) in cat.items():
            for mode, roi in (("full", np.isfinite(h)), ("roi", rf != 0)):
                r = refs[mode]
                with np.errstate(invalid="ignore"):
                    vol, area, maxd = O.depth_map_to_volume_cm3(h, roi, C.TAIL_MM_PER_PX, C.TAIL_EPS)
                assert area == r["area"] and maxd == r["maxd"], (P, kind, mode)
                if float(r["vol32"]) == r["vol_exact"]:
                    # dyadic depths, a dyadic pixel area: the oracle's float32 pairwise sum and product are exact, like the exact sum here
                    assert vol == C.volume_cm3(r["vol32"], r["area_px"]), (P, kind, mode)
                else:
                    # the frames with a depth one ulp above eps: a float32 sum of positive terms, pairwise or in any other order, is off by at
                    # most one rounding per level of its tree (at most P - 1 levels), each within 2^-24 of the running sum
                    assert base_of(kind) in ("specials", "specials_neg"), (P, kind)
                    assert abs(vol - C.volume_cm3(r["vol32"], r["area_px"])) <= P * 2.0 ** -24 * vol, (P, kind, mode)
                assert (r["count"] == 0) == ((vol, area, maxd) == (0.0, 0.0, 0.0)), (P, kind, mode)


def test_tail_frames_reach_their_branches():
    for P in C.TAIL_P:
        rs, cat = tail_catalogue(P)
        pairs = C.tie_pairs(P)
        seen_neg = set()
        for kind, (h, rf, u, refs) in cat.items():
            r, base = refs["full"], kind.rstrip("0123456789")
            seen_neg.add(r["use_neg"])
            if base == "tie":
                assert r["sums"][0] == r["sums"][1] and not r["use_neg"] and (P < 2 or r["sums"][0] > 0), (P, kind)
            if base == "below_eps":
                assert r["count"] == 0 and refs["roi"]["count"] == 0 and (P < 16 or (np.abs(h) == np.float32(C.TAIL_EPS)).any()), (P, kind)
            if base == "no_finite_roi":
                assert r["arg"] == -1 and r["minidx"] == -1 and np.isnan(r["minval"]), (P, kind)
            if base in ("specials", "specials_neg") and P >= 1023:
                eps = np.float32(C.TAIL_EPS)
                assert np.isnan(h).any() and (np.isneginf(h) if r["use_neg"] else np.isposinf(h)).any() and (np.abs(h) == eps).any(), (P, kind)
                assert (np.abs(h) == np.nextafter(eps, np.float32(1))).any() and r["use_neg"] == (base == "specials_neg"), (P, kind)
                assert (~np.isfinite(h) & (rf != 0)).any() and (~np.isfinite(h) & (rf == 0)).any(), (P, kind)        # inside and outside the frame's ROI
                assert (~np.isfinite(u) & (rs != 0)).any(), (P, kind)
            if base in ("zeromax", "zerorev", "valtie") and pairs:
                i, j = pairs[int(kind[len(base):])]
                assert r["arg"] == i and r["minidx"] == i and h[i] == h[j] and u[i] == u[j], (P, kind, r["arg"], r["minidx"])
                if base != "valtie":
                    assert r["minval"] == 0.0 and h[i] == 0.0 and C.bits32(h)[i] != C.bits32(h)[j] and C.bits32(u)[i] != C.bits32(u)[j], (P, kind)
                if base == "zeromax":                       # the later zero is the one an order by float bits prefers
                    assert C.bits32(h)[i] == 0x80000000 and C.bits32(h)[j] == 0 and C.bits32(u)[i] == 0 and C.bits32(u)[j] == 0x80000000, (P, kind)
        assert seen_neg == {False, True} or P == 1, P
    # NumPy's own answer on the two smallest signed-zero ties
    assert np.nanargmax(np.array([-0.0, 0.0], np.float32)) == 0 and np.argmin(np.array([0.0, -0.0, 0.0], np.float32)) == 0


# =======================================================================================================================================
# CPU: smoothing, composition, holes, sign flip, back end

def finish_cases(h, w):
    return cached(("finish", h, w), lambda: [C.finish_case(h, w, ci, g) for ci in range(len(C.FINISH_CONFIGS)) for g in (0, 1)
                                             if (h * w <= 64 * 64 or ci < 6)])


def test_composition_restatement_equals_the_oracle_and_reaches_its_branches():
    for sigma, taps in C.SIGMAS.items():
        assert (cvlite.gaussian_ksize(sigma) if sigma > 0 else 0) == taps
    seen = set()
    for h, w in C.FINISH_SHAPES[:4]:
        roi = C.frame_roi(h, w)
        for case in finish_cases(h, w):
            sigma = case["sigma"]
            if sigma > 0 and case["extra"] != "den_min":      # the denominator handed in is masked_gaussian_smooth's own
                z = np.where(roi, case["unitless"][0], np.float32(np.nan)).astype(np.float32)
                assert_bits32(C.ref_masked_smooth(z, roi, sigma, case["roi_den"]), O.masked_gaussian_smooth(z, roi, sigma), (h, w, sigma))
            if case["extra"] == "den_min":
                assert (case["roi_den"][roi] == np.float32(1e-6)).any()
            for n, kind in enumerate(case["kinds"]):
                rel = (case["reliable"][n] != 0) & roi
                ul = case["unitless"][n]
                assert np.isnan(ul[~roi]).all() and not np.isnan(ul[roi & ~rel]).any(), (h, w, kind)
                with np.errstate(invalid="ignore"):
                    assert not (ul[roi & np.isfinite(ul)] > 0).any()
                # np.minimum(x, 0.0) hands back its second operand for a zero of either sign: the clamp leaves no negative zero
                assert not (C.bits32(ul) == 0x80000000).any(), (h, w, kind)
                if kind == "border":
                    assert (case["reliable"][n] != 0)[~roi].any() and rel.any()
                if kind == "ring" and min(h, w) >= 17:
                    assert rel.any() and (cvlite.dist_l2_3x3(rel.astype(np.uint8) * 255)[rel] < 1.5).all()
                if case["use_band"] and rel.any() and min(h, w) >= 17 and kind in ("blob", "full"):
                    de = np.maximum(case["dist_in"][n] - 1.0, 0.0)
                    assert (rel & (de > 0) & (de < case["band"])).any(), (h, w, kind)          # blend pixels exist
                    seen.add("blend")
                    if (rel & (de == 0) & (case["hmap"][n] < 0)).any():
                        seen.add("edge weight 0 on a negative height")
                if case["extra"] == "specials" and rel.sum() >= 5:
                    assert np.isnan(ul[rel]).any() and np.isinf(ul[rel]).any() and (C.bits32(case["hmap"][n])[rel] == 0x80000000).any(), (h, w, kind)
                    seen.add("specials")
                if case["extra"] == "positive":
                    d = case["depth64"][n]
                    assert not (roi & np.isfinite(d) & (d > 0)).any()
                    seen.add("no candidate")
                if (case["hmap"][n][rel] > 0).any():
                    seen.add("clamp")
    assert seen == {"blend", "edge weight 0 on a negative height", "specials", "no candidate", "clamp"}, seen


def to_mm_cases():
    """(curve, use_neg, unitless, roi, float64 depth) for every curve type and both signs"""
    def make():
        out = []
        for cv in C.CURVES:
            for use_neg in (0, 1):
                u, roi = C.to_mm_case(use_neg)
                out.append((cv, use_neg, u, roi, C.ref_to_mm(u, cv, use_neg)))
        return out
    return cached("to_mm", make)


def test_to_mm_cases_put_the_maximum_off_the_roi():
    for cv, use_neg, u, roi, r in to_mm_cases():
        on = roi != 0
        with np.errstate(invalid="ignore", over="ignore"):
            d = r.astype(np.float32)
            pos = np.isfinite(d) & (d > 0)
        assert (pos[0] & ~on).any() and (pos[0] & on).any() and d[0][pos[0] & ~on].max() > d[0][pos[0] & on].max(), (cv, use_neg)
        assert np.isnan(u[0][~on]).any() and np.isposinf(u[0][~on]).any() and np.isneginf(u[0][~on]).any() and np.isnan(u[0][on]).any() and np.isinf(u[0][on]).any(), (cv, use_neg)
        assert (pos[1] & ~on).any(), (cv, use_neg)
        if cv[0] != 1:                                      # (the line with an offset is positive at argument 0)
            assert not (pos[1] & on).any(), (cv, use_neg)


def hole_cases(h, w, ksize):
    def make():
        out = []
        for kind, thr in (("plain", (0.6, 2.0)), ("plain", None), ("sparse", None), ("all_nan", (0.6, 2.0))):
            hm, rel = C.hole_frame(h, w, kind)
            frac_thr, min_dist = thr if thr else C.hole_thresholds(h, w, ksize, kind)
            frac, dist = C.hole_inputs(hm, rel, ksize)
            cand = O.compute_internal_holes_within_mask(rel, rel & np.isfinite(hm), ksize, frac_thr, min_dist)
            out.append(dict(kind=kind, hmap=hm, reliable=rel, dist=dist, frac=frac, frac_thr=frac_thr, min_dist=min_dist, cand=cand, exact=thr is None))
        return out
    return cached(("holes", h, w, ksize), make)


def test_hole_cases_reach_their_branches():
    for h, w in C.HOLE_SHAPES:
        for ksize in C.HOLE_KSIZES:
            for case in hole_cases(h, w, ksize):
                hm, rel, cand = case["hmap"], case["reliable"], case["cand"]
                holes = rel & ~np.isfinite(hm)
                fr_ok, ds_ok = case["frac"] >= np.float32(case["frac_thr"]), case["dist"] >= np.float32(case["min_dist"])
                assert np.array_equal(cand, holes & fr_ok & ds_ok), (h, w, ksize, case["kind"])
                if case["kind"] == "all_nan":
                    assert not cand.any() and holes.all() == rel.all()
                    continue
                if ksize <= 11:
                    assert cand.any(), (h, w, ksize, case["kind"])
                    assert (holes & ~fr_ok & ds_ok).any() and (holes & fr_ok & ~ds_ok).any(), (h, w, ksize, case["kind"])     # one rejection by each criterion
                if case["exact"] and cand.any():
                    assert (case["frac"][cand] == np.float32(case["frac_thr"])).any() and (case["dist"][cand] == np.float32(case["min_dist"])).any()
                # the glue: medians as process_frame and inpaint_only_mask take them
                tmp, med = C.ref_hole_tmp(hm, rel, cand)
                zin, fill = C.ref_hole_zin(tmp)
                assert np.isfinite(zin).all() and np.array_equal(np.isfinite(tmp), rel & ~cand)
                if cand.any():                              # against inpaint_only_mask itself: what it leaves outside the candidates is zin
                    tmp_o = np.where(rel & np.isfinite(hm), hm, np.float32(med)).astype(np.float32)
                    filled = O.inpaint_only_mask(np.where(rel, tmp_o, np.float32(np.nan)), rel, cand, 3)
                    assert_bits32(filled[rel & ~cand], zin[rel & ~cand], (h, w, ksize))


def test_core_flip_reference_flips_positive_medians_only():
    hm = C.core_flip_planes()
    flips = [C.ref_core_flip(hm[b], m)[1] for b, m in enumerate(C.CORE_MEDIANS)]
    assert flips == [False, False, False, True, False, True, False]


# backend_fused_fits depends on the pixel count alone.  2 x 27259 = 54518 pixels: the largest label forest + mask copy + tail scratch that fits LDS;
# 3 x 18173 = 54519: the first that does not.  151 x 361 = 54511 (an odd P that fits) and 151 x 362 = 54662 (one column more, which does not): the
# same in a frame's usual proportions
BACKEND_FITS = [(2, 27259), (151, 361)]
BACKEND_BEYOND = [(3, 18173), (151, 362)]
BACKEND_SMALL = [(5, 7), (33, 65)]


def backend_case(h, w, run):
    """B = 3 frames under threshold setting `run`: planes, and the per-frame references"""
    def make():
        min_peak, rel_frac = C.BACKEND_THRESHOLDS[run % 3]
        roi = C.backend_roi(h, w)
        layouts = [C.BACKEND_LAYOUTS[(3 * run + n) % len(C.BACKEND_LAYOUTS)] for n in range(3)]
        status = np.array([[0, 1, 2], [3, 0, 0], [2, 0, 3]][run % 3], np.int32)
        rng = np.random.default_rng([h, w, run])
        reliable = (rng.random((3, h, w)) < 0.7).astype(np.uint8)
        frames = [C.backend_frame(h, w, lay, min_peak, rel_frac, 10 * run + n) for n, lay in enumerate(layouts)]
        refs = [C.ref_backend(f[0], roi, f[3], int(status[n]), reliable[n], min_peak, rel_frac) for n, f in enumerate(frames)]
        return dict(roi=roi, layouts=layouts, status=status, reliable=reliable, depth=np.stack([f[0] for f in frames]), cand=np.stack([f[1] for f in frames]),
                    gmax=np.array([f[2] for f in frames], np.float32), unitless=np.stack([f[3] for f in frames]), pinned=[f[4] for f in frames], refs=refs,
                    min_peak=min_peak, rel_frac=rel_frac)
    return cached(("backend", h, w, run), make)


def test_backend_reference_equals_the_plain_blob_filter_and_reaches_its_branches():
    seen = set()
    for h, w in BACKEND_SMALL:
        for run in range(4):
            case = backend_case(h, w, run)
            for n, ref in enumerate(case["refs"]):
                kept, out = M.ref_blob(case["depth"][n], case["cand"][n], ref["labels"], case["gmax"][n], case["min_peak"], case["rel_frac"])
                assert_equal(kept, ref["kept"], (h, w, run, n))
                assert_bits32(out, ref["depth"], (h, w, run, n))
                lab, pin = ref["labels"], case["pinned"][n]
                if not case["cand"][n].any():
                    assert case["gmax"][n] == 0 and ref["tail"]["count"] == 0
                    seen.add("no candidate")
                if "at_thr" in pin and case["gmax"][n] == C.BACKEND_GMAX:
                    assert ref["kept"][lab == pin["at_thr"]].all()
                    seen.add("peak at the threshold kept, rel_frac %s 0" % ("<" if case["rel_frac"] < 0 else ">="))
                if "below_thr" in pin and case["gmax"][n] == C.BACKEND_GMAX:
                    assert not ref["kept"][lab == pin["below_thr"]].any() and (ref["depth"][lab == pin["below_thr"]] == 0).all()
                    seen.add("peak below the threshold removed")
                if case["layouts"][n] == "border_ring":
                    ys, xs = np.nonzero(lab == lab[0, 0])
                    assert ys.min() == 0 and xs.min() == 0 and ys.max() == h - 1 and xs.max() == w - 1
                    seen.add("four borders")
                if case["status"][n] in (1, 3):
                    assert np.isnan(ref["out_h"]).all() and not ref["out_r"].any()
                    seen.add("status %d" % case["status"][n])
    assert seen == {"no candidate", "peak at the threshold kept, rel_frac < 0", "peak at the threshold kept, rel_frac >= 0", "peak below the threshold removed",
                    "four borders", "status 1", "status 3"}, seen


# =======================================================================================================================================
# CPU: the entry points' signatures and refusals (no HIP call is made by a refused call)

def test_post_hook_prototypes_match_their_signature_table(pkg):
    text = open(os.path.join(os.path.dirname(pkg.__file__), "csrc", "test_hooks_post.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = "\n".join(ln for ln in text.split("\n") if not ln.lstrip().startswith("#"))
    protos = {name: (ret.strip(), [" ".join(q.split()) for q in params.split(",")])
              for ret, name, params in re.findall(r"([A-Za-z_][\w \t\*]*?)\b(vistaf_\w+)\s*\(([^()]*)\)\s*;", text)}
    table = pkg._lib.POST_SIGNATURES
    assert sorted(protos) == sorted(table) and len(table) == 12
    assert not set(table) & {n for grp in pkg._lib.SIGNATURES.values() for n in grp}
    lib = pkg._lib.load()
    scalar = {"int": ctypes.c_int, "double": ctypes.c_double, "float": ctypes.c_float}
    for name, (ret, params) in protos.items():
        restype, argtypes = table[name]
        assert ret == "int" and restype is ctypes.c_int and len(params) == len(argtypes), name
        for q, a in zip(params, argtypes):
            assert a is (ctypes.c_void_p if "*" in q else scalar[q.split()[0]]), (name, q, a)
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    hooks_h = open(os.path.join(os.path.dirname(pkg.__file__), "csrc", "test_hooks.h")).read()
    assert "test_hooks_post.h" in hooks_h


def _call(fn, good, **bad):
    a = dict(good, **bad)
    return fn(*a.values())


def test_post_hooks_refuse_bad_arguments(pkg):
    """every plane is a live host buffer: a refused call touches none of them"""
    lib = pkg._lib.load()
    buf = [np.zeros(256, np.float64) for _ in range(16)]
    p = [ctypes.c_void_p(b.ctypes.data) for b in buf]
    sizes = [dict(B=0), dict(B=-1), dict(B=65536), dict(h=0), dict(w=0), dict(w=-3), dict(h=65536, w=65536)]
    flat = [dict(B=0), dict(B=65536), dict(P=0), dict(P=-1)]

    def check(fn, good, bads, planes):
        assert all(_call(fn, good, **bad) == E_INVALID for bad in bads), fn.__name__
        for k in planes:
            assert _call(fn, good, **{k: None}) == E_INVALID, (fn.__name__, k)

    good = dict(detr=p[0], bg=p[1], rel=p[2], sigma=0.75, hmap=p[3], B=1, h=4, w=5, variant=0, st=None)
    check(lib.vistaf_ftp_test_smooth_reliable, good, sizes + [dict(variant=3), dict(variant=-1), dict(sigma=-1.0), dict(sigma=float("nan")), dict(sigma=100.0),
                                                             dict(sigma=2.0, variant=2), dict(sigma=0.0, variant=2)], ("detr", "bg", "rel", "hmap"))
    good = dict(hmap=p[0], med=p[1], flipped=p[2], B=1, P=6, st=None)
    check(lib.vistaf_ftp_test_core_flip, good, flat, ("hmap", "med", "flipped"))
    good = dict(hmap=p[0], rel=p[1], dist=p[2], ksize=3, frac=0.6, mind=2.0, cand=p[3], B=1, h=4, w=5, st=None)
    check(lib.vistaf_ftp_test_hole_candidates, good, sizes + [dict(ksize=1), dict(ksize=4), dict(ksize=513), dict(ksize=-3)], ("hmap", "rel", "dist", "cand"))
    good = dict(hmap=p[0], rel=p[1], cand=p[2], med=p[3], tmp=p[4], B=1, P=6, st=None)
    check(lib.vistaf_ftp_test_hole_tmp, good, flat, ("hmap", "rel", "cand", "med", "tmp"))
    good = dict(tmp=p[0], fill=p[1], B=1, P=6, st=None)
    check(lib.vistaf_ftp_test_hole_zin, good, flat, ("tmp", "fill"))
    good = dict(hmap=p[0], rel=p[1], cand=p[2], zin=p[3], orel=p[4], B=1, P=6, st=None)
    check(lib.vistaf_ftp_test_hole_merge, good, flat, ("hmap", "rel", "cand", "zin", "orel"))
    good = dict(hmap=p[0], rel=p[1], roi=p[2], din=p[3], dout=p[4], den=p[5], band=3.0, use_band=1, sigma=0.75, ct=4, ca=1.0, cb=1.0, cc=0.0, use_neg=1,
                ul=p[6], depth=p[7], cand=p[8], gmax=p[9], B=1, h=4, w=5, variant=0, st=None)
    check(lib.vistaf_ftp_test_height_finish, good,
          sizes + [dict(variant=3), dict(variant=-1), dict(use_band=2), dict(use_band=-1), dict(band=0.0), dict(band=-2.0), dict(band=float("nan")), dict(ct=6),
                   dict(ct=-1), dict(ca=float("nan")), dict(sigma=-0.5), dict(sigma=float("inf")), dict(sigma=2.0, variant=2), dict(sigma=0.0, variant=2)],
          ("hmap", "rel", "roi", "din", "dout", "den", "ul", "depth", "cand", "gmax"))
    good = dict(ul=p[0], roi=p[1], ct=4, ca=1.0, cb=1.0, cc=0.0, use_neg=1, depth=p[2], cand=p[3], gmax=p[4], B=1, P=6, st=None)
    check(lib.vistaf_ftp_test_to_mm, good, flat + [dict(ct=6), dict(ct=-1), dict(cb=float("nan"))], ("ul", "roi", "depth", "cand", "gmax"))
    good = dict(height=p[0], rf=p[1], ul=p[2], rs=p[3], mm=0.25, eps=0.01, period=7.0, ft=5, fa=1.0, fb=1.0, fc=0.0, scal=p[4], nscal=16, out3=p[5], B=1, P=6,
                variant=0, st=None)
    check(lib.vistaf_ftp_test_tail, good, flat + [dict(variant=3), dict(variant=-1), dict(ft=6), dict(ft=-1), dict(nscal=8), dict(scal=None, out3=None), dict(rs=None)],
          ("height",))
    good = dict(depth=p[0], cand=p[1], gmax=p[2], ul=p[3], rs=p[4], rel=p[5], status=p[6], mp=0.1, rf=0.3, mm=0.25, eps=0.01, period=7.0, ft=5, fa=1.0, fb=1.0,
                fc=0.0, labels=p[7], peaks=p[8], kept=p[9], scal=p[10], nscal=16, oh=p[11], orr=p[12], B=1, h=4, w=5, variant=0, st=None)
    check(lib.vistaf_ftp_test_backend, good, sizes + [dict(variant=3), dict(variant=-1), dict(ft=7), dict(nscal=8), dict(h=3, w=18173, variant=2),
                                                     dict(h=256, w=256, variant=2)],
          ("depth", "cand", "gmax", "rs", "rel", "status", "labels", "peaks", "scal"))
    good = dict(rc=p[0], fl=p[1], at=p[2], ct=p[3], bm=p[4], bc=p[5], scal=p[6], nscal=16, status=p[7], B=1, st=None)
    check(lib.vistaf_ftp_test_frame_records, good, [dict(B=0), dict(nscal=15), dict(scal=None, status=None)], ("rc",))
    assert b"bad argument" in lib.vistaf_ftp_last_error()
    assert all(not b.any() for b in buf)
    fits = lib.vistaf_ftp_test_backend_fits
    assert all(fits(h, w) == 1 for h, w in BACKEND_FITS + BACKEND_SMALL) and all(fits(h, w) == 0 for h, w in BACKEND_BEYOND + [(256, 256)])
    assert fits(0, 5) == E_INVALID and fits(5, -1) == E_INVALID


# =======================================================================================================================================
# GPU: the force tails

def run_tail(pkg, heights, roi_frames, unitless, roi_static, variant, want_scalars=True, want_out3=True):
    """(tier, scalars [B, NSCAL] or None, out3 [B, 3] or None)"""
    import torch
    B, P = heights.shape
    dh = _dev(heights)
    dr = _dev(roi_frames) if roi_frames is not None else None
    du = _dev(unitless) if unitless is not None else None
    ds = _dev(roi_static) if roi_static is not None else None
    sc = _full((B, NSCAL), SENTINEL, torch.float64) if want_scalars else None
    o3 = _full((B, 3), SENTINEL, torch.float64) if want_out3 else None
    t, a, b, c = C.TAIL_FORCE
    tier = pkg._lib.load().vistaf_ftp_test_tail(_ptr(dh), _ptr(dr), _ptr(du), _ptr(ds), C.TAIL_MM_PER_PX, C.TAIL_EPS, C.TAIL_PERIOD, t, a, b, c, _ptr(sc), NSCAL,
                                               _ptr(o3), B, P, variant, None)
    assert tier >= 0, pkg._lib.load().vistaf_ftp_last_error()
    return tier, (sc.cpu().numpy() if want_scalars else None), (o3.cpu().numpy() if want_out3 else None)


def check_tail_record(S, r, what, has_unitless=True, out3=None):
    """one frame's scalar record (and out3) against ref_tail's dict"""
    area_px = r["area_px"]
    assert C.bits64(S[1]) == C.bits64(r["area"]) and C.bits64(S[2]) == C.bits64(r["maxd"]), (what, "area / max depth", S[1], r["area"], S[2], r["maxd"])
    # the float32 behind the volume: float64 products and quotients move a float32 by far less than its spacing, so the cast recovers it
    got32 = np.float32(S[0] * 1000.0 / area_px)
    assert C.bits64(S[0]) == C.bits64(C.volume_cm3(got32, area_px) if r["count"] else 0.0), (what, "volume is not a float32 sum through the tail's expression", S[0])
    want32 = r["vol32"]
    assert got32 in (want32, np.nextafter(want32, np.float32(np.inf)), np.nextafter(want32, np.float32(-np.inf))), (what, "volume", got32, want32)
    force = O.predict_force_from_volume(C.curve_model(*C.TAIL_FORCE), float(S[0]))
    assert C.within_depth_rule(S[3], force), (what, "force", S[3], force)
    assert S[4] == r["arg"], (what, "arg-max of the depth", S[4], r["arg"])
    assert C.bits64(S[5]) == C.bits64(C.TAIL_PERIOD) and C.bits64(S[6]) == C.bits64(C.TAIL_MM_PER_PX), (what, S[5], S[6])
    if has_unitless and r["minidx"] >= 0:
        if r["minval"] == 0.0:
            assert S[7] == 0.0, (what, "minimum", S[7])        # a zero extremum: either sign of zero
        else:
            assert C.bits64(S[7]) == C.bits64(r["minval"]), (what, "minimum", S[7], r["minval"])
        assert S[8] == r["minidx"], (what, "arg-min of the unitless height", S[8], r["minidx"])
    else:
        assert C.bits64(S[7]) == C.QNAN64 and S[8] == -1.0, (what, S[7], S[8])
    assert (S[9:] == SENTINEL).all(), (what, "the rest of the record was written")
    if out3 is not None:
        assert np.array_equal(C.bits64(out3), C.bits64(S[:3])), (what, "out3", out3, S[:3])


def expected_tail_tier(B, P):
    return 2 if (P >= 262144 and B <= 192) else 1       # big_frames of k_big.hip: the pure function launch_tail dispatches on


@pytest.mark.gpu
@pytest.mark.parametrize("P", C.TAIL_P, ids=["P%d" % p for p in C.TAIL_P])
def test_tails_equal_reference_and_each_other(pkg, P):
    rs, cat = tail_catalogue(P)
    names = list(cat)
    groups = [names[i:i + 3] for i in range(0, len(names), 3)] + [names[:1], names[-1:]]          # B = 3, a short last group, and B = 1 twice
    for g, grp in enumerate(groups):
        H, RF, U = (np.stack([cat[k][c] for k in grp]) for c in range(3))
        got = {}
        for variant in (1, 2, 0):
            tier, S, o3 = run_tail(pkg, H, None, U, rs, variant)
            assert tier == (variant or expected_tail_tier(len(grp), P)), (variant, tier)
            for b, k in enumerate(grp):
                check_tail_record(S[b], cat[k][3]["full"], (P, k, "variant %d" % variant), out3=o3[b])
            got[variant] = (S, o3)
        assert np.array_equal(C.bits64(got[1][0]), C.bits64(got[2][0])) and np.array_equal(C.bits64(got[1][1]), C.bits64(got[2][1])), (P, grp, "variants 1 and 2 differ")
        if g < 2:                   # the frame's own ROI, no unitless plane; then out3 alone, without the static ROI
            for variant in (1, 2):
                _, S, _ = run_tail(pkg, H, RF, None, rs, variant, want_out3=False)
                _, _, o3 = run_tail(pkg, H, RF, None, None, variant, want_scalars=False)
                for b, k in enumerate(grp):
                    check_tail_record(S[b], cat[k][3]["roi"], (P, k, "own ROI, variant %d" % variant), has_unitless=False, out3=o3[b])


# =======================================================================================================================================
# GPU: the back end from the candidates on

def run_backend(pkg, case, variant):
    import torch
    B, h, w = case["depth"].shape
    dd, dc, dg, du = _dev(case["depth"]), _dev(case["cand"]), _dev(case["gmax"]), _dev(case["unitless"])
    dr, drel, dst = _dev(case["roi"]), _dev(case["reliable"]), _dev(case["status"])
    lab = _full((B, h, w), -7, torch.int32)
    pk = _full((B, h, w), 0x5a5a5a5a, torch.int32)
    kept = _full((B, h, w), 77, torch.uint8)
    sc = _full((B, NSCAL), SENTINEL, torch.float64)
    oh = _full((B, h, w), -3.0, torch.float32)
    orr = _full((B, h, w), 77, torch.uint8)
    t, a, b, c = C.TAIL_FORCE
    tier = pkg._lib.load().vistaf_ftp_test_backend(_ptr(dd), _ptr(dc), _ptr(dg), _ptr(du), _ptr(dr), _ptr(drel), _ptr(dst), case["min_peak"], case["rel_frac"],
                                                  C.TAIL_MM_PER_PX, C.TAIL_EPS, C.TAIL_PERIOD, t, a, b, c, _ptr(lab), _ptr(pk), _ptr(kept), _ptr(sc), NSCAL, _ptr(oh),
                                                  _ptr(orr), B, h, w, variant, None)
    assert tier >= 0, pkg._lib.load().vistaf_ftp_last_error()
    return tier, dict(depth=dd.cpu().numpy(), labels=lab.cpu().numpy(), peaks=pk.cpu().numpy().view(np.uint32), kept=kept.cpu().numpy(), scalars=sc.cpu().numpy(),
                      out_h=oh.cpu().numpy(), out_r=orr.cpu().numpy())


def check_backend(got, case, what):
    for n, ref in enumerate(case["refs"]):
        w_ = (what, case["layouts"][n])
        assert_equal(got["labels"][n], ref["labels"], w_ + ("labels",))
        assert_equal(got["kept"][n], ref["kept"], w_ + ("kept",))
        assert_bits32(got["depth"][n], ref["depth"], w_ + ("depth",))
        assert_bits32(got["out_h"][n], ref["out_h"], w_ + ("out_h",))
        assert_equal(got["out_r"][n], ref["out_r"], w_ + ("out_r",))
        lab = ref["labels"]
        roots = np.flatnonzero(lab.ravel() == np.arange(lab.size))
        peak = np.zeros(lab.size, np.float32)
        np.maximum.at(peak, lab.ravel()[lab.ravel() >= 0], case["depth"][n].ravel()[lab.ravel() >= 0])
        assert_equal(got["peaks"][n].ravel()[roots], C.bits32(peak)[roots], w_ + ("peak bits at the roots",))
        check_tail_record(got["scalars"][n], ref["tail"], w_)


BACKEND_RUNS = [(h, w, run) for h, w in BACKEND_SMALL for run in range(4)] + [(h, w, 1) for h, w in BACKEND_FITS + BACKEND_BEYOND]


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,run", BACKEND_RUNS, ids=["%dx%d_run%d" % r for r in BACKEND_RUNS])
def test_backend_tiers_equal_reference_and_each_other(pkg, h, w, run):
    case = backend_case(h, w, run)
    fits = (h, w) not in BACKEND_BEYOND
    assert pkg._lib.load().vistaf_ftp_test_backend_fits(h, w) == int(fits)
    outs = {}
    for variant in (1, 2, 0) if fits else (1, 0):
        tier, got = run_backend(pkg, case, variant)
        assert tier == (variant or (2 if fits else 1)), (variant, tier)
        check_backend(got, case, (h, w, run, "variant %d" % variant))
        outs[variant] = got
    if fits:
        roots = np.stack([r["labels"].ravel() == np.arange(h * w) for r in case["refs"]]).reshape(-1, h, w)
        for k in ("depth", "labels", "kept", "out_h", "out_r"):
            assert np.array_equal(outs[1][k].view(np.uint8), outs[2][k].view(np.uint8)), (h, w, run, k, "variants 1 and 2 differ")
        assert np.array_equal(C.bits64(outs[1]["scalars"]), C.bits64(outs[2]["scalars"])) and np.array_equal(outs[1]["peaks"][roots], outs[2]["peaks"][roots])
    else:
        assert pkg._lib.load().vistaf_ftp_test_backend(*([None] * 7), 0.1, 0.3, 0.25, 0.01, 7.0, 5, 1.0, 1.0, 0.0, *([None] * 4), NSCAL, None, None, 1, h, w, 2,
                                                      None) == E_INVALID


@pytest.mark.gpu
def test_frame_records_and_empty_marks(pkg):
    import torch
    B = 5
    rel = np.array([0, 7, 0, 0, 12345], np.int32)
    fl, bad = np.array([1, 0, 1, 0, 0], np.int32), np.array([3, 0, 99, 5, 1], np.int32)
    at, ct, bm = (np.array(v, np.float32) for v in ([0.5, np.nan, 1e-3, 2.0, 0.1], [1.5, 2.5, np.inf, 0.0, -0.0], [-0.25, 0.0, np.nan, 3.0, 1e-40]))
    status = np.array([0, 0, 2, 3, 0], np.int32)
    sc = _full((B, NSCAL + 2), SENTINEL, torch.float64)
    ds = _dev(status)
    planes = [_dev(a) for a in (rel, fl, at, ct, bm, bad)]
    lib = pkg._lib.load()
    pkg._lib.check(lib.vistaf_ftp_test_frame_records(*[_ptr(t) for t in planes], _ptr(sc), NSCAL + 2, _ptr(ds), B, None))
    S = sc.cpu().numpy()
    want = np.stack([rel, fl, at, ct, bm, bad, np.zeros(B)], 1).astype(np.float64)
    assert np.array_equal(C.bits64(S[:, 9:16]), C.bits64(want)) and (S[:, :9] == SENTINEL).all() and (S[:, 16:] == SENTINEL).all()
    assert ds.cpu().numpy().tolist() == [1, 0, 2, 3, 0]            # empty and without a status yet: 1; a status already there stays
    sc2 = _full((B, NSCAL), SENTINEL, torch.float64)
    pkg._lib.check(lib.vistaf_ftp_test_frame_records(_ptr(planes[0]), None, None, None, None, None, _ptr(sc2), NSCAL, None, B, None))
    assert np.array_equal(sc2.cpu().numpy()[:, 10:16], np.zeros((B, 6)))


# =======================================================================================================================================
# GPU: sign flip, smoothing, holes, composition

@pytest.mark.gpu
def test_core_flip_equals_reference(pkg):
    import torch
    hm = C.core_flip_planes()
    B, P = hm.shape
    dh, dm = _dev(hm), _dev(C.CORE_MEDIANS)
    fl = _full((B,), -7, torch.int32)
    pkg._lib.check(pkg._lib.load().vistaf_ftp_test_core_flip(_ptr(dh), _ptr(dm), _ptr(fl), B, P, None))
    got, flags = dh.cpu().numpy(), fl.cpu().numpy()
    for b, med in enumerate(C.CORE_MEDIANS):
        want, flipped = C.ref_core_flip(hm[b], med)
        assert flags[b] == int(flipped), (b, med)
        assert_bits32(got[b], want, ("median", med))


def run_smooth(pkg, case, variant):
    import torch
    B, h, w = case["detr"].shape
    dd, db, dr = _dev(case["detr"]), _dev(case["bg_med"]), _dev(case["reliable"])
    out = _full((B, h, w), -3.0, torch.float32)
    tier = pkg._lib.load().vistaf_ftp_test_smooth_reliable(_ptr(dd), _ptr(db), _ptr(dr), case["sigma"], _ptr(out), B, h, w, variant, None)
    assert tier >= 0, pkg._lib.load().vistaf_ftp_last_error()
    return tier, out.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", C.FINISH_SHAPES, ids=["%dx%d" % s for s in C.FINISH_SHAPES])
def test_smooth_reliable_equals_reference(pkg, h, w):
    for sigma, taps in C.SIGMAS.items():
        for group in (0, 1):
            case = cached(("smooth", h, w, sigma, group), lambda: C.smooth_case(h, w, sigma, group))
            tile = 0 < taps <= 15
            outs = {}
            for variant in (1, 2, 0) if tile else (1, 0):
                tier, got = run_smooth(pkg, case, variant)
                assert tier == (3 if taps == 0 else variant or (2 if tile else 1)), (sigma, variant, tier)
                assert_bits32(got, case["hmap"], (h, w, sigma, "variant %d" % variant))
                outs[variant] = got
                one = dict(case, **{k: case[k][1:2] for k in ("detr", "bg_med", "reliable", "hmap")})          # B = 1: the middle frame alone
                assert_bits32(run_smooth(pkg, one, variant)[1], one["hmap"], (h, w, sigma, "B = 1, variant %d" % variant))
            if not tile:                # variant 2 does not take this blur: refused, the output plane untouched
                d = _dev(case["detr"])
                assert pkg._lib.load().vistaf_ftp_test_smooth_reliable(_ptr(d), _ptr(_dev(case["bg_med"])), _ptr(_dev(case["reliable"])), sigma, _ptr(d), 3, h, w, 2,
                                                                       None) == E_INVALID


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", C.HOLE_SHAPES, ids=["%dx%d" % s for s in C.HOLE_SHAPES])
def test_hole_kernels_equal_reference(pkg, h, w):
    import torch
    lib = pkg._lib.load()
    for ksize in C.HOLE_KSIZES:
        cases = hole_cases(h, w, ksize)
        for lo in range(0, len(cases), 2):                  # two frames per launch; the thresholds belong to a launch, so one launch per setting
            for case in cases[lo:lo + 2]:
                hm = np.stack([case["hmap"], cases[0]["hmap"]])
                rel = np.stack([case["reliable"], cases[0]["reliable"]]).astype(np.uint8)
                dist = np.stack([case["dist"], cases[0]["dist"]])
                want = [case["cand"], O.compute_internal_holes_within_mask(cases[0]["reliable"], cases[0]["reliable"] & np.isfinite(cases[0]["hmap"]), ksize,
                                                                           case["frac_thr"], case["min_dist"])]
                dh, dr, dd = _dev(hm), _dev(rel), _dev(dist)
                dc = _full((2, h, w), 77, torch.uint8)
                pkg._lib.check(lib.vistaf_ftp_test_hole_candidates(_ptr(dh), _ptr(dr), _ptr(dd), ksize, case["frac_thr"], case["min_dist"], _ptr(dc), 2, h, w, None))
                cand = dc.cpu().numpy()
                for n in range(2):
                    assert_equal(cand[n], want[n].astype(np.uint8), (h, w, ksize, case["kind"], n, "candidates"))
                # the glue on the reference's candidates
                refs = [C.ref_hole_tmp(hm[n], rel[n] != 0, want[n]) for n in range(2)]
                med = np.array([r[1] for r in refs], np.float32)
                dcand, dmed = _dev(np.stack(want).astype(np.uint8)), _dev(med)
                tmp = _full((2, h, w), -3.0, torch.float32)
                pkg._lib.check(lib.vistaf_ftp_test_hole_tmp(_ptr(dh), _ptr(dr), _ptr(dcand), _ptr(dmed), _ptr(tmp), 2, h * w, None))
                got_tmp = tmp.cpu().numpy()
                zins = [C.ref_hole_zin(r[0]) for r in refs]
                for n in range(2):
                    assert_bits32(got_tmp[n], refs[n][0], (h, w, ksize, case["kind"], n, "tmp"))
                dfill = _dev(np.array([z[1] for z in zins], np.float32))
                pkg._lib.check(lib.vistaf_ftp_test_hole_zin(_ptr(tmp), _ptr(dfill), 2, h * w, None))
                got_zin = tmp.cpu().numpy()
                for n in range(2):
                    assert_bits32(got_zin[n], zins[n][0], (h, w, ksize, case["kind"], n, "zin"))
                # after the march: the candidates carry new values, one of them none
                after = np.stack([z[0] for z in zins]) * np.float32(0.5) - np.float32(0.125)
                for n in range(2):
                    idx = np.flatnonzero(want[n].ravel())
                    if len(idx):
                        after[n].ravel()[idx[len(idx) // 2]] = np.nan
                dz = _dev(after)
                orel = _full((2, h, w), 77, torch.uint8)
                dh2 = _dev(hm)
                pkg._lib.check(lib.vistaf_ftp_test_hole_merge(_ptr(dh2), _ptr(dr), _ptr(dcand), _ptr(dz), _ptr(orel), 2, h * w, None))
                got_h, got_r = dh2.cpu().numpy(), orel.cpu().numpy()
                for n in range(2):
                    want_h, want_r = C.ref_hole_merge(hm[n], rel[n] != 0, want[n], after[n])
                    assert_bits32(got_h[n], want_h, (h, w, ksize, case["kind"], n, "merged heights"))
                    assert_equal(got_r[n], want_r, (h, w, ksize, case["kind"], n, "output_reliable"))
                    if len(np.flatnonzero(want[n].ravel())):
                        assert (want[n] & (want_r == 0)).any()              # the candidate whose zin is NaN left the mask


@pytest.mark.gpu
def test_to_mm_alone_ignores_what_lies_off_the_roi(pkg):
    """launch_to_mm on unitless planes whose largest value, NaN and infinities sit off the ROI: the composition writes NaN there in both of its
    variants, so only this entry point reaches the ROI test of to_mm_px and of k_to_mm's maximum (k_compose_finalize_mm cannot be fed such a plane)"""
    import torch
    lib = pkg._lib.load()
    for cv, use_neg, u, roi, r in to_mm_cases():
        B, P = u.shape
        du, dr = _dev(u), _dev(roi)
        dp, cand, gm = _full((B, P), -3.0, torch.float32), _full((B, P), 77, torch.uint8), _full((B,), -3.0, torch.float32)
        pkg._lib.check(lib.vistaf_ftp_test_to_mm(_ptr(du), _ptr(dr), *cv, use_neg, _ptr(dp), _ptr(cand), _ptr(gm), B, P, None))
        d, c, g = dp.cpu().numpy(), cand.cpu().numpy(), gm.cpu().numpy()
        on = roi != 0
        for n in range(B):
            what = (cv, use_neg, n)
            nan = np.isnan(r[n])
            assert np.array_equal(np.isnan(d[n]), nan) and (C.bits32(d[n])[nan] == C.QNAN32).all(), what + ("NaN depths",)
            assert C.within_depth_rule(d[n][~nan], r[n][~nan]).all(), what + ("depth",)
            with np.errstate(invalid="ignore"):
                pos = np.isfinite(d[n]) & (d[n] > 0)
            assert not c[n][~on].any(), what + ("a candidate off the ROI",)
            assert_equal(c[n], (on & pos).astype(np.uint8), what + ("cand",))
            gmax = d[n][on & pos].max() if (on & pos).any() else np.float32(0)
            assert C.bits32(g[n]) == C.bits32(gmax), what + ("gmax", g[n], gmax)
            if n < 2:
                assert d[n][pos & ~on].max() > g[n], what                # the larger depth off the ROI did not reach the maximum


def run_finish(pkg, case, variant):
    import torch
    B, h, w = case["hmap"].shape
    planes = [_dev(case[k]) for k in ("hmap", "reliable", "roi", "dist_in", "dist_out", "roi_den")]
    ul, dp = _full((B, h, w), -3.0, torch.float32), _full((B, h, w), -3.0, torch.float32)
    cand = _full((B, h, w), 77, torch.uint8)
    gm = _full((B,), -3.0, torch.float32)
    t, a, b, c = case["curve"]
    tier = pkg._lib.load().vistaf_ftp_test_height_finish(*[_ptr(p) for p in planes], case["band"] if case["use_band"] else 0.0, case["use_band"], case["sigma"], t, a, b, c,
                                                        case["use_neg"], _ptr(ul), _ptr(dp), _ptr(cand), _ptr(gm), B, h, w, variant, None)
    assert tier >= 0, pkg._lib.load().vistaf_ftp_last_error()
    return tier, dict(unitless=ul.cpu().numpy(), depth=dp.cpu().numpy(), cand=cand.cpu().numpy(), gmax=gm.cpu().numpy())


def check_finish(got, case, what):
    roi = case["roi"] != 0
    assert_bits32(got["unitless"], case["unitless"], what + ("unitless",))
    for n in range(len(case["kinds"])):
        d, r = got["depth"][n], case["depth64"][n]
        nan = np.isnan(r)
        assert np.array_equal(np.isnan(d), nan) and (C.bits32(d)[nan] == C.QNAN32).all(), what + (case["kinds"][n], "NaN depths")
        ok = C.within_depth_rule(d[~nan], r[~nan])
        assert ok.all(), what + (case["kinds"][n], "depth: %d beyond the bound, first got %r for %r" % ((~ok).sum(), d[~nan][~ok][0], r[~nan][~ok][0]))
        with np.errstate(invalid="ignore"):
            cand = roi & np.isfinite(d) & (d > 0)
        assert_equal(got["cand"][n], cand.astype(np.uint8), what + (case["kinds"][n], "cand"))
        gmax = d[cand].max() if cand.any() else np.float32(0)
        assert C.bits32(got["gmax"][n]) == C.bits32(gmax), what + (case["kinds"][n], "gmax", got["gmax"][n], gmax)


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", C.FINISH_SHAPES, ids=["%dx%d" % s for s in C.FINISH_SHAPES])
def test_height_finish_equals_reference(pkg, h, w):
    for case in finish_cases(h, w):
        tile = 0 < case["taps"] <= 15
        outs = {}
        for variant in (1, 2, 0) if tile else (1, 0):
            tier, got = run_finish(pkg, case, variant)
            assert tier == (variant or (2 if tile else 1)), (variant, tier)
            check_finish(got, case, (h, w, case["sigma"], case["use_band"], case["kinds"][0], "variant %d" % variant))
            outs[variant] = got
        if tile:
            for k in ("unitless", "depth", "cand", "gmax"):
                assert np.array_equal(outs[1][k].view(np.uint8), outs[2][k].view(np.uint8)), (h, w, case["sigma"], k, "variants 1 and 2 differ")
        # the last frame alone: B = 1, and a frame's result does not depend on its place in a batch
        one = dict(case, kinds=case["kinds"][2:], **{k: case[k][2:] for k in ("hmap", "reliable", "dist_in", "dist_out", "unitless", "depth64")})
        for variant in (1, 2) if tile else (1,):
            _, got = run_finish(pkg, one, variant)
            check_finish(got, one, (h, w, case["sigma"], case["use_band"], "B = 1", "variant %d" % variant))
            for k in ("unitless", "depth", "cand", "gmax"):
                assert np.array_equal(got[k].view(np.uint8), outs[variant][k][2:].view(np.uint8)), (h, w, case["sigma"], k, "B = 1 differs from its place in B = 3")
