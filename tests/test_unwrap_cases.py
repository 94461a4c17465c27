"""CPU side of the direct unwrap tests: every case of tests/unwrap_cases.py is what its name says (so that tests/test_unwrap_direct.py reaches the
branch it is about), and the references agree with one another where they must: the C oracle with the literal Python form of the reference on
tie-heavy inputs (which pins its tie order to heapq's before the GPU is held to it), the restated flood with both."""
import numpy as np
import pytest

import unwrap_cases as U
from oracle import cvlite
from oracle import ftp_oracle as O


def _shape(name):
    return U.case(name).frames[0].mask.shape


@pytest.mark.parametrize("name", U.CASE_NAMES)
def test_case_meets_its_stated_conditions(name):
    c, refs = U.case(name), U.references(name)
    assert len(c.frames) == len(c.need) == len(c.reasons) == len(refs)
    h, w = _shape(name)
    assert h >= 8 and w >= 8
    from test_unwrap_direct import SHAPE_TIER           # the tiers the GPU tests pin, against the launcher's arithmetic restated
    assert U.tier_of(h, w) == SHAPE_TIER[(h, w)] and U.tier_of(h, w, 2) == (2 if SHAPE_TIER[(h, w)] == 1 else 0), name
    for f, r, need, why in zip(c.frames, refs, c.need, c.reasons):
        tag = (name, f.name)
        on = f.mask != 0
        # the hook's contract: quality finite and >= +0 on the mask (no -0.0), wrapped finite in [-pi, pi]
        assert f.wrapped.dtype == np.float32 and f.quality.dtype == np.float32 and f.mask.dtype == np.uint8 and f.mask.shape == (h, w), tag
        assert np.isfinite(f.quality).all() and not np.signbit(f.quality).any(), tag
        assert np.isfinite(f.wrapped).all() and np.abs(f.wrapped).max() <= U.PI32, tag
        # the oracle is the yardstick only away from the branch cut
        margin = U.cut_margin(f.wrapped, f.mask)
        assert margin >= U.CUT_MARGIN or name in U.RULE_CASES, (tag, margin)
        got = U.check_reasons(f, r)
        assert (why in got) if isinstance(why, str) else (got == set(why)), (tag, got, why)
        assert bool(got) == bool(need), (tag, got, need)
        # the reference itself: the seed is its own parent, a parent is an 8-neighbour, nothing off the mask is reached
        seed = U.first_argmax(f.quality, f.mask)
        par = r["parent"]
        assert np.array_equal(par >= 0, ~r["nan"]) and not (~r["nan"] & ~on).any(), tag
        if seed >= 0:
            assert par.flat[seed] == seed and int((par == np.arange(h * w).reshape(h, w)).sum()) == 1, tag
            p = np.flatnonzero(par.ravel() >= 0)
            q = par.ravel()[p]
            assert (np.maximum(np.abs(p // w - q // w), np.abs(p % w - q % w)) <= 1).all(), tag
        else:
            assert r["nan"].all(), tag


def test_cases_reach_the_branches_they_are_named_for():
    # the two sides of the uint16 rank range
    assert (921 + 2) * (69 + 2) == 65533 and (215 + 2) * (300 + 2) == 65534
    assert [U.tier_of(*s) for s in ((921, 69), (215, 300), (254, 254), (6000, 24), (800, 64))] == [0, 1, 1, 1, 0]
    assert U.tier_of(254, 254, 2) == 2 and U.tier_of(151, 203, 2) == 0
    # the combs: eight runs per row pass the 6144 runs the propagation holds in LDS and stay within rcap; sixteen do not
    comb8, comb16 = U.case("combs_800x64").frames
    R, E = U.run_edge_counts(comb8.mask)
    assert U.run_cap(800) == 6400 and U.LDS_RUNS < R <= U.run_cap(800) and E <= U.edge_cap(800), (R, E)
    R, E = U.run_edge_counts(comb16.mask)
    assert R > U.run_cap(800), R
    # E > ecap with R <= rcap: two rows of a and b runs touch in at most a + b - 1 pairs, so E <= 2 R - (h - 1) < ecap while ecap = 2 rcap
    # (h <= 4062); the lattice is tall enough for ecap's ceiling
    R, E = U.run_edge_counts(U.case("lattice_6000x24").frames[0].mask)
    assert (R, E) == (36000, 65989) and R <= U.run_cap(6000) == 48000 and E > U.edge_cap(6000) == 65000
    for name in ("random80_224x224", "mixed_151x203", "mixed_254x254"):
        f = U.case(name).frames[-2 if name.startswith("mixed") else 0]
        rows = f.mask[:f.mask.shape[0] // 2] if name == "mixed_254x254" else f.mask          # that one keeps to the upper half of the frame
        assert U.run_edge_counts(f.mask)[0] > U.run_cap(f.mask.shape[0]) == 4096 and 0.78 < rows.mean() < 0.82, name
    # int8: counts beyond 126 in the reference itself
    rows, (aliased, cols), m127 = (U.references(n) for n in ("int8_rows_8x300", "int8_cols_300x64", "int8_m127_8x267"))
    assert np.abs(rows[0]["k"]).max() > 126 and np.abs(cols["k"]).max() > 126
    assert np.abs(aliased["k"]).max() <= 126                   # the (0.5, 2.9) ramp aliases along a diagonal: handed on as inconsistent instead
    assert m127[0]["k"].min() == -127 and m127[0]["k"].max() == 0 and int((m127[0]["k"] == -127).sum()) >= 1
    f = U.case("int8_m127_8x267").frames[0]
    assert U.run_edge_counts(f.mask) == (1, 0)
    # deep trees: the serpentines' depth is at least half their pixels
    for name in ("deep_64x64", "deep_254x254"):
        for f, r in zip(U.case(name).frames, U.references(name)):
            n = int((f.mask != 0).sum())
            depth = U.tree_depth(r["parent"], r["order"])
            assert int((~r["nan"]).sum()) == n and (depth >= n // 2 or not f.name.startswith("serpentine")), (name, f.name, depth, n)
            assert depth >= n // 4, (name, f.name, depth, n)
    # the serpentine's vortex sits in the 2 x 2 block of the first turn, three pixels of which are in the mask
    f = U.case("deep_64x64").frames[2]
    assert f.name == "serpentine_vortex" and f.mask[0:2, 62:64].tolist() == [[1, 1], [0, 1]]
    # components: the seed's blob is the smallest one and the other two stay NaN
    for name in ("components_64x64", "components_215x300"):
        f, r = U.case(name).frames[0], U.references(name)[0]
        num, lab, areas = cvlite.cc8(f.mask)
        seed = U.first_argmax(f.quality, f.mask)
        assert num - 1 == 3 and areas[lab.flat[seed]] == areas[1:].min() == int((~r["nan"]).sum()), name
        last = U.case(name).frames[3]
        assert U.first_argmax(last.quality, last.mask) == last.mask.size - 1
    # the branch cut: the step is exactly float32(pi), inside the tie band, outside it
    for name in U.RULE_CASES:
        exact, near, far = U.case(name).frames
        steps = [float(np.ptp(f.wrapped.astype(np.float64))) for f in (exact, near, far)]
        assert steps[0] == float(U.PI32) and len(np.unique(exact.wrapped)) == 2
        assert U.cut_margin(exact.wrapped, exact.mask) < 1e-7 and 4e-6 < U.cut_margin(near.wrapped, near.mask) < 6e-6 < U.TIE_BAND
        assert 10 * U.TIE_BAND - 1e-5 < U.cut_margin(far.wrapped, far.mask) < U.CUT_MARGIN
        # on the cut the rule wraps a step of +pi_f to -1 and of -pi_f to +1, and 1e-4 beyond the cut likewise
        for f, r in zip((exact, far), (U.references(name)[0], U.references(name)[2])):
            assert sorted(np.unique(r["k"]).tolist()) in ([-1, 0], [0, 1]), (name, f.name)
        assert np.unique(U.references(name)[1]["k"]).tolist() == [0]
    # and the rule along the oracle's tree is the whole flood restated in Python, on the cut too
    for f, r in zip(U.case("cut_64x64").frames, U.references("cut_64x64")):
        k, nan, parent = U.flood_py(f.wrapped, f.quality, f.mask)
        assert np.array_equal(k, r["k"]) and np.array_equal(nan, r["nan"]) and np.array_equal(parent, r["parent"]), f.name
    # dd <= -pi against dd < -pi in the kernels' rule differs only where w[p] - w[par] is exactly -pi in float64, which no two float32 values
    # of [-pi, pi] give: pi's lowest set bit is 2^-48, so one operand is below 2^-24 and the other, in [2, 4), a multiple of 2^-22 within
    # 2^-24 of pi -- but pi lies 0.63 of the way between two such multiples
    assert np.pi * 2.0 ** 48 % 2 == 1 and 0.25 < np.pi * 2.0 ** 22 % 1 < 0.75
    assert U.wrap_count(float(U.PI32)) == -1 and U.wrap_count(-float(U.PI32)) == 1 and U.wrap_count(np.pi) == 0 and U.wrap_count(-np.pi) == 1


def test_run_and_edge_counts_equal_the_run_intervals():
    rng = np.random.default_rng(3)
    masks = [U.m_boundary_runs(8, w) for w in U.CHUNK_WIDTHS] + [U.m_lattice(40, 24), U.m_comb(30, 64, 2, 2), U.m_serpentine(20, 20),
                                                                  U.m_spiral(21, 17), U.m_blobs(40, 40), U.m_empty(8, 8), U.m_full(9, 9)]
    masks += [U.m_random(h, w, rng, d) for h, w in ((8, 70), (33, 65)) for d in (0.2, 0.5, 0.8)]
    for m in masks:
        assert U.run_edge_counts(m) == U.run_edge_counts_plain(m), m.shape
    assert U.run_edge_counts(U.m_lattice(40, 24)) == (240, 11 * 39)            # every contact of the lattice is corner to corner
    on = U.m_lattice(40, 24) != 0
    assert not (on[:-1] & on[1:]).any()


TIE_SHAPES = [(24, 31), (40, 40)]


@pytest.mark.parametrize("h,w", TIE_SHAPES, ids=["%dx%d" % s for s in TIE_SHAPES])
def test_oracle_literal_python_and_restated_flood_agree_on_ties(h, w):
    """The C oracle against the literal Python form: same NaN layout, same counts, and values within the bar the two float32 chains allow.
    Both add one step per tree edge to a float32 running sum: each rounds its sum once per edge (half an ulp of |u| at most, each), and their
    steps differ by atan2f(sinf(d), cosf(d)) against np.angle, at most 4 ulp of pi.  So along a path of `depth` edges they part by at most
    depth * (ulp(max |u|) + 4 ulp(pi)): the oracle's own ulp at the largest |u| of the case, times the depth of its tree -- a few ulp on the
    short paths of full and random masks, more on the one-pixel paths, and always far below the 2 pi of a wrong count.  And the restated
    flood: same layout, counts and parents (the literal form keeps no parents; the flood is the same loop with them)."""
    rng = U.rng_of("agree%dx%d" % (h, w))
    fields = {"ramp": U.ramp(h, w, 0.9, 1.3), "steep": U.ramp(h, w, 2.9, 0.2), "vortex": U.centre_vortex(h, w),
              "two_vortices": U.ramp(h, w, 0.3, 0.2) + U.vortex(h, w, 7.5, 9.5) + U.vortex(h, w, h - 6.5, w - 8.5, -1)}
    qualities = {"constant": U.q_constant(h, w), "two_level": U.q_two_level(h, w, rng), "plateaus": U.q_plateaus(h, w), "random": U.q_random(h, w, rng)}
    masks = {"full": U.m_full(h, w), "random80": U.m_random(h, w, rng), "serpentine": U.m_serpentine(h, w), "blobs": U.m_blobs(h, w)}
    worst = 0.0
    for fn, phi in fields.items():
        wr = U.wrap(phi)
        for qn, q in qualities.items():
            for mn, m in masks.items():
                tag = (fn, qn, mn)
                assert U.cut_margin(wr, m) >= U.CUT_MARGIN, tag
                u, par, order = cvlite.unwrap_quality_guided(wr, m, q, want_tree=True)
                py = O.unwrap_quality_guided_py(wr, m, q)
                assert np.array_equal(np.isnan(u), np.isnan(py)), tag
                ok = ~np.isnan(u)
                k_c, k_py = (np.rint((a[ok].astype(np.float64) - wr[ok]) / U.TWO_PI) for a in (u, py))
                assert np.array_equal(k_c, k_py), tag
                depth = U.tree_depth(par, order)
                bar = depth * (float(np.spacing(np.float32(np.abs(u[ok]).max()))) + 4.0 * float(np.spacing(U.PI32)))
                diff = float(np.abs(u[ok].astype(np.float64) - py[ok]).max())
                worst = max(worst, diff / float(np.spacing(np.float32(np.abs(u[ok]).max()))))
                assert diff <= bar, (tag, diff, bar, depth)
                k, nan, parent = U.flood_py(wr, q, m)
                assert np.array_equal(nan, ~ok) and np.array_equal(parent, par) and np.array_equal(k[ok], k_c.astype(np.int32)), tag
                assert np.array_equal(U.counts_along_tree(wr, par, order), k), tag
    print("largest difference between the C oracle and the literal Python form: %.1f ulp of the case's largest |u|" % worst)
