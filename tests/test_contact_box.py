"""The box walk the four per-contact row kernels share (csrc/contact_rows.hpp), on tables written by hand.

The other tests of the shape, thermal, motion and pressure read-outs feed them boxes that a contacts table holds for its own index plane.
Here the boxes are the test's: widths at which the walk's step changes (wider than a workgroup of 256 or 512 threads, exactly as wide, one
pixel), a box on all four borders, and values no table should hold -- NaN, inf, beyond the int range, inverted, reaching out of the frame,
lying outside it.  Every row owns pixels of the index plane, so a box that is read wrongly shows as pixels counted.  The references are the
NumPy restatements of the four read-outs, compared as tests/test_shapes.py, test_thermal.py, test_motion.py and test_pressure.py compare.

The frame is 6 x 520, so the box one pixel wide has 6 pixels: the motion read-out runs with min_pixels = 6 for it to be registered at all.
"""
import numpy as np
import pytest

import motion_helpers as MH
import pressure_helpers as PH
import shapes_helpers as SH
import test_motion as TM
import test_pressure as TP
import test_shapes as TS
import test_thermal as TT
import thermal_helpers as TH

H, W, K, B, PAD, MARGIN, EPS, FRAC, S_MM = 6, 520, 4, 3, 4, 8, 0.01, 0.5, 0.3
MIN_PIXELS = 6
NAN, INF = np.nan, np.inf
# (frame, row): the box as the table holds it, the rectangles of the index plane the row owns (painted in row order, later rows on top)
ROWS = {
    (0, 0): ((0, 0, 519, 2), [(0, 0, 519, 2)]),                              # 520 wide: wider than 256 and 512 threads, step_y = 0
    (0, 1): ((NAN, 3, 60, 5), [(10, 3, 60, 5)]),                             # x0 = NaN
    (0, 2): ((300, 0, 300, 5), [(300, 0, 300, 5)]),                          # 1 wide
    (0, 3): ((100, 3, 160, INF), [(100, 3, 160, 5)]),                        # y1 = +inf
    (1, 0): ((4, 0, 515, 2), [(4, 0, 515, 2)]),                              # exactly 512 wide: step_x = 0 for 256 and 512 threads
    (1, 1): ((2.0e9, 3, 80, 5), [(50, 3, 80, 5)]),                           # x0 = 2e9
    (1, 2): ((100, 3, 355, 5), [(100, 3, 355, 5)]),                          # exactly 256 wide: step_x = 0
    (1, 3): ((420, 3, 400, 5), [(400, 3, 420, 5)]),                          # inverted
    (2, 0): ((0, 0, 519, 5), [(0, 0, 519, 5)]),                              # on all four borders
    (2, 1): ((-5, 2, W + 9, 4), [(0, 2, 40, 4), (480, 2, 519, 4)]),          # reaches out of the frame on both sides
    (2, 2): ((W + 3, 0, W + 20, 5), [(200, 0, 230, 1)]),                     # wholly outside
    (2, 3): ((250, 1, 269, 3), [(250, 1, 269, 3)]),                          # 20 wide: several box rows per stride
}
NO_PIXELS = [(0, 1), (0, 3), (1, 1), (1, 3), (2, 2)]
_SCENE, _REF = {}, {}


def _scene():
    """depth [B,h,w] f32 (a smooth surface above eps everywhere, shifted a little from frame to frame), index, table, count, tracks (row k
    follows row k of the frame before), mm_per_px, the registered temperature planes, forces and status"""
    if not _SCENE:
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
        depth = np.stack([0.5 + 0.25 * np.sin((xx - 0.4 * t) / 23.0) + 0.12 * np.cos((yy - 0.1 * t) * 1.1) + 0.08 * np.sin((xx - 0.4 * t) / 5.3 + yy)
                          for t in range(B)]).astype(np.float32)
        index = np.full((B, H, W), -1, np.int8)
        for (b, k), (_, owned) in sorted(ROWS.items()):
            for x0, y0, x1, y1 in owned:
                index[b, y0:y1 + 1, x0:x1 + 1] = k
        tab, count = SH.table_from_planes(depth, index, K, EPS)
        for (b, k), (box, _) in ROWS.items():
            tab[b, k, [SH.C_X0, SH.C_Y0, SH.C_X1, SH.C_Y1]] = box
        tracks = MH.tracks_rows(B, K)
        for t in range(B):
            for k in range(K):
                MH.link(tracks, t, k, k)
                tracks[t, k, MH.T_DX], tracks[t, k, MH.T_DY] = 0.0, 0.0
        temp = np.stack([TH.temperature_crop(H, W, 20 + b, [(index[b] == k, 3.0 + k) for k in range(K)]) for b in range(B)])
        _SCENE.update(depth=depth, index=index, tab=tab, count=count, tracks=tracks, mpp=np.full(B, S_MM), eps=EPS, frac=FRAC, K=K, temp=temp,
                      margin=MARGIN, status=np.zeros(B, np.int32), params={"min_pixels": MIN_PIXELS}, force=np.array([1.5, 2.1, 2.7]), kinds=("hand",) * B)
    return _SCENE


def _reference():
    """the restatements on the scene and the bars of the four test files, computed once"""
    if not _REF:
        c = _scene()
        assert (c["count"] == K).all()
        want, ne = SH.numpy_shapes(*TS._args(c)), SH.numpy_shapes_ne(*TS._args(c))
        assert SH.exact_equal(want, ne)
        bar = {g: max(4.0 * e, 64.0 * SH.ULP) for g, e in SH.distances(ne, want, c["tab"], c["mpp"]).items()}
        assert all(v < TS.CEILING for v in bar.values()), bar
        _REF["shapes"] = (want, bar)
        want, fs = TH.numpy_thermal(*TH.args(c)), TH.numpy_thermal_fsum(*TH.args(c))
        assert TH.exact_equal(fs, want)
        bar = {g: max(4.0 * v, 64.0 * TH.ULP) for g, v in TH.distances(fs, want, c["temp"]).items()}
        assert all(v < TT.CEILING for v in bar.values()), bar
        _REF["thermal"] = (want, bar)
        first = MH.run(c)
        second = MH.run(c, carry=first[2])                                 # frame 0 follows frame 2: its boxes are walked too
        for order in ("reversed", "fsum"):                                 # no verdict hangs on the order of a sum
            for got, carry in ((first, None), (second, first[2])):
                m2, f2, _ = MH.run(c, order=order, carry=carry)
                assert MH.exact_equal(got[0], m2) and MH.exact_equal(got[1], f2, MH.FRAME_EXACT, MH.MF), order
        _REF["motion"] = (first, second)
    return _REF


def test_the_restatements_accept_every_row_and_see_no_pixel_of_a_hostile_box():
    c, r = _scene(), _reference()
    shapes, (thermal, _) = r["shapes"][0], r["thermal"][0]
    (m1, _, _), (m2, _, _) = r["motion"]
    p32 = (c["depth"] * np.float32(10.0)).astype(np.float32)              # any plane: the tables count pixels of whatever they are given
    rows = PH.tables(p32, c["mpp"], K, 0.5, c["index"], c["tab"], c["count"], c["force"], None)[0]
    for (b, k), (_, owned) in ROWS.items():
        n = sum(int((c["index"][b, y0:y1 + 1, x0:x1 + 1] == k).sum()) for x0, y0, x1, y1 in owned)
        assert n >= 16 or (b, k) == (0, 2), (b, k, n)
        want = 0 if (b, k) in NO_PIXELS else n
        assert shapes[b, k, SH.S["contact_pixels"]] == want and thermal[b, k, TH.T["contact_pixels"]] == want and rows[b, k, PH.R["pixels"]] == want, (b, k)
        # the motion row of (b + 1, k) registers the box of (b, k); frame 0 of the second update follows frame 2
        mrow = m1[b + 1, k] if b + 1 < B else m2[0, k]
        assert mrow[MH.M["template_pixels"]] == want and mrow[MH.M["parent_row"]] == k, (b, k)
        assert (mrow[MH.M["status"]] == MH.TOO_FEW) == (want < MIN_PIXELS), (b, k, mrow[MH.M["status"]])
    assert (m1[0, :, MH.M["status"]] == MH.NO_PARENT).all()
    fits = {(b, k): int(shapes[b, k, SH.S["fit_status"]]) for (b, k) in ROWS}
    assert all(fits[bk] == SH.NONE for bk in NO_PIXELS + [(0, 2)]), fits
    assert all(fits[bk] != SH.NONE for bk in [(0, 0), (1, 0), (1, 2), (2, 0), (2, 1)]), fits                                     # the cap fit runs
    assert (m1[1:, :, MH.M["status"]] == MH.OK).sum() + (m2[0, :, MH.M["status"]] == MH.OK).sum() >= 6                          # and so does motion
    assert all(thermal[b, k, TH.T["surround_pixels"]] == 0 for b, k in NO_PIXELS[:4]) and thermal[0, 0, TH.T["surround_pixels"]] > 0      # no box does not grow


@pytest.mark.gpu
def test_shapes_on_hand_made_boxes(pkg):
    c = _scene()
    want, bar = _reference()["shapes"]
    got = TS._measure(pkg, c)
    TS._check(got, want, bar, c, "hand-made boxes")
    assert np.array_equal(got.view(np.int64), TS._measure(pkg, c).view(np.int64))


@pytest.mark.gpu
def test_thermal_on_hand_made_boxes(pkg):
    c = _scene()
    want, bar = _reference()["thermal"]
    got = TT._measure(pkg, c)
    TT._check(got, want, bar, c, "hand-made boxes")
    again = TT._measure(pkg, c)
    assert np.array_equal(got[0].view(np.int64), again[0].view(np.int64)) and np.array_equal(got[1].view(np.int64), again[1].view(np.int64))


def _check_motion(got, want, what):
    bars = TM._bars()
    assert MH.exact_equal(got[0], want[0]), (what, got[0][..., :4], want[0][..., :4])
    assert MH.exact_equal(got[1], want[1], MH.FRAME_EXACT, MH.MF), (what, got[1], want[1])
    d, df = MH.field_distances(got[0], want[0]), MH.frame_distances(got[1], want[1])
    print(what, "distance to numpy_motion", d, df, "bars", bars["row"], bars["frame"])
    for k in d:
        assert d[k] <= bars["row"][k], (what, k, d[k], bars["row"][k])
    for k in df:
        assert df[k] <= bars["frame"][k], (what, k, df[k], bars["frame"][k])


@pytest.mark.gpu
def test_motion_on_hand_made_boxes(pkg):
    c = _scene()
    first, second = _reference()["motion"]
    mo = pkg.ContactMotion(H, W, B, K, **c["params"])
    got1 = TM._update(pkg, c, reader=mo)
    got2 = TM._update(pkg, c, reader=mo)                                   # frame 0 follows frame 2
    _check_motion(got1, first, "first update")
    _check_motion(got2, second, "second update")
    mo.reset()
    again = TM._update(pkg, c, reader=mo)
    mo.close()
    assert MH.same_bits(again[0], got1[0]) and MH.same_bits(again[1], got1[1])


@pytest.mark.gpu
def test_pressure_on_hand_made_boxes(pkg):
    c = _scene()
    p, rows, frame = TP._measure(pkg, c, PAD, "layer")
    assert p.dtype == np.float32 and np.isfinite(p).all()
    worst = TP._check_tables(c, "layer", p, rows, frame)
    print("hand-made boxes, tables: largest distance in units of the bar", worst)
    for b, k in NO_PIXELS:
        assert rows[b, k, PH.R["pixels"]] == 0, (b, k)
    p2, rows2, frame2 = TP._measure(pkg, c, PAD, "layer")
    assert PH.same_bits(p, p2) and PH.same_bits(rows, rows2) and PH.same_bits(frame, frame2)
