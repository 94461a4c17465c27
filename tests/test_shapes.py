"""Per-contact shape read-out (include/vistaf_shape.h, ContactShapes, FtpSensor.shapes): footprint ellipse, boundary and cap curvature.

The definition is restated in NumPy in tests/shapes_helpers.py: `numpy_shapes` (fit by lstsq) and `numpy_shapes_ne` (normal equations and
Cholesky).  The direct GPU tests hand the read-out hand-made planes and tables (no FTP session), base shape 37 x 53 (P = 1961 is odd, every
frame starts at another misalignment), and ask that the exact fields (pixel counts, fit status, NaN pattern) equal `numpy_shapes` and that
the float fields lie within max(4 e_ne, 64 ulps) of it, every field relative to its own scale, e_ne being the distance between the two
restatements on that case: the device shares the normal-equation form and differs in summation order only, 4 is the project's margin for
"same formulation, other rounding order".  Analytic surfaces pin the numbers independently of the restatement.
"""
import csv
import ctypes
import os
import re

import numpy as np
import pytest

import contacts_helpers as CH
import shapes_helpers as SH
from shapes_helpers import S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
CEILING = 1e-9                  # the bar may never exceed this share of a field's scale
_CASES, _REF = {}, {}


def _case(name):
    if not _CASES:
        _CASES.update(SH.cases())
    return _CASES[name]


def _args(c):
    return c["depth"], c["index"], c["tab"], c["count"], c["mpp"], c["eps"], c["frac"]


def _reference(name):
    """(numpy_shapes, bar per group) of a case, computed once"""
    if name not in _REF:
        c = _case(name)
        want, ne = SH.numpy_shapes(*_args(c)), SH.numpy_shapes_ne(*_args(c))
        assert SH.exact_equal(want, ne), name
        e_ne = SH.distances(ne, want, c["tab"], c["mpp"])
        bar = {g: max(4.0 * e, 64.0 * SH.ULP) for g, e in e_ne.items()}
        assert all(v < CEILING for v in bar.values()), (name, bar)
        _REF[name] = (want, bar, e_ne)
    return _REF[name]


CASE_NAMES = ("single_pixel", "lines", "six_pixels", "whole_frame", "whole_frame_all_pixels", "corners", "ring", "saddle_bowl", "nan_and_eps",
              "stray_rows_and_count_0", "count_above_k", "k64", "mixed_batch", "strip_3x1100", "big_130x130")


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_shape_names_follow_the_header(pkg):
    hdr = open(os.path.join(ROOT, "include", "vistaf_shape.h")).read()
    idx = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define VISTAF_SHAPE_(\w+)\s+(\d+)\b", hdr)}
    assert sorted(idx.values()) == list(range(18))
    for name, i in idx.items():
        assert pkg.SHAPE_NAMES[i] == name
    assert list(pkg.SHAPE_NAMES) == list(pkg._lib.SHAPE_NAMES) == list(pkg.writers.SHAPE_FIELDS) == list(SH.FIELDS)
    assert int(re.search(r"#define VISTAF_NSHAPE\s+(\d+)", hdr).group(1)) == pkg._lib.NSHAPE == SH.NSHAPE == 24
    fit = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define VISTAF_SHAPEFIT_(\w+)\s+(\d+)\b", hdr)}
    assert fit == pkg._lib.SHAPE_FIT == pkg.shapes.SHAPE_FIT == {"ok": SH.OK, "none": SH.NONE, "not_a_cap": SH.NOT_A_CAP}
    assert set(pkg.writers.SHAPE_INT_FIELDS) == set(SH.EXACT)
    for name in ("ContactShapes", "SHAPE_NAMES", "shapes_table", "write_shapes_csv"):
        assert name in pkg.__all__ and hasattr(pkg, name)


def test_library_exports_every_declared_shape_symbol(pkg):
    hdr = open(os.path.join(ROOT, "include", "vistaf_shape.h")).read()
    declared = sorted(set(re.findall(r"\b(vistaf_shape_\w+)\s*\(", hdr)))
    assert declared == sorted(["vistaf_shape_create", "vistaf_shape_measure", "vistaf_shape_destroy"])
    lib = pkg._lib.load()
    for name in declared:
        assert hasattr(lib, name), name
    assert sorted(pkg._lib.SHAPE_EXPORTS) == declared
    for other in ("vistaf_ftp.h", "vistaf_track.h"):
        assert "vistaf_shape" not in open(os.path.join(ROOT, "include", other)).read(), other      # its own header; the others are unchanged


def test_shape_c_abi_refuses_null_and_bad_arguments(pkg):
    lib = pkg._lib.load()
    E_INVALID = -1
    buf = (ctypes.c_double * 32)()
    f32 = (ctypes.c_float * 16)()
    i8 = (ctypes.c_int8 * 16)()
    cnt = (ctypes.c_int32 * 1)()
    assert lib.vistaf_shape_measure(None, f32, i8, buf, cnt, buf, 0.01, 1, buf, None) == E_INVALID
    assert b"null" in lib.vistaf_ftp_last_error()
    lib.vistaf_shape_destroy(None)
    assert lib.vistaf_shape_create(8, 8, 1, 8, 0.5, None) == E_INVALID
    h = ctypes.c_void_p()
    for args in ((0, 8, 1, 8, 0.5), (8, 0, 1, 8, 0.5), (8, 8, 0, 8, 0.5), (8, 8, 1, 0, 0.5), (8, 8, 1, 65, 0.5), (8, 8, 1, 8, -0.1),
                 (8, 8, 1, 8, 1.0), (8, 8, 1, 8, float("nan")), (8, 8, 1, 8, float("inf")), (65536, 65536, 1, 8, 0.5)):
        assert lib.vistaf_shape_create(*args, ctypes.byref(h)) == E_INVALID, args
        assert not h.value and lib.vistaf_ftp_last_error()
    # create touches no device, so the checks of measure run without one; nothing is launched for a refused call
    assert lib.vistaf_shape_create(4, 4, 2, 2, 0.0, ctypes.byref(h)) == 0 and h.value
    for args in ((None, i8, buf, cnt, buf, 0.01, 1, buf), (f32, None, buf, cnt, buf, 0.01, 1, buf), (f32, i8, None, cnt, buf, 0.01, 1, buf),
                 (f32, i8, buf, None, buf, 0.01, 1, buf), (f32, i8, buf, cnt, None, 0.01, 1, buf), (f32, i8, buf, cnt, buf, 0.01, 1, None)):
        assert lib.vistaf_shape_measure(h, *args, None) == E_INVALID, args
        assert b"null" in lib.vistaf_ftp_last_error()
    for batch in (0, 3, -1):
        assert lib.vistaf_shape_measure(h, f32, i8, buf, cnt, buf, 0.01, batch, buf, None) == E_INVALID
        assert b"batch" in lib.vistaf_ftp_last_error()
    for eps in (float("nan"), float("inf"), -float("inf")):
        assert lib.vistaf_shape_measure(h, f32, i8, buf, cnt, buf, eps, 1, buf, None) == E_INVALID
        assert b"depth_eps_mm" in lib.vistaf_ftp_last_error()
    lib.vistaf_shape_destroy(h)


def _hand_made():
    c = np.full((3, 2, 16), np.nan)
    t = np.full((3, 2, 24), np.nan)
    t[0, 0, :18] = [120, 31, 10.5, 7.25, 2.5, 1.25, 0.3, 64, 0, 10.4, 7.3, 0.9, -0.05, -0.02, -1.2, 20.0, 50.0, 1e-8]
    t[0, 1, :9] = [1, 1, 4.0, 5.0, 0.0, 0.0, 0.0, 1, 1]
    t[2, 0, :9] = [40, 22, 3.5, 3.5, 1.0, 1.0, 0.0, 40, 2]
    t[2, 0, 12:15] = [0.04, -0.03, np.pi / 2]
    t[2, 0, 17] = 0.002
    t[2, 1, :2] = [0, 0]
    t[2, 1, 7:9] = [0, 1]
    return t, c, np.array([2, 0, 7], np.int32)


def test_shapes_table_and_csv_round_trip(pkg, tmp_path):
    t, c, n = _hand_made()
    rows = pkg.shapes_table(t, c, n)
    assert [(r["frame"], r["contact"]) for r in rows] == [(0, 0), (0, 1), (2, 0), (2, 1)]
    assert list(rows[0])[2:] == list(pkg.SHAPE_NAMES)
    for r in rows:
        assert all(isinstance(r[k], int) for k in SH.EXACT) and all(isinstance(v, float) for k, v in r.items() if k not in SH.EXACT + ("frame", "contact"))
    assert rows[0]["boundary_pixels"] == 31 and rows[0]["radius_2_mm"] == 50.0 and rows[0]["fit_rms_mm"] == 1e-8
    assert rows[1]["fit_status"] == 1 and np.isnan(rows[1]["apex_x"]) and np.isnan(rows[1]["curvature_1_per_mm"])
    assert rows[2]["fit_status"] == 2 and rows[2]["curvature_axis_rad"] == np.pi / 2 and np.isnan(rows[2]["radius_1_mm"])
    assert rows[3]["contact_pixels"] == 0 and np.isnan(rows[3]["footprint_cx"])
    one = pkg.shapes_table(t[2], c[2], n[2])
    assert len(one) == 2 and one[0]["fit_pixels"] == 40
    with pytest.raises(ValueError):
        pkg.shapes_table(t[:, :, :10], c, n)
    with pytest.raises(ValueError):
        pkg.shapes_table(t, c[:, :1], n)
    path = pkg.write_shapes_csv(str(tmp_path), t, c, n)
    with open(path, newline="") as f:
        back = list(csv.DictReader(f))
    assert len(back) == 4 and list(back[0]) == ["frame", "contact"] + list(pkg.SHAPE_NAMES)
    for r, s in zip(rows, back):
        for k, v in r.items():
            got = float(s[k])
            assert (np.isnan(v) and np.isnan(got)) or got == v, k


def test_contact_shapes_needs_a_device_or_refuses_bad_arguments(pkg):
    import torch
    with pytest.raises(ValueError):
        pkg.ContactShapes(8, 8, 1, 0)
    with pytest.raises(ValueError):
        pkg.ContactShapes(8, 8, 1, 8, fit_min_fraction=1.0)
    with pytest.raises(ValueError):
        pkg.ContactShapes(8, 8, 1, 8, fit_min_fraction=float("nan"))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):
            pkg.ContactShapes(8, 8, 1)


@pytest.mark.parametrize("angle_deg", [0.0, 30.0, -75.0])
def test_numpy_shapes_recovers_an_analytic_paraboloid(angle_deg):
    """the checker checked: both restatements on a float32-sampled cap find its radii, axis, apex and depth to the sampling error (2^-24 of
    the depth per sample), and leave a residual below one float32 step"""
    c, truth, d64 = SH.analytic_case(np.deg2rad(angle_deg))
    for fn in (SH.numpy_shapes, SH.numpy_shapes_ne):
        row = fn(*_args(c))[0, 0]
        assert row[S["fit_status"]] == SH.OK and row[S["fit_pixels"]] >= 30 and SH.analytic_errors(row, truth, c) < 1e-7
        assert abs(row[S["curvature_axis_rad"]] - truth["curvature_axis_rad"]) < 1e-6
        assert 0.0 < row[S["fit_rms_mm"]] < 2.0 ** -24 * truth["apex_depth_mm"]
        n = int(row[S["contact_pixels"]])
        assert n == int((d64 > 0.35).sum()) and 0 < row[S["boundary_pixels"]] < n


def test_both_restatements_agree_and_meet_the_ceiling_on_every_case():
    for name in CASE_NAMES:
        want, bar, e_ne = _reference(name)                             # asserts exact agreement and bar < 1e-9
        assert want.shape[2] == 24 and np.isnan(want[..., 18:]).all()
    st = _reference("lines")[0][0, :3]
    assert (st[:, S["fit_status"]] == SH.NONE).all() and st[0, S["minor_axis_mm"]] == 0.0 and st[1, S["minor_axis_mm"]] == 0.0      # m >= 6, rank-deficient
    assert st[0, S["fit_pixels"]] == 9 and st[1, S["fit_pixels"]] == 9 and st[2, S["fit_pixels"]] >= 6
    assert _reference("six_pixels")[0][0, 0, S["fit_pixels"]] == 6 and _reference("six_pixels")[0][0, 0, S["fit_status"]] == SH.OK
    assert _reference("whole_frame")[0][0, 0, S["boundary_pixels"]] == 2 * (SH.H + SH.W) - 4
    assert list(_reference("saddle_bowl")[0][0, :2, S["fit_status"]]) == [SH.NOT_A_CAP, SH.NOT_A_CAP]
    assert np.isnan(_reference("stray_rows_and_count_0")[0][1]).all() and np.isnan(_reference("stray_rows_and_count_0")[0][0, 2:]).all()


# ---------------------------------------------------------------------------------------------------------------- GPU, direct
def _measure(pkg, c, max_batch=None, reader=None):
    import torch
    B, h, w = c["index"].shape
    sh = reader or pkg.ContactShapes(h, w, max_batch or B, c["K"], c["frac"])
    out = sh.measure(c["depth"], c["index"], c["tab"], c["count"], c["mpp"], c["eps"])
    torch.cuda.synchronize()
    if reader is None:
        sh.close()
    return out.cpu().numpy()


def _check(got, want, bar, c, what):
    assert got.shape == want.shape and got.dtype == np.float64
    assert SH.exact_equal(got, want), (what, got[..., :9], want[..., :9])
    d = SH.distances(got, want, c["tab"], c["mpp"])
    print(what, "distance to numpy_shapes", d, "bar", bar)
    for g in d:
        assert d[g] <= bar[g], (what, g, d[g], bar[g])
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_direct_case_equals_numpy_shapes(pkg, name):
    c = _case(name)
    want, bar, e_ne = _reference(name)
    print(name, "e_ne", e_ne)
    _check(_measure(pkg, c), want, bar, c, name)


@pytest.mark.gpu
def test_batch_equals_frames_one_by_one_and_two_calls_give_the_same_bits(pkg):
    c = _case("mixed_batch")
    whole = _measure(pkg, c)
    again = _measure(pkg, c)
    assert np.array_equal(whole.view(np.int64), again.view(np.int64))                  # every bit, NaNs included
    sh = pkg.ContactShapes(SH.H, SH.W, 5, c["K"], c["frac"])
    for b in range(5):
        one = {k: (v[b:b + 1] if isinstance(v, np.ndarray) else v) for k, v in c.items()}
        got = _measure(pkg, one, reader=sh)
        assert np.array_equal(got.view(np.int64), whole[b:b + 1].view(np.int64)), b
    with pytest.raises(ValueError):
        pkg.ContactShapes(SH.H, SH.W, 2, c["K"]).measure(c["depth"], c["index"], c["tab"], c["count"], c["mpp"], c["eps"])       # batch > max_batch
    with pytest.raises(ValueError):
        sh.measure(c["depth"], c["index"], c["tab"][:, :2], c["count"], c["mpp"], c["eps"])
    with pytest.raises(ValueError):
        sh.measure(c["depth"], c["index"], c["tab"], c["count"], c["mpp"], float("nan"))
    sh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("angle_deg", [0.0, 30.0, -75.0])
def test_analytic_cap_is_recovered_to_the_float32_sampling_error(pkg, angle_deg):
    """d = d0 - (u'^2 / 2 R1 + v'^2 / 2 R2) sampled in float32, R1 = 18 mm, R2 = 41 mm, s = 0.23 mm/px, apex off the pixel grid.  The bar is 4 x
    what numpy_shapes itself gets on the same samples against the true values, the largest error over radii, axis, apex and depth, each
    relative to its scale: the sampling error is one number per surface, and a field numpy_shapes happens to hit exactly would otherwise
    ask the device for more than the samples hold."""
    c, truth, d64 = SH.analytic_case(np.deg2rad(angle_deg))
    ref = SH.numpy_shapes(*_args(c))[0, 0]
    got = _measure(pkg, c)[0, 0]
    e_ref, e_got = SH.analytic_errors(ref, truth, c), SH.analytic_errors(got, truth, c)
    fit = (c["index"][0] == 0) & (c["depth"][0] >= np.float32(c["frac"] * c["tab"][0, 0, SH.C_PEAK]))
    q = d64[fit] - c["depth"][0][fit].astype(np.float64)
    q_rms, peak = np.sqrt((q * q).mean()), truth["apex_depth_mm"]
    r_ref, r_got = abs(ref[S["fit_rms_mm"]] - q_rms) / peak, abs(got[S["fit_rms_mm"]] - q_rms) / peak
    print("angle", angle_deg, "error numpy_shapes", e_ref, "device", e_got, "rms", got[S["fit_rms_mm"]], "quantisation", q_rms, "rms error numpy_shapes",
          r_ref, "device", r_got)
    assert got[S["fit_status"]] == SH.OK and got[S["fit_pixels"]] == ref[S["fit_pixels"]] == fit.sum()
    assert e_got <= 4.0 * e_ref and e_ref < 1e-7
    assert r_got <= 4.0 * r_ref and r_ref < 1e-7


@pytest.mark.gpu
def test_footprint_of_a_filled_ellipse(pkg):
    h, w, s = SH.H, SH.W, 0.23
    yy, xx = np.mgrid[0:h, 0:w]
    m = ((xx - 26) / 20.0) ** 2 + ((yy - 18) / 8.0) ** 2 <= 1.0
    c = SH.pack([SH.Scene(h, w, 0.0).paint(0, m, 0.5)], 4, s, 0.5)
    row = _measure(pkg, c)[0, 0]
    print("ellipse axes", row[S["major_axis_mm"]] / s, row[S["minor_axis_mm"]] / s, "orientation", row[S["orientation_rad"]])
    assert abs(row[S["major_axis_mm"]] - 40 * s) <= s and abs(row[S["minor_axis_mm"]] - 16 * s) <= s
    assert abs(row[S["orientation_rad"]]) <= np.arctan(1.0 / 20.0)
    assert row[S["contact_pixels"]] == m.sum() and (row[S["footprint_cx"]], row[S["footprint_cy"]]) == (26.0, 18.0)


@pytest.mark.gpu
def test_native_size_planes_two_contacts(pkg):
    n, s = 1182, 0.05
    sc = SH.Scene(n, n)
    sc.paint(0, SH.disc(n, n, 640, 500, 180.0), SH.quadric(n, n, 641.3, 498.6, 2.4, 60.0, 45.0, 0.8, s))
    sc.paint(1, SH.rect(n, n, 1150, 1160, 1181, 1181), SH.quadric(n, n, 1170.2, 1172.9, 0.9, 3.0, 5.0, -0.4, s))
    c = SH.pack([sc], 8, s, 0.5)
    want, ne = SH.numpy_shapes(*_args(c)), SH.numpy_shapes_ne(*_args(c))
    bar = {g: max(4.0 * e, 64.0 * SH.ULP) for g, e in SH.distances(ne, want, c["tab"], c["mpp"]).items()}
    assert all(v < CEILING for v in bar.values()) and SH.exact_equal(want, ne)
    got = _measure(pkg, c)
    _check(got, want, bar, c, "native")
    assert got[0, 0, S["contact_pixels"]] > 100000 and list(got[0, :2, S["fit_status"]]) == [SH.OK, SH.OK]


# ---------------------------------------------------------------------------------------------------------------- GPU, through the session
def _session(pkg, n, max_batch):
    model, neg = pkg.load_calibration(os.path.join(G, "calibration_phase_to_height.json"))
    fm = pkg.load_force_calibration(os.path.join(G, "calibration_height_to_force.json"))["best_model"]
    return pkg.FtpSensor(pkg.synth.reference_frame(n), pkg.synth.roi_circle(n), pkg.FtpConfig.scaled(n), model, neg, fm, max_batch=max_batch)


@pytest.mark.gpu
def test_session_shapes_equal_numpy_on_the_gpu_planes(pkg):
    import torch
    n, nb, K = 224, 8, 8
    s = _session(pkg, n, nb)
    o = s.predict_batch(CH.multi_contact_batch(pkg, n, 0, nb))
    r = s.shapes(K)
    torch.cuda.synchronize()
    assert set(r) == {"contacts", "count", "contact_index", "shapes"} and tuple(r["shapes"].shape) == (nb, K, 24)
    depth, mpp = o["height_map_mm"].cpu().numpy(), o["scalars"][:, 6].cpu().numpy()
    got, tab, cnt, idx = (r[k].cpu().numpy() for k in ("shapes", "contacts", "count", "contact_index"))
    eps = s.config.depth_eps_mm
    s.close()
    args = (depth, idx, tab, cnt, mpp, eps, 0.5)
    want, ne = SH.numpy_shapes(*args), SH.numpy_shapes_ne(*args)
    assert SH.exact_equal(want, ne)
    e_ne = SH.distances(ne, want, tab, mpp)
    bar = {g: max(4.0 * e, 64.0 * SH.ULP) for g, e in e_ne.items()}
    print("session e_ne", e_ne, "counts", cnt, "status", got[..., S["fit_status"]][~np.isnan(got[..., 0])])
    assert all(v < CEILING for v in bar.values()), bar
    _check(got, want, bar, {"tab": tab, "mpp": mpp}, "session")
    used = ~np.isnan(got[..., 0])
    assert used.sum() == np.minimum(cnt, K).sum() >= nb
    assert np.array_equal(got[..., S["contact_pixels"]][used], tab[..., SH.C_CONTACT_PIXELS][used])          # the table's column
    assert (got[..., S["fit_status"]][used] == SH.OK).any()                             # the bumps are caps


@pytest.mark.gpu
def test_shapes_leave_the_predict_path_alone(pkg):
    import torch
    n, nb = 224, 4
    a, other = CH.multi_contact_batch(pkg, n, 0, nb), pkg.synth.deformed_batch(n, 0, nb)

    def snap(o):
        return {k: v.clone() for k, v in o.items()}

    def equal(x, y):
        return all(torch.equal(x[k].contiguous().view(torch.uint8), y[k].contiguous().view(torch.uint8)) for k in x)
    s1, s2 = _session(pkg, n, nb), _session(pkg, n, nb)
    with pytest.raises(RuntimeError):
        s1.shapes()                                      # no predict yet
    o = s1.predict_batch(a)
    before = snap(o)
    plain = snap(s1.contacts(8, index_plane=True))
    got = s1.shapes(8)
    first = s1._shapes
    assert s1.shapes(8)["shapes"].shape == got["shapes"].shape and s1._shapes is first          # reused
    assert tuple(s1.shapes(4)["shapes"].shape) == (nb, 4, 24) and s1._shapes is not first      # rebuilt for another K ...
    second = s1._shapes
    s1.shapes(4, fit_min_fraction=0.25)
    assert s1._shapes is not second and s1._shapes.fit_min_fraction == 0.25                    # ... and another fraction
    torch.cuda.synchronize()
    assert equal(o, before) and equal({k: got[k] for k in plain}, plain)
    assert equal(snap(s1.contacts(8, index_plane=True)), plain)                                # a following contacts() is what it was
    after, fresh = snap(s1.predict_batch(other)), s2.predict_batch(other)
    torch.cuda.synchronize()
    assert equal(after, fresh)
    assert equal(s1.contacts(8, index_plane=True), s2.contacts(8, index_plane=True))
    s1.close()
    assert s1._shapes is None
    s2.close()


@pytest.mark.gpu
def test_predict_shapes_flag(pkg):
    n = 224
    s = _session(pkg, n, 1)
    frame = CH.multi_contact_frame(pkg, n, 2)
    plain, with_contacts = s.predict(frame), s.predict(frame, contacts=4)
    res = s.predict(frame, contacts=4, shapes=True)
    assert set(res) == set(with_contacts) | {"shapes"} and set(with_contacts) == set(plain) | {"contacts", "contact_count"}
    assert "shapes" not in with_contacts and "shapes" not in plain
    assert len(res["shapes"]) == len(res["contacts"]) >= 1
    for sh, ct in zip(res["shapes"], res["contacts"]):
        assert list(sh)[0] == "contact" and list(sh)[1:] == list(pkg.SHAPE_NAMES)
        assert sh["contact_pixels"] == ct["contact_pixels"] and isinstance(sh["fit_status"], int)
    with pytest.raises(ValueError):
        s.predict(frame, shapes=True)
    s.close()
