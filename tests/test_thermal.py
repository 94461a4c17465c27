"""Thermal read-out (include/vistaf_thermal.h, ThermalReadout, FtpSensor.thermal): a temperature map registered into the aligned crop and
reduced over the rows of the contacts table.

The definition is restated in NumPy in tests/thermal_helpers.py: `numpy_register` (the registration formula, operation by operation),
`numpy_thermal` (plain float64 sums in row-major order) and `numpy_thermal_fsum` (`math.fsum`).  The direct GPU tests hand the read-out
hand-made planes and tables (no FTP session): crop 37 x 53 of a 61 x 83 photograph at (9, 5), all sizes odd so every frame starts at
another misalignment.  Registration is a fixed sequence of float64 operations stored once as float32, so the device must equal
`numpy_register` bit for bit.  Of the rows, the counts and the NaN pattern must be equal and the selections (min, max, peak) bit-equal; the
summed fields must lie within max(4 e, 64 ulps) of `numpy_thermal`, relative to the field's scale, e being the distance between the two
restatements on that case: the device differs in summation order only, 4 is the project's margin for "same formulation, other rounding
order" (tests/test_shapes.py).
"""
import csv
import ctypes
import os
import re

import numpy as np
import pytest

import contacts_helpers as CH
import thermal_helpers as TH
from thermal_helpers import F, T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
INCLUDE = os.path.join(ROOT, "include")
CEILING = 1e-9                  # the bar may never exceed this share of a field's scale
_CASES, _REF, _REG = {}, {}, {}

CASE_NAMES = ("single_pixel", "corners_margin_clipped", "margin_0", "touching", "no_finite_temperature", "half_covered", "depth_eps_and_nan",
              "count_0", "count_above_k", "stray_index_values", "k64", "status_in_the_middle", "strip_3x1100", "big_130x130")
REGISTER_NAMES = ("identity_null_info", "integer_shift", "fractional_shift", "rotation_0.3", "last_row_and_column", "nan_holes", "non_finite_info",
                  "shift_not_applied", "batch_of_3")


def _case(name):
    if not _CASES:
        _CASES.update(TH.cases())
    return _CASES[name]


def _reference(name):
    """(numpy_thermal, bar per group, e per group) of a case, computed once"""
    if name not in _REF:
        c = _case(name)
        want, fs = TH.numpy_thermal(*TH.args(c)), TH.numpy_thermal_fsum(*TH.args(c))
        assert TH.exact_equal(fs, want), name
        e = TH.distances(fs, want, c["temp"])
        bar = {g: max(4.0 * v, 64.0 * TH.ULP) for g, v in e.items()}
        assert all(v < CEILING for v in bar.values()), (name, bar)
        _REF[name] = (want, bar, e)
    return _REF[name]


def _register_case(name):
    """(map, info, apply_global_shift, numpy_register of them), computed once"""
    if not _REG:
        for k, (m, info, apply) in TH.register_cases().items():
            _REG[k] = (m, info, apply, TH.numpy_register(m, info, TH.H, TH.W, *TH.ORIGIN, apply))
    return _REG[name]


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_thermal_names_follow_the_header(pkg):
    hdr = open(os.path.join(INCLUDE, "vistaf_thermal.h")).read()
    idx = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define VISTAF_THERMAL_(\w+)\s+(\d+)\b", hdr)}
    assert sorted(idx.values()) == list(range(12))
    for name, i in idx.items():
        assert pkg.THERMAL_NAMES[i].lower() == name.lower() and pkg.THERMAL_NAMES[i].endswith("_C") == name.endswith("_C")
    fidx = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define VISTAF_THERMALFRAME_(\w+)\s+(\d+)\b", hdr)}
    assert sorted(fidx.values()) == list(range(7))
    for name, i in fidx.items():
        assert pkg.THERMAL_FRAME_NAMES[i].lower() == name.lower()
    assert list(pkg.THERMAL_NAMES) == list(pkg._lib.THERMAL_NAMES) == list(pkg.writers.THERMAL_FIELDS) == list(TH.FIELDS)
    assert list(pkg.THERMAL_FRAME_NAMES) == list(pkg._lib.THERMAL_FRAME_NAMES) == list(pkg.writers.THERMAL_FRAME_FIELDS) == list(TH.FRAME_FIELDS)
    assert int(re.search(r"#define VISTAF_NTHERMAL\s+(\d+)", hdr).group(1)) == pkg._lib.NTHERMAL == TH.NTHERMAL == 16
    assert int(re.search(r"#define VISTAF_NTHERMALFRAME\s+(\d+)", hdr).group(1)) == pkg._lib.NTHERMALFRAME == TH.NTHERMALFRAME == 8
    ninfo = int(re.search(r"#define VISTAF_ALIGN_NINFO\s+(\d+)", open(os.path.join(INCLUDE, "vistaf_align.h")).read()).group(1))
    assert ninfo == pkg._lib.ALIGN_NINFO == pkg.align.NINFO == TH.NINFO
    assert set(pkg.writers.THERMAL_INT_FIELDS) == set(TH.COUNTS) and set(pkg.writers.THERMAL_FRAME_INT_FIELDS) == set(TH.FRAME_EXACT)
    for name in ("ThermalReadout", "THERMAL_NAMES", "THERMAL_FRAME_NAMES", "thermal", "thermal_table", "write_thermal_csv", "thermal_frame_record"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    for word in ("parity-unpinned", "whatever the batch", "without float atomics"):
        assert word in hdr, word


def test_library_exports_every_declared_thermal_symbol(pkg):
    hdr = open(os.path.join(INCLUDE, "vistaf_thermal.h")).read()
    declared = sorted(set(re.findall(r"\b(vistaf_thermal_\w+)\s*\(", hdr)))
    assert declared == sorted(["vistaf_thermal_create", "vistaf_thermal_register", "vistaf_thermal_measure", "vistaf_thermal_destroy"])
    lib = pkg._lib.load()
    for name in declared:
        assert hasattr(lib, name), name
    assert sorted(pkg._lib.THERMAL_EXPORTS) == declared
    for other in sorted(os.listdir(INCLUDE)):
        if other != "vistaf_thermal.h":
            assert "vistaf_thermal" not in open(os.path.join(INCLUDE, other)).read(), other      # its own header; the others are unchanged


GOOD_CREATE = (8, 8, 16, 16, 2, 3, 1, 2, 8, 4)              # h, w, H, W, crop_x1, crop_y1, apply_global_shift, max_batch, max_contacts, margin


def _with(**kw):
    names = ("h", "w", "H", "W", "crop_x1", "crop_y1", "apply_global_shift", "max_batch", "max_contacts", "margin")
    return tuple(kw.get(n, v) for n, v in zip(names, GOOD_CREATE))


def test_thermal_c_abi_refuses_null_and_bad_arguments(pkg):
    lib = pkg._lib.load()
    E_INVALID = -1
    buf = (ctypes.c_double * 64)()
    f32 = (ctypes.c_float * 256)()
    i8 = (ctypes.c_int8 * 64)()
    cnt = (ctypes.c_int32 * 2)()
    lib.vistaf_thermal_destroy(None)
    assert lib.vistaf_thermal_create(*GOOD_CREATE, None) == E_INVALID and b"out" in lib.vistaf_ftp_last_error()
    h = ctypes.c_void_p()
    bad = [_with(h=0), _with(w=0), _with(h=65537), _with(w=65537), _with(h=65536, w=32768), _with(H=1), _with(W=1), _with(H=65536, W=32768),
           _with(max_batch=0), _with(max_batch=-3), _with(max_batch=65536), _with(max_contacts=0), _with(max_contacts=65), _with(margin=-1), _with(margin=4097),
           _with(crop_x1=2 ** 20 + 1), _with(crop_x1=-2 ** 20 - 1), _with(crop_y1=2 ** 20 + 1), _with(crop_y1=-2 ** 20 - 1)]
    for a in bad:
        assert lib.vistaf_thermal_create(*a, ctypes.byref(h)) == E_INVALID, a
        assert not h.value and lib.vistaf_ftp_last_error()
    for a in (_with(h=65536, w=32767), _with(H=65536, W=32767), _with(margin=0), _with(margin=4096), _with(crop_x1=-2 ** 20, crop_y1=2 ** 20), _with(max_contacts=64),
              _with(max_batch=65535)):              # the frame is grid dimension y of the register launch
        assert lib.vistaf_thermal_create(*a, ctypes.byref(h)) == 0 and h.value, a          # the ends of every range are inside
        lib.vistaf_thermal_destroy(h)
        h = ctypes.c_void_p()
    # create touches no device, so the checks of register and measure run without one; nothing is launched for a refused call
    assert lib.vistaf_thermal_create(*GOOD_CREATE, ctypes.byref(h)) == 0 and h.value
    for a, word in (((None, f32, buf, 1, f32), b"th"), ((h, None, buf, 1, f32), b"d_temp_map"), ((h, f32, buf, 1, None), b"d_temp_crop")):
        assert lib.vistaf_thermal_register(*a, None) == E_INVALID, word
        assert b"null" in lib.vistaf_ftp_last_error() and word in lib.vistaf_ftp_last_error()
    for batch in (0, 3, -1):
        assert lib.vistaf_thermal_register(h, f32, None, batch, f32, None) == E_INVALID
        assert b"batch" in lib.vistaf_ftp_last_error()
    good = [h, f32, f32, i8, buf, cnt, None, 0.01, 1, buf, buf]
    for pos, word in ((0, b"th"), (1, b"d_temp_crop"), (2, b"d_depth_mm"), (3, b"d_contact_index"), (4, b"d_contacts"), (5, b"d_count"), (9, b"d_thermal"),
                      (10, b"d_frame")):
        a = list(good)
        a[pos] = None
        assert lib.vistaf_thermal_measure(*a, None) == E_INVALID, word
        assert b"null" in lib.vistaf_ftp_last_error() and word in lib.vistaf_ftp_last_error()
    for batch in (0, 3, -1):
        a = list(good)
        a[8] = batch
        assert lib.vistaf_thermal_measure(*a, None) == E_INVALID and b"batch" in lib.vistaf_ftp_last_error()
    for eps in (float("nan"), float("inf"), -float("inf")):
        a = list(good)
        a[7] = eps
        assert lib.vistaf_thermal_measure(*a, None) == E_INVALID and b"depth_eps_mm" in lib.vistaf_ftp_last_error()
    lib.vistaf_thermal_destroy(h)


def _hand_made():
    c = np.full((3, 2, 16), np.nan)
    t = np.full((3, 2, 16), np.nan)
    t[0, 0, :12] = [120, 100, 100 / 120, 36.5, 36.75, 33.0, 39.25, 1.5, 38.0, 410, 31.25, 5.25]
    t[0, 1, [0, 1, 9]] = [7, 0, 0]                                                      # no valid pixel, no surround
    t[2, 0, :12] = [1, 1, 1.0, 29.0, 29.0, 29.0, 29.0, 0.0, 29.0, 24, 30.5, -1.5]
    t[2, 1, [0, 1, 9, 10]] = [0, 0, 3, 30.0]
    return t, c, np.array([2, 0, 7], np.int32)


def test_thermal_table_and_csv_round_trip(pkg, tmp_path):
    t, c, n = _hand_made()
    rows = pkg.thermal_table(t, c, n)
    assert [(r["frame"], r["contact"]) for r in rows] == [(0, 0), (0, 1), (2, 0), (2, 1)]
    assert list(rows[0])[2:] == list(pkg.THERMAL_NAMES)
    for r in rows:
        assert all(isinstance(r[k], int) for k in TH.COUNTS) and all(isinstance(v, float) for k, v in r.items() if k not in TH.COUNTS + ("frame", "contact"))
    assert rows[0]["valid_pixels"] == 100 and rows[0]["contrast_C"] == 5.25 and rows[0]["coverage"] == 100 / 120
    assert rows[1]["contact_pixels"] == 7 and np.isnan(rows[1]["mean_C"]) and np.isnan(rows[1]["surround_mean_C"])
    assert rows[2]["std_C"] == 0.0 and rows[2]["contrast_C"] == -1.5 and rows[3]["surround_pixels"] == 3
    failed = t.copy()
    failed[0] = np.nan                                                                   # a frame whose status was not 0
    assert [(r["frame"], r["contact"]) for r in pkg.thermal_table(failed, c, n)] == [(2, 0), (2, 1)]
    one = pkg.thermal_table(t[2], c[2], n[2])
    assert len(one) == 2 and one[0]["surround_pixels"] == 24
    with pytest.raises(ValueError):
        pkg.thermal_table(t[:, :, :10], c, n)
    with pytest.raises(ValueError):
        pkg.thermal_table(t, c[:, :1], n)
    path = pkg.write_thermal_csv(str(tmp_path), t, c, n)
    with open(path, newline="") as f:
        back = list(csv.DictReader(f))
    assert len(back) == 4 and list(back[0]) == ["frame", "contact"] + list(pkg.THERMAL_NAMES)
    for r, s in zip(rows, back):
        for k, v in r.items():
            got = float(s[k])
            assert (np.isnan(v) and np.isnan(got)) or got == v, k
    rec = pkg.thermal_frame_record([1900.0, 30.5, 221.0, 36.0, 5.5, 1.0, 0.0, np.nan])
    assert list(rec) == list(pkg.THERMAL_FRAME_NAMES) and rec["registered_pixels"] == 1900 and rec["hottest_contact"] == 1 and rec["contrast_C"] == 5.5
    rec = pkg.thermal_frame_record(np.array([1900.0, 30.5, 0.0, np.nan, np.nan, np.nan, np.nan, np.nan]))
    assert rec["hottest_contact"] == rec["coldest_contact"] == -1 and np.isnan(rec["contact_mean_C"]) and isinstance(rec["contact_pixels"], int)
    with pytest.raises(ValueError):
        pkg.thermal_frame_record(np.zeros(5))


def test_thermal_readout_needs_a_device_or_refuses_bad_arguments(pkg):
    import torch
    with pytest.raises(ValueError):
        pkg.ThermalReadout(8, 8, 16, 16, (0, 0), max_contacts=0)
    with pytest.raises(ValueError):
        pkg.ThermalReadout(8, 8, 16, 16, (0, 0), surround_margin_px=-1)
    with pytest.raises(ValueError):
        pkg.ThermalReadout(8, 8, 16, 16, (0, 0), surround_margin_px=5000)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):
            pkg.ThermalReadout(8, 8, 16, 16, (0, 0))


def test_predict_with_thermal_needs_contacts(pkg):
    s = object.__new__(pkg.FtpSensor)                       # the check comes before anything of the session is touched
    with pytest.raises(ValueError, match="contacts"):
        s.predict(np.zeros((8, 8), np.uint8), thermal=np.zeros((8, 8), np.float32))


def test_numpy_register_does_what_the_cases_say():
    """the checker checked: slices, the NaN patterns and the independence from the batch, on the restatement itself"""
    x1, y1 = TH.ORIGIN
    m, _, _, ident = _register_case("identity_null_info")
    assert TH.same_bits(ident[0], m[0, y1:y1 + TH.H, x1:x1 + TH.W])
    assert TH.same_bits(_register_case("integer_shift")[3][0], m[0, y1 + 2:y1 + 2 + TH.H, x1 - 3:x1 - 3 + TH.W])      # u = x + 9 - 3, v = y + 5 + 2
    assert TH.same_bits(_register_case("shift_not_applied")[3], ident)
    frac = _register_case("fractional_shift")[3][0]
    assert not np.isnan(frac).any() and not TH.same_bits(frac, ident[0]) and np.abs(frac - ident[0]).max() < 6.0
    rot = _register_case("rotation_0.3")[3][0]
    assert 0 < np.isnan(rot).sum() < 40 and np.isnan(rot[0, 0]) and not np.isnan(rot[TH.H // 2]).any()              # a corner leaves the photograph
    last = _register_case("last_row_and_column")[3][0]
    assert last[TH.H - 1, TH.W - 1] == m[0, TH.PH - 1, TH.PW - 1] and TH.same_bits(last, m[0, TH.PH - TH.H:, TH.PW - TH.W:])
    holes, _, _, got = _register_case("nan_holes")
    want = np.zeros((TH.H, TH.W), bool)
    for y, x in zip(*np.nonzero(~np.isfinite(holes[0]))):
        want[max(y - 1 - y1, 0):y - y1 + 1, max(x - 1 - x1, 0):x - x1 + 1] = True                                   # a hole erases its four dependants
    assert np.array_equal(np.isnan(got[0]), want) and want.sum() == 4 * 5 + 6 - 3                                   # (5, 9): on the crop's first row and column
    assert np.isnan(_register_case("non_finite_info")[3]).all()
    m3, i3, _, b3 = _register_case("batch_of_3")
    for b in range(3):
        assert TH.same_bits(TH.numpy_register(m3[b:b + 1], i3[b:b + 1], TH.H, TH.W, x1, y1), b3[b:b + 1])
    assert not TH.same_bits(b3[0], b3[2])


def _eroded_disc(h, w, circle, px):
    yy, xx = np.mgrid[0:h, 0:w]
    return (xx - circle[0]) ** 2 + (yy - circle[1]) ** 2 <= (circle[2] - px) ** 2


DIRECTION_CIRCLE = (120, 100, 70)


def _direction_scene(name):
    from align_scenes import dark_scene, rolled, smooth_frame
    if name == "smooth":
        return smooth_frame(200, 240), smooth_frame(200, 240, 0.02, 3.3, -2.4), True
    d = dark_scene(200, 240)
    return d, rolled(d, 3, -5), False


def _direction_errors(register, grey, aligned, info_row, crop_box, circle_crop):
    """mean |registered - aligned crop| inside the circle eroded by 8 px, with the record, with its shift negated, and without a record"""
    h, w = aligned.shape
    inside = _eroded_disc(h, w, circle_crop, 8)
    flipped = info_row.copy()
    flipped[:2] = -flipped[:2]
    return [float(np.abs(register(grey, row)[inside].astype(np.float64) - aligned[inside]).mean()) for row in (info_row, flipped, None)]


@pytest.mark.parametrize("scene", ["smooth", "rolled"])
def test_registration_formula_follows_the_alignment_oracle(scene):
    """The grey plane of the deformed photograph, registered by the formula with the record the oracle's aligner wrote, must land on the
    oracle's aligned crop: mean |difference| inside the ROI circle eroded by 8 px at most one fifth of the unregistered crop slice's.
    Measured (grey levels; registered / shift negated / unregistered): smooth 0.284 / 0.284 / 3.86 -- the estimated shift is (0.015, 0.034),
    this scene tests the direction of the warp; rolled 0.052 / 4.19 / 2.26 -- at this size the phase correlation returns (-0.70, 0.26), not the
    roll, and the aligner applies what it returned: the scene tests that the formula undoes that shift with the right sign."""
    from oracle import align_oracle as A
    ref, dfr, ecc = _direction_scene(scene)
    _, aligned, circle_crop, info = A.aligned_crops_arrays(ref, dfr, DIRECTION_CIRCLE, use_ecc=ecc)
    x1, x2, y1, y2 = info["crop"]
    row = TH.info_row(info["shift"], tuple(np.asarray(info["warp"], np.float64).ravel()))
    grey = A.bgr2gray_u8(dfr, 4).astype(np.float32)

    def register(g, r):
        return TH.numpy_register(g[None], None if r is None else r[None], y2 - y1, x2 - x1, x1, y1)[0]
    e_reg, e_flip, e_unreg = _direction_errors(register, grey, aligned.astype(np.float64), row, info["crop"], circle_crop)
    print(scene, "shift", info["shift"], "registered", e_reg, "shift negated", e_flip, "unregistered", e_unreg)
    assert e_reg <= e_unreg / 5.0
    if scene == "rolled":
        assert e_flip > e_unreg > 10.0 * e_reg                          # the wrong sign is worse than no registration at all


def test_both_restatements_agree_and_meet_the_ceiling_on_every_case():
    for name in CASE_NAMES + ("mixed_batch",):
        (want, frame), bar, e = _reference(name)                       # asserts exact agreement and bar < 1e-9
        assert want.shape[2] == 16 and np.isnan(want[..., 12:]).all() and frame.shape[1] == 8 and np.isnan(frame[:, 7]).all()
    row = _reference("single_pixel")[0][0][0, 0]
    assert row[T["contact_pixels"]] == row[T["valid_pixels"]] == 1 and row[T["std_C"]] == 0.0 and row[T["min_C"]] == row[T["max_C"]] == row[T["peak_temp_C"]]
    assert row[T["surround_pixels"]] == 17 * 16 - 1 and row[T["contrast_C"]] > 2.0              # (10, 7) grown by 8: x 2..18, y 0..15
    clipped, zero = _reference("corners_margin_clipped")[0][0][0], _reference("margin_0")[0][0][0]
    assert (clipped[:, T["surround_pixels"]] == 15 * 14 - 42).all() and (zero[:, T["surround_pixels"]] == 0).all() and np.isnan(zero[:, T["contrast_C"]]).all()
    assert np.array_equal(clipped[:, T["mean_C"]], zero[:, T["mean_C"]])
    touch = _reference("touching")[0][0][0]
    assert touch[0, T["surround_pixels"]] == 20 * 23 - 10 * 13 - 5 * 13 and touch[1, T["surround_pixels"]] == 22 * 23 - 12 * 13 - 5 * 13
    none = _reference("no_finite_temperature")[0]
    assert none[0][0, 0, T["contact_pixels"]] > 100 and none[0][0, 0, T["valid_pixels"]] == 0 and none[0][0, 0, T["coverage"]] == 0.0
    assert np.isnan(none[0][0, 0, [T["mean_C"], T["std_C"], T["peak_temp_C"], T["contrast_C"]]]).all() and none[0][0, 0, T["surround_pixels"]] > 0
    assert none[1][0, F["hottest_contact"]] == none[1][0, F["coldest_contact"]] == 1
    half = _reference("half_covered")[0][0][0]
    assert (half[:2, T["coverage"]] > 0.2).all() and (half[:2, T["coverage"]] < 0.8).all() and np.isnan(half[0, T["peak_temp_C"]])
    eps = _reference("depth_eps_and_nan")[0][0][0, 0]
    assert eps[T["contact_pixels"]] == 23 * 20 - 9 - 19 - 1
    assert np.isnan(_reference("count_0")[0][0]).all() and _reference("count_0")[0][1][0, F["contact_pixels"]] == 0
    assert _reference("count_0")[0][1][0, F["registered_pixels"]] == TH.H * TH.W and np.isnan(_reference("count_0")[0][1][0, F["hottest_contact"]])
    above, stray = _reference("count_above_k")[0], _reference("stray_index_values")[0]
    assert above[0].shape[1] == 2 and not np.isnan(above[0][0, :, 0]).any() and np.isnan(stray[0][0, 2:]).all()
    assert np.array_equal(above[0][0, :, :12], stray[0][0, :2, :12])                    # rows 2, 3, 5 of the plane are skin for both
    k64 = _reference("k64")[0]
    assert not np.isnan(k64[0][0, :, T["mean_C"]]).any() and k64[1][0, F["hottest_contact"]] == np.argmax(k64[0][0, :, T["mean_C"]])
    assert k64[1][0, F["coldest_contact"]] == np.argmin(k64[0][0, :, T["mean_C"]])
    mid = _reference("status_in_the_middle")[0]
    assert np.isnan(mid[0][1]).all() and np.isnan(mid[1][1]).all() and not np.isnan(mid[1][[0, 2], :7]).any()
    assert _reference("strip_3x1100")[0][0][0, 0, T["surround_pixels"]] == 0 and _reference("big_130x130")[0][0][0, 0, T["contact_pixels"]] == 130 * 130


# ---------------------------------------------------------------------------------------------------------------- GPU, direct
def _reader(pkg, h, w, max_batch, K, margin, H=TH.PH, W=TH.PW, origin=TH.ORIGIN, apply=True):
    return pkg.ThermalReadout(h, w, H, W, origin, apply, max_batch, K, margin)


@pytest.mark.gpu
@pytest.mark.parametrize("name", REGISTER_NAMES)
def test_registration_equals_numpy_register_bit_for_bit(pkg, name):
    import torch
    m, info, apply, want = _register_case(name)
    th = _reader(pkg, TH.H, TH.W, m.shape[0], 4, 8, apply=apply)
    got = th.register(m, info)
    torch.cuda.synchronize()
    th.close()
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), (name, np.isnan(got).sum(), np.isnan(want).sum())
    assert TH.same_bits(got, want), (name, np.nanmax(np.abs(got - want)))


def _measure(pkg, c, max_batch=None, reader=None):
    import torch
    B, h, w = c["index"].shape
    th = reader or _reader(pkg, h, w, max_batch or B, c["K"], c["margin"], H=max(h, 2), W=max(w, 2), origin=(0, 0))
    out = th.measure(c["temp"], c["depth"], c["index"], c["tab"], c["count"], c["eps"], status=c["status"])
    torch.cuda.synchronize()
    if reader is None:
        th.close()
    return out["thermal"].cpu().numpy(), out["frame"].cpu().numpy()


def _check(got, want, bar, c, what):
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape and got[0].dtype == got[1].dtype == np.float64
    assert TH.exact_equal(got, want), (what, got[0][..., :12], want[0][..., :12], got[1], want[1])
    d = TH.distances(got, want, c["temp"])
    print(what, "distance to numpy_thermal", d, "bar", bar)
    for g in d:
        assert d[g] <= bar[g], (what, g, d[g], bar[g])
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_direct_case_equals_numpy_thermal(pkg, name):
    c = _case(name)
    want, bar, e = _reference(name)
    print(name, "e", e)
    _check(_measure(pkg, c), want, bar, c, name)


@pytest.mark.gpu
def test_batch_equals_frames_one_by_one_and_two_calls_give_the_same_bits(pkg):
    c = _case("mixed_batch")
    want, bar, e = _reference("mixed_batch")
    whole = _measure(pkg, c)
    again = _measure(pkg, c)
    _check(whole, want, bar, c, "mixed_batch")
    assert TH.same_bits(whole[0], again[0]) and TH.same_bits(whole[1], again[1])          # every bit, NaNs included
    th = _reader(pkg, TH.H, TH.W, 5, c["K"], c["margin"])
    for b in range(5):
        one = {k: (v[b:b + 1] if isinstance(v, np.ndarray) else v) for k, v in c.items()}
        got = _measure(pkg, one, reader=th)
        assert TH.same_bits(got[0], whole[0][b:b + 1]) and TH.same_bits(got[1], whole[1][b:b + 1]), b
    with pytest.raises(ValueError):
        _reader(pkg, TH.H, TH.W, 2, c["K"], c["margin"]).measure(*TH.args(c)[:6])                # batch > max_batch
    with pytest.raises(ValueError):
        th.measure(c["temp"], c["depth"], c["index"], c["tab"][:, :2], c["count"], c["eps"])
    with pytest.raises(ValueError):
        th.measure(c["temp"], c["depth"], c["index"], c["tab"], c["count"], float("nan"))
    with pytest.raises(ValueError):
        th.register(np.zeros((1, TH.PH, TH.PW + 1), np.float32))
    with pytest.raises(ValueError):
        th.register(np.zeros((2, TH.PH, TH.PW), np.float32), np.zeros((1, 12)))
    th.close()


# ---------------------------------------------------------------------------------------------------------------- GPU, against the aligner
@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["smooth", "rolled"])
def test_registered_grey_plane_lands_on_the_aligners_crop(pkg, scene):
    """The direction test on the device's own aligner: the grey plane of the deformed photograph, registered with the record `FtpAligner.align`
    returned, against the aligned crop it returned; mean |difference| inside the ROI circle eroded by 8 px at most one fifth of the
    unregistered crop slice's.  A condition that separates a right map from a wrong one, not a precision claim.  Measured on the CPU
    oracle's aligner (grey levels; registered / shift negated / unregistered): smooth 0.284 / 0.284 / 3.86, rolled 0.052 / 4.19 / 2.26; on an
    MI355X with the device's aligner: smooth 0.278 / 0.279 / 3.86 (shift (0.018, 0.029)), rolled 0.055 / 4.20 / 2.26 (shift (-0.70, 0.26))."""
    import torch
    from oracle import align_oracle as A
    ref, dfr, ecc = _direction_scene(scene)
    al = pkg.FtpAligner(ref, circle=DIRECTION_CIRCLE, use_ecc=ecc)
    out = al.align(dfr)
    th = pkg.ThermalReadout.from_aligner(al)
    assert (th.h, th.w) == al.crop_shape and (th.H, th.W) == (200, 240) and th.crop_origin == al.crop_box[:2] and th.apply_global_shift is True
    grey = A.bgr2gray_u8(dfr, 4).astype(np.float32)

    def register(g, r):
        return th.register(g, None if r is None else r[None])[0].cpu().numpy()
    e_reg, e_flip, e_unreg = _direction_errors(register, grey, out["aligned_gray"][0].cpu().numpy().astype(np.float64), out["info"][0], al.crop_box,
                                               al.circle_crop)
    torch.cuda.synchronize()
    print(scene, "shift", out["shift"][0], "registered", e_reg, "shift negated", e_flip, "unregistered", e_unreg)
    assert TH.same_bits(register(grey, out["info"][0]), TH.numpy_register(grey[None], out["info"], *al.crop_shape, *al.crop_box[:2])[0])
    assert e_reg <= e_unreg / 5.0
    th.close()
    al.close()


# ---------------------------------------------------------------------------------------------------------------- GPU, through the session
def _session(pkg, n, max_batch):
    model, neg = pkg.load_calibration(os.path.join(G, "calibration_phase_to_height.json"))
    fm = pkg.load_force_calibration(os.path.join(G, "calibration_height_to_force.json"))["best_model"]
    return pkg.FtpSensor(pkg.synth.reference_frame(n), pkg.synth.roi_circle(n), pkg.FtpConfig.scaled(n), model, neg, fm, max_batch=max_batch)


@pytest.mark.gpu
def test_session_thermal_equals_the_readout_and_predict_equals_the_table_writer(pkg):
    import torch
    n, nb, K = 64, 3, 4
    s = _session(pkg, n, nb)
    crops = np.stack([TH.temperature_crop(n, n, 40 + i) for i in range(nb)])
    crops[:, :, :5] = np.nan                                                              # the photograph ended there
    with pytest.raises(RuntimeError):
        s.thermal(crops)                                                                  # no predict yet
    o = s.predict_batch(CH.multi_contact_batch(pkg, n, 1, nb))
    r = s.thermal(crops, K)
    assert set(r) == {"contacts", "count", "contact_index", "thermal", "thermal_frame"}
    assert tuple(r["thermal"].shape) == (nb, K, 16) and tuple(r["thermal_frame"].shape) == (nb, 8)
    first = s._thermal
    th = pkg.ThermalReadout(n, n, 2 * n, 2 * n, (7, 9), True, nb, K, 8)                   # the photograph's geometry plays no part in measure
    m = th.measure(crops, o["height_map_mm"], r["contact_index"], r["contacts"], r["count"], s.config.depth_eps_mm, status=o["status"])
    torch.cuda.synchronize()
    assert torch.equal(r["thermal"].view(torch.int64), m["thermal"].view(torch.int64))
    assert torch.equal(r["thermal_frame"].view(torch.int64), m["frame"].view(torch.int64))
    got, cnt = r["thermal"].cpu().numpy(), r["count"].cpu().numpy()
    assert cnt.min() >= 1 and (got[:, 0, T["contact_pixels"]] > 0).all() and (got[:, 0, T["valid_pixels"]] > 0).all()
    assert np.array_equal(got[..., T["contact_pixels"]][~np.isnan(got[..., 0])], r["contacts"].cpu().numpy()[..., 1][~np.isnan(got[..., 0])])
    want = TH.numpy_thermal(crops, o["height_map_mm"].cpu().numpy(), r["contact_index"].cpu().numpy(), r["contacts"].cpu().numpy(), cnt,
                            s.config.depth_eps_mm, 8, o["status"].cpu().numpy())
    assert TH.exact_equal((got, r["thermal_frame"].cpu().numpy()), want)
    assert s.thermal(crops, K)["thermal"].shape == r["thermal"].shape and s._thermal is first          # reused
    s.thermal(crops, K, surround_margin_px=3)
    assert s._thermal is not first and s._thermal.surround_margin_px == 3                              # rebuilt for another margin
    th.close()
    s.close()
    assert s._thermal is None
    # one frame through predict: the same numbers as the table writer makes of FtpSensor.thermal
    s = _session(pkg, n, 1)
    frame = CH.multi_contact_frame(pkg, n, 2)
    plain = s.predict(frame, contacts=K)
    res = s.predict(frame, contacts=K, thermal=crops[0])
    assert set(res) == set(plain) | {"thermal", "thermal_frame"} and len(res["thermal"]) == len(res["contacts"]) >= 1
    t = s.thermal(crops[:1], K)
    rows = pkg.thermal_table(t["thermal"].cpu().numpy(), t["contacts"].cpu().numpy(), t["count"].cpu().numpy())
    for a, b, ct in zip(res["thermal"], rows, res["contacts"]):
        assert list(a)[0] == "contact" and list(a)[1:] == list(pkg.THERMAL_NAMES) and a["contact_pixels"] == ct["contact_pixels"]
        for k in a:
            assert a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])), k
    rec = pkg.thermal_frame_record(t["thermal_frame"][0].cpu().numpy())
    assert list(res["thermal_frame"]) == list(rec) == list(pkg.THERMAL_FRAME_NAMES) and res["thermal_frame"]["contact_pixels"] > 0
    for k, v in rec.items():
        assert res["thermal_frame"][k] == v or (np.isnan(v) and np.isnan(res["thermal_frame"][k])), k
    with pytest.raises(ValueError):
        s.predict(frame, thermal=crops[0])
    s.close()
