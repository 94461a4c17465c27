"""Contact motion read-out (include/vistaf_motion.h, ContactMotion, FtpSensor.motion): slide, twist and lift of each tracked touch.

The definition is restated in NumPy in tests/motion_helpers.py (`numpy_motion`): the same float64 operations per pixel, so that what is left
between it and the device is the order of the sums and the device's sin / cos.  The direct GPU tests hand the read-out hand-made planes,
tables and tracker rows (no FTP session), frames of 40 x 52 and 37 x 53, B = 3, K = 4, and ask that the integer fields, the status and the NaN
pattern equal `numpy_motion` and that every float field lies within max(16 e, 1e-12) of it, e being the largest distance over these very
cases between the restatement and itself with its pixel sums reversed and with math.fsum.  Analytic surfaces pin the signs and the
composition independently of the device.
"""
import csv
import ctypes
import os
import re

import numpy as np
import pytest

import motion_helpers as MH
import shapes_helpers as SH
from motion_helpers import M, MF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
FLOOR = 1e-12
_CASES, _REF, _BARS = {}, {}, {}


def _case(name):
    if not _CASES:
        _CASES.update(MH.cases())
    return _CASES[name]


CASE_NAMES = tuple("%s_%dx%d" % (n, h, w) for h, w in MH.SIZES for n in ("main", "empty_frame", "jump")) + ("main_nan_background_37x53",)


def _reference(name):
    """(motion, frame) of numpy_motion on a case and its distances to itself under the two other summation orders, computed once"""
    if name not in _REF:
        c = _case(name)
        m, f, _ = MH.run(c)
        e, ef = {}, {}
        for order in ("reversed", "fsum"):
            m2, f2, _ = MH.run(c, order=order)
            assert MH.exact_equal(m, m2) and MH.exact_equal(f, f2, MH.FRAME_EXACT, MF), (name, order)
            for k, v in MH.field_distances(m, m2).items():
                e[k] = max(e.get(k, 0.0), v)
            for k, v in MH.frame_distances(f, f2).items():
                ef[k] = max(ef.get(k, 0.0), v)
        _REF[name] = (m, f, e, ef)
    return _REF[name]


def _bars():
    """per field: 16 x the largest self-distance over all cases, floor 1e-12"""
    if not _BARS:
        e, ef = {}, {}
        for name in CASE_NAMES:
            for k, v in _reference(name)[2].items():
                e[k] = max(e.get(k, 0.0), v)
            for k, v in _reference(name)[3].items():
                ef[k] = max(ef.get(k, 0.0), v)
        _BARS["row"] = {k: max(16.0 * v, FLOOR) for k, v in e.items()}
        _BARS["frame"] = {k: max(16.0 * v, FLOOR) for k, v in ef.items()}
        _BARS["e"] = (e, ef)
    return _BARS


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_motion_names_follow_the_header(pkg):
    hdr = open(os.path.join(ROOT, "include", "vistaf_motion.h")).read()
    idx = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define VISTAF_MOTION_(\w+)\s+(\d+)\b", hdr)}
    assert sorted(idx.values()) == list(range(20))
    for name, i in idx.items():
        assert pkg.MOTION_NAMES[i] == name
    assert list(pkg.MOTION_NAMES) == list(pkg._lib.MOTION_NAMES) == list(pkg.writers.MOTION_FIELDS) == list(MH.FIELDS)
    fidx = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define VISTAF_MOTIONFRAME_(\w+)\s+(\d+)\b", hdr)}
    assert sorted(fidx.values()) == list(range(8))
    for name, i in fidx.items():
        assert pkg.MOTION_FRAME_NAMES[i] == name
    assert list(pkg.MOTION_FRAME_NAMES) == list(pkg.writers.MOTION_FRAME_FIELDS) == list(MH.FRAME_FIELDS)
    assert int(re.search(r"#define VISTAF_NMOTION\s+(\d+)", hdr).group(1)) == pkg._lib.NMOTION == MH.NMOTION == 24
    assert int(re.search(r"#define VISTAF_NMOTIONFRAME\s+(\d+)", hdr).group(1)) == pkg._lib.NMOTIONFRAME == MH.NFRAME == 8
    st = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define VISTAF_MOTIONST_(\w+)\s+(\d+)\b", hdr)}
    assert st == pkg._lib.MOTION_STATUS == pkg.MOTION_STATUS == {"ok": MH.OK, "not_converged": MH.NOT_CONVERGED, "no_parent": MH.NO_PARENT,
                                                                  "too_few": MH.TOO_FEW, "singular": MH.SINGULAR}
    trk = open(os.path.join(ROOT, "include", "vistaf_track.h")).read()
    for name, i in (("PARENT_ROW", MH.T_PARENT), ("DX", MH.T_DX), ("DY", MH.T_DY)):
        assert int(re.search(r"#define VISTAF_TRACK_%s\s+(\d+)" % name, trk).group(1)) == i
    for name in ("ContactMotion", "MOTION_NAMES", "MOTION_FRAME_NAMES", "motion_table", "write_motion_csv", "motion_frame_record"):
        assert name in pkg.__all__ and hasattr(pkg, name)


def test_library_exports_every_declared_motion_symbol(pkg):
    hdr = open(os.path.join(ROOT, "include", "vistaf_motion.h")).read()
    declared = sorted(set(re.findall(r"\b(vistaf_motion_\w+)\s*\(", hdr)))
    assert declared == sorted(["vistaf_motion_create", "vistaf_motion_update", "vistaf_motion_reset", "vistaf_motion_destroy"])
    lib = pkg._lib.load()
    for name in declared:
        assert hasattr(lib, name), name
    assert sorted(pkg._lib.MOTION_EXPORTS) == declared
    for other in ("vistaf_ftp.h", "vistaf_track.h", "vistaf_shape.h", "vistaf_cloud.h"):
        assert "vistaf_motion" not in open(os.path.join(ROOT, "include", other)).read(), other      # its own header; the others are unchanged


def test_motion_c_abi_refuses_null_and_bad_arguments(pkg):
    lib = pkg._lib.load()
    E_INVALID = -1
    buf = (ctypes.c_double * 64)()
    f32 = (ctypes.c_float * 16)()
    i8 = (ctypes.c_int8 * 16)()
    cnt = (ctypes.c_int32 * 2)()
    good = (f32, i8, buf, cnt, buf, buf, 0.01, 1, buf, buf)
    assert lib.vistaf_motion_update(None, *good, None) == E_INVALID and b"null" in lib.vistaf_ftp_last_error()
    assert lib.vistaf_motion_reset(None) == E_INVALID
    lib.vistaf_motion_destroy(None)
    assert lib.vistaf_motion_create(8, 8, 1, 8, 8, 1e-3, 16, 1, None) == E_INVALID
    h = ctypes.c_void_p()
    for args in ((0, 8, 1, 8, 8, 1e-3, 16, 1), (8, 0, 1, 8, 8, 1e-3, 16, 1), (8, 8, 0, 8, 8, 1e-3, 16, 1), (8, 8, 1, 0, 8, 1e-3, 16, 1),
                 (8, 8, 1, 65, 8, 1e-3, 16, 1), (8, 8, 1, 8, 0, 1e-3, 16, 1), (8, 8, 1, 8, 17, 1e-3, 16, 1), (8, 8, 1, 8, 8, -1e-3, 16, 1),
                 (8, 8, 1, 8, 8, float("nan"), 16, 1), (8, 8, 1, 8, 8, float("inf"), 16, 1), (8, 8, 1, 8, 8, 1e-3, 0, 1), (8, 8, 1, 8, 8, 1e-3, 16, 2),
                 (65536, 65536, 1, 8, 8, 1e-3, 16, 1)):
        assert lib.vistaf_motion_create(*args, ctypes.byref(h)) == E_INVALID, args
        assert not h.value and lib.vistaf_ftp_last_error()
    # create touches no device, so the checks of update run without one; nothing is launched or allocated for a refused call
    assert lib.vistaf_motion_create(4, 4, 2, 2, 8, 1e-3, 16, 1, ctypes.byref(h)) == 0 and h.value
    for i in (0, 1, 2, 3, 4, 5, 8, 9):
        args = list(good)
        args[i] = None
        assert lib.vistaf_motion_update(h, *args, None) == E_INVALID, i
        assert b"null" in lib.vistaf_ftp_last_error()
    for batch in (0, 3, -1):
        assert lib.vistaf_motion_update(h, f32, i8, buf, cnt, buf, buf, 0.01, batch, buf, buf, None) == E_INVALID
        assert b"batch" in lib.vistaf_ftp_last_error()
    for eps in (float("nan"), float("inf"), -float("inf")):
        assert lib.vistaf_motion_update(h, f32, i8, buf, cnt, buf, buf, eps, 1, buf, buf, None) == E_INVALID
        assert b"depth_eps_mm" in lib.vistaf_ftp_last_error()
    odd = ctypes.c_void_p(ctypes.addressof(buf) + 4)
    for i in (2, 4, 5, 8, 9):
        args = list(good)
        args[i] = odd
        assert lib.vistaf_motion_update(h, *args, None) == E_INVALID, i
        assert b"aligned" in lib.vistaf_ftp_last_error()
    assert lib.vistaf_motion_update(h, ctypes.c_void_p(ctypes.addressof(f32) + 2), i8, buf, cnt, buf, buf, 0.01, 1, buf, buf, None) == E_INVALID
    assert lib.vistaf_motion_reset(h) == 0
    lib.vistaf_motion_destroy(h)


def test_motion_table_and_csv_round_trip(pkg, tmp_path):
    c = _case("main_37x53")
    m, f, _, _ = _reference("main_37x53")
    rows = pkg.motion_table(m, c["tab"], c["count"])
    assert [(r["frame"], r["contact"]) for r in rows] == [(b, k) for b in range(3) for k in range(4)]
    assert list(rows[0])[2:] == list(pkg.MOTION_NAMES)
    ints = pkg.writers.MOTION_INT_FIELDS
    for r in rows:
        assert all(isinstance(r[k], int) for k in ints) and all(isinstance(v, float) for k, v in r.items() if k not in ints + ("frame", "contact"))
    assert rows[4]["status"] == MH.OK and rows[4]["tx_px"] == m[1, 0, M["tx_px"]] and rows[7]["status"] == MH.TOO_FEW and np.isnan(rows[7]["tx_px"])
    assert rows[0]["status"] == MH.NO_PARENT and rows[0]["parent_row"] == -1 and rows[10]["parent_row"] == 7 and rows[11]["status"] == MH.SINGULAR
    one = pkg.motion_table(m[1], c["tab"][1], c["count"][1])
    assert len(one) == 4 and one[0]["template_pixels"] == rows[4]["template_pixels"]
    with pytest.raises(ValueError):
        pkg.motion_table(m[:, :, :10], c["tab"], c["count"])
    with pytest.raises(ValueError):
        pkg.motion_table(m, c["tab"][:, :1], c["count"])
    path = pkg.write_motion_csv(str(tmp_path), m, c["tab"], c["count"])
    with open(path, newline="") as fh:
        back = list(csv.DictReader(fh))
    assert len(back) == 12 and list(back[0]) == ["frame", "contact"] + list(pkg.MOTION_NAMES)
    for r, s in zip(rows, back):
        for k, v in r.items():
            got = float(s[k])
            assert (np.isnan(v) and np.isnan(got)) or got == v, k
    rec = pkg.motion_frame_record(f[1])
    assert list(rec) == list(pkg.MOTION_FRAME_NAMES) and rec["registered"] == 2 and isinstance(rec["max_slide_row"], int) and rec["max_slide_mm"] == f[1, 1]
    empty = pkg.motion_frame_record(np.full(8, np.nan))
    assert empty["registered"] == -1 and empty["max_twist_row"] == -1 and np.isnan(empty["mean_tx_mm"])
    with pytest.raises(ValueError):
        pkg.motion_frame_record(f[1, :5])


def test_contact_motion_needs_a_device_or_refuses_bad_arguments(pkg):
    import torch
    for kw in ({"max_contacts": 0}, {"iterations": 0}, {"iterations": 17}, {"tol_px": -1.0}, {"tol_px": float("nan")}, {"min_pixels": 0}):
        with pytest.raises(ValueError):
            pkg.ContactMotion(8, 8, 1, **kw)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):
            pkg.ContactMotion(8, 8, 1)


def _pair(f, origin, s, h, w, move, noise=None):
    """one analytic pair: the surface f placed at `origin`, moved by `move` about its footprint centre; returns (row, tracker-style dxy)"""
    a0 = MH.Contact(f, origin, s)
    sc0, sc1 = SH.Scene(h, w, 0.0), SH.Scene(h, w, 0.0)
    m0 = MH.paint(sc0, 0, a0)
    centre = MH.footprint_centre(m0)
    m1 = MH.paint(sc1, 0, a0.moved(centre, move[:3], move[3]))
    if noise is not None:
        sc1.depth += noise.astype(np.float32)
    c1 = MH.footprint_centre(m1)
    dxy = (c1[0] - centre[0], c1[1] - centre[1])
    ys, xs = np.nonzero(m0)
    return MH.register(sc0.depth, sc1.depth, m0, (xs.max() - xs.min() + 1, ys.max() - ys.min() + 1), s, dxy, dxy), dxy


# what `register` itself shows on the two-bump surface moved by MOVE_A, |estimate - truth| of (tx px, ty px, theta rad, beta mm): the error of
# central differences and bilinear sampling on this surface at 0.3 and at 0.15 mm per pixel (at 0.075 it is 8.6e-4, 9.0e-4, 6.3e-5, 5.6e-4)
RECOVERY_ERROR = {0.3: (5.1e-3, 1.6e-3, 1.6e-3, 7.4e-3), 0.15: (4.7e-3, 1.9e-3, 3.6e-4, 2.0e-3)}


def test_the_restatement_recovers_a_known_motion():
    """pins the signs and the composition of the definition: a surface sampled analytically at t-1 and at t, moved by (1.3, -0.7, 0.05, 0.02)"""
    got = {}
    for s, h, w, origin in ((0.3, 40, 52, (20.3, 18.6)), (0.15, 80, 104, (40.3, 36.6))):
        row, _ = _pair(MH.two_bump, origin, s, h, w, MH.MOVE_A)
        err = np.abs(row[[M["tx_px"], M["ty_px"], M["theta_rad"], M["beta_mm"]]] - np.array(MH.MOVE_A))
        print("mm per px", s, "n", row[M["template_pixels"]], "estimate", row[4:8], "error", err, "rms", row[12:14], "last step", row[M["last_step_px"]])
        assert row[M["status"]] == MH.OK and row[M["iterations"]] == 8 and row[M["last_step_px"]] < 1e-3 / 4
        assert row[M["rms_after_mm"]] < 0.5 * row[M["rms_before_mm"]]
        assert (err <= 2.0 * np.array(RECOVERY_ERROR[s])).all(), (s, err)
        got[s] = err
    assert got[0.15][2] < got[0.3][2] and got[0.15][3] < got[0.3][3]              # twist and depth change gain from the finer grid


def test_a_pure_press_of_a_ball_is_not_a_slide():
    """the case the read-out exists for: a ball pressed 0.5 -> 0.8 mm deep next to a wall at the left edge of its footprint, which can grow
    to the right, up and down only.  The tracker-style (depth-weighted) centroid moves 0.38 px; the registration sees the same surface
    0.3 mm deeper.  A ball's twist is unobservable and wanders (NOT_CONVERGED by the twist alone); it reaches the translation only through
    the distance between the twist's centre and the apex, which the discrete footprint keeps below half a pixel."""
    s, h, w, R, origin = 0.15, 80, 104, 4.0, (50.3, 40.6)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    T, I = (MH.ball(R, d)((xx - origin[0]) * s, (yy - origin[1]) * s) for d in (0.5, 0.8))
    m0 = T > 0.05
    ys, xs = np.nonzero(m0)
    I[:, :xs.min()] = 0.0
    T32, I32 = T.astype(np.float32), I.astype(np.float32)

    def weighted(d, m):
        py, px = np.nonzero(m)
        dd = d[m].astype(np.float64)
        return (px * dd).sum() / dd.sum(), (py * dd).sum() / dd.sum()
    c0, c1 = weighted(T32, m0), weighted(I32, I > 0.05)
    dxy = (c1[0] - c0[0], c1[1] - c0[1])
    row = MH.register(T32, I32, m0, (xs.max() - xs.min() + 1, ys.max() - ys.min() + 1), s, dxy, dxy)
    shift, slide = float(np.hypot(*dxy)), float(np.hypot(row[M["tx_px"]], row[M["ty_px"]]))
    print("centroid shift", dxy, shift, "registered", row[4:8], "|t|", slide, "status", row[M["status"]], "tx - DX", row[18:20])
    assert row[M["status"]] in (MH.OK, MH.NOT_CONVERGED) and shift > 0.3
    assert slide <= 0.5 * abs(row[M["theta_rad"]]) + 2.0 * RECOVERY_ERROR[0.15][0]
    assert slide <= shift / 5.0                                                    # 0.037 against 0.383
    assert abs(row[M["beta_mm"]] - 0.3) < 2.0 * RECOVERY_ERROR[0.15][3]
    assert abs(row[M["tx_minus_dx"]] + dxy[0]) <= slide                            # the centroid motion is footprint change


SE_RATIO = 131.6      # what `register` gives below: se_theta of the round cap (0.0930 rad) over the anisotropic contact's (7.06e-4 rad)


def test_a_round_cap_says_its_twist_is_unobservable():
    """the same motion and the same 0.01 mm noise on frame t for an anisotropic contact and for the cap of a 9 mm ball 0.3 mm deep: the
    standard error of theta is two orders of magnitude larger for the ball (that of tx three times), and the ball is not SINGULAR (the floor test decides that)"""
    s, h, w, origin = 0.15, 80, 104, (40.3, 36.6)
    noise = np.random.default_rng(5).normal(0.0, 0.01, (h, w))
    aniso, _ = _pair(MH.two_bump, origin, s, h, w, MH.MOVE_A, noise)
    round_, _ = _pair(MH.ball(9.0, 0.3), origin, s, h, w, MH.MOVE_A, noise)
    ratio = round_[M["se_theta_rad"]] / aniso[M["se_theta_rad"]]
    print("se_theta anisotropic", aniso[M["se_theta_rad"]], "round", round_[M["se_theta_rad"]], "ratio", ratio, "rms", aniso[13], round_[13],
          "se_tx", aniso[M["se_tx_px"]], round_[M["se_tx_px"]])
    assert aniso[M["status"]] == MH.OK and round_[M["status"]] in (MH.OK, MH.NOT_CONVERGED)
    assert SE_RATIO / 10.0 <= ratio
    assert round_[M["se_tx_px"]] < 10.0 * aniso[M["se_tx_px"]]                     # the slide of a ball is as observable as anyone's


def test_cases_are_what_they_claim_and_no_verdict_hangs_on_rounding():
    bars = _bars()
    print("self-distances", bars["e"])
    for name in CASE_NAMES:
        m, f, e, ef = _reference(name)
        assert m.shape == (3, 4, 24) and np.isnan(m[..., 20:]).all() and f.shape == (3, 8)
        run = np.isin(m[..., M["status"]], (MH.OK, MH.NOT_CONVERGED))
        last = m[..., M["last_step_px"]][run]
        assert ((last < 1e-3 / 4.0) | (last > 1e-3 * 4.0)).all(), (name, last)     # OK / NOT_CONVERGED cannot flip on rounding
        assert (m[0, :, M["status"]][~np.isnan(m[0, :, 0])] == MH.NO_PARENT).all()  # before the first frame
    for size in ("40x52", "37x53"):
        st = _reference("main_" + size)[0][..., M["status"]]
        assert list(st[1]) == [MH.OK, MH.OK, MH.NOT_CONVERGED, MH.TOO_FEW] and list(st[2]) == [MH.OK, MH.NO_PARENT, MH.NO_PARENT, MH.SINGULAR]
        m = _reference("main_" + size)[0]
        assert m[1, 3, M["template_pixels"]] == 15 and m[2, 2, M["parent_row"]] == 7 and m[2, 1, M["parent_row"]] == -1
        assert _case("main_" + size)["tab"][0, 1, SH.C_X1] == int(size.split("x")[1]) - 1          # the box touches the border
        err = np.abs(m[1, 0, 4:8] - np.array(MH.MOVE_A))
        assert (err <= 2.0 * np.array(RECOVERY_ERROR[0.3])).all(), err
        e = _reference("empty_frame_" + size)
        assert np.isnan(e[0][1]).all() and np.isnan(e[1][1]).all() and e[0][2, 0, M["status"]] == MH.NO_PARENT and e[1][2, 0] == 0
        j = _reference("jump_" + size)[0]
        assert list(j[1:, 0, M["status"]]) == [MH.NOT_CONVERGED] * 2 and np.isfinite(j[1:, 0, 4:20]).all()
    nb = _reference("main_nan_background_37x53")[0]
    assert list(nb[2, :, M["status"]]) == [MH.OK, MH.NO_PARENT, MH.NO_PARENT, MH.SINGULAR]
    assert nb[2, 0, M["template_pixels"]] == _reference("main_37x53")[0][2, 0, M["template_pixels"]] - 2       # two template pixels are NaN


# ---------------------------------------------------------------------------------------------------------------- GPU, direct
def _update(pkg, c, frames=slice(None), reader=None, max_batch=None):
    import torch
    B, h, w = c["index"][frames].shape
    mo = reader or pkg.ContactMotion(h, w, max_batch or B, MH.K, **c["params"])
    out = mo.update(c["depth"][frames], c["index"][frames], c["tab"][frames], c["count"][frames], c["tracks"][frames], c["mpp"][frames], c["eps"])
    torch.cuda.synchronize()
    if reader is None:
        mo.close()
    return out["motion"].cpu().numpy(), out["motion_frame"].cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_direct_case_equals_numpy_motion(pkg, name):
    want, wantf, e, ef = _reference(name)
    bars = _bars()
    got, gotf = _update(pkg, _case(name))
    assert got.shape == want.shape and got.dtype == np.float64 and gotf.shape == wantf.shape
    assert MH.exact_equal(got, want), (name, got[..., :4], want[..., :4])
    assert MH.exact_equal(gotf, wantf, MH.FRAME_EXACT, MF), (name, gotf, wantf)
    d, df = MH.field_distances(got, want), MH.frame_distances(gotf, wantf)
    print(name, "distance to numpy_motion", d, df, "self-distance", e, ef, "bars", bars["row"], bars["frame"])
    for k in d:
        assert d[k] <= bars["row"][k], (name, k, d[k], bars["row"][k])
    for k in df:
        assert df[k] <= bars["frame"][k], (name, k, df[k], bars["frame"][k])


def _stream(c, order):
    idx = np.array(order)
    return {k: (v[idx] if isinstance(v, np.ndarray) else v) for k, v in c.items()}


@pytest.mark.gpu
def test_same_bits_whatever_the_batching(pkg):
    c = _stream(_case("main_37x53"), [0, 1, 2, 1, 2, 1, 2])
    want, wantf, _ = MH.run(c)
    whole = _update(pkg, c)
    assert MH.exact_equal(whole[0], want) and (whole[0][3:, 0, M["status"]] == MH.OK).all()
    again = _update(pkg, c)                                                        # another handle
    assert MH.same_bits(whole[0], again[0]) and MH.same_bits(whole[1], again[1])
    mo = pkg.ContactMotion(37, 53, 7, MH.K)
    first = _update(pkg, c, reader=mo)
    carried = _update(pkg, c, reader=mo)                                           # frame 0 now follows frame 6
    assert MH.same_bits(first[0], whole[0]) and MH.same_bits(carried[0], whole[0]) and MH.same_bits(carried[1], whole[1])     # its rows are born
    want2 = MH.run(c, carry=MH.run(c)[2])[0]
    assert MH.exact_equal(carried[0], want2)
    mo.reset()
    after_reset = _update(pkg, c, reader=mo)
    assert MH.same_bits(after_reset[0], whole[0]) and MH.same_bits(after_reset[1], whole[1])
    mo.reset()
    parts = [_update(pkg, c, slice(0, 3), reader=mo), _update(pkg, c, slice(3, 7), reader=mo)]
    assert MH.same_bits(np.concatenate([p[0] for p in parts]), whole[0]) and MH.same_bits(np.concatenate([p[1] for p in parts]), whole[1])
    mo.reset()
    singles = [_update(pkg, c, slice(t, t + 1), reader=mo) for t in range(7)]      # every frame first and last of its batch
    assert MH.same_bits(np.concatenate([p[0] for p in singles]), whole[0]) and MH.same_bits(np.concatenate([p[1] for p in singles]), whole[1])
    with pytest.raises(ValueError):
        pkg.ContactMotion(37, 53, 2, MH.K).update(c["depth"], c["index"], c["tab"], c["count"], c["tracks"], c["mpp"], c["eps"])      # batch > max_batch
    with pytest.raises(ValueError):
        mo.update(c["depth"], c["index"], c["tab"], c["count"], c["tracks"][:, :2], c["mpp"], c["eps"])
    with pytest.raises(ValueError):
        mo.update(c["depth"], c["index"], c["tab"], c["count"], c["tracks"], c["mpp"], float("nan"))
    mo.close()


# ---------------------------------------------------------------------------------------------------------------- GPU, through the session
def _shifted_frames(pkg, n, shifts):
    """frames of two Gaussian bumps (contacts_helpers.bumps_phase's phase model) whose centres are shifted by whole pixels"""
    cx, cy, r = pkg.synth.roi_circle(n)
    yy, xx = np.mgrid[0:n, 0:n].astype(np.float64)
    frames = []
    for t, (sx, sy) in enumerate(shifts):
        phi = np.zeros((n, n))
        for x0, y0, amp in ((cx - 0.35 * r, cy - 0.1 * r, 1.1), (cx + 0.4 * r, cy + 0.15 * r, 0.8)):
            phi -= amp * np.exp(-((xx - x0 - sx) ** 2 + (yy - y0 - sy) ** 2) / (2.0 * (0.07 * n) ** 2))
        frames.append(pkg.synth._base(n, phi, np.random.default_rng(4100 + t)))
    return np.stack(frames)


@pytest.mark.gpu
def test_session_motion_through_the_public_interface(pkg, tmp_path):
    import torch
    n, K, step = 224, 4, (3, -2)
    shifts = [(step[0] * t, step[1] * t) for t in range(4)]
    frames = _shifted_frames(pkg, n, shifts)
    model, neg = pkg.load_calibration(os.path.join(G, "calibration_phase_to_height.json"))
    fm = pkg.load_force_calibration(os.path.join(G, "calibration_height_to_force.json"))["best_model"]
    s = pkg.FtpSensor(pkg.synth.reference_frame(n), pkg.synth.roi_circle(n), pkg.FtpConfig.scaled(n), model, neg, fm, max_batch=2)
    with pytest.raises(RuntimeError):
        s.motion(K)                                      # no predict yet
    outs, carry, args = [], None, []
    for b in range(2):
        o = s.predict_batch(frames[2 * b:2 * b + 2])
        r = s.motion(K)
        torch.cuda.synchronize()
        assert set(r) == {"contacts", "count", "contact_index", "tracks", "fate", "motion", "motion_frame"}
        assert tuple(r["motion"].shape) == (2, K, 24) and tuple(r["motion_frame"].shape) == (2, 8)
        a = (o["height_map_mm"].cpu().numpy(), r["contact_index"].cpu().numpy(), r["contacts"].cpu().numpy(), r["count"].cpu().numpy(),
             r["tracks"].cpu().numpy(), o["scalars"][:, 6].cpu().numpy(), s.config.depth_eps_mm)
        want, wantf, carry = MH.numpy_motion(*a, carry=carry)
        rev = MH.numpy_motion(*a, carry=args[-1][1] if args else None, order="reversed")[0]
        fs = MH.numpy_motion(*a, carry=args[-1][1] if args else None, order="fsum")[0]
        args.append((a, carry))
        got, gotf = r["motion"].cpu().numpy(), r["motion_frame"].cpu().numpy()
        outs.append((got, a))
        cnt, trk = a[3], a[4]
        used = np.arange(K)[None, :] < np.minimum(cnt, K)[:, None]
        assert np.array_equal(~np.isnan(got[..., 0]), used) and np.isnan(got[~used]).all()
        link = used & (got[..., M["status"]] != MH.NO_PARENT)
        assert np.array_equal(got[..., M["parent_row"]][link], trk[..., MH.T_PARENT][link])                   # the tracker's rows
        assert MH.exact_equal(got, want) and MH.exact_equal(gotf, wantf, MH.FRAME_EXACT, MF)
        e = {k: max(v, MH.field_distances(want, fs)[k]) for k, v in MH.field_distances(want, rev).items()}
        d = MH.field_distances(got, want)
        print("batch", b, "count", cnt, "status", got[..., M["status"]], "tx", got[..., M["tx_px"]], "ty", got[..., M["ty_px"]], "distance", d, "self", e)
        for k in ("tx_px", "ty_px", "theta_rad", "beta_mm"):
            assert d[k] <= max(16.0 * e[k], FLOOR), (k, d[k], e[k])
        ok = got[..., M["status"]] == MH.OK
        if b:
            assert got[0, 0, M["status"]] != MH.NO_PARENT                          # frame 0 of the second batch follows the first batch
        for t, k in zip(*np.nonzero(ok)):
            err_want = max(abs(want[t, k, M["tx_px"]] - step[0]), abs(want[t, k, M["ty_px"]] - step[1]))
            err_got = max(abs(got[t, k, M["tx_px"]] - step[0]), abs(got[t, k, M["ty_px"]] - step[1]))
            print("  frame", t, "row", k, "error against the shift: restatement", err_want, "device", err_got)
            assert err_got <= err_want + max(16.0 * max(e["tx_px"], e["ty_px"]), FLOOR)
    assert (outs[0][0][0, :, M["status"]][~np.isnan(outs[0][0][0, :, 0])] == MH.NO_PARENT).all()
    assert (outs[1][0][..., M["status"]] == MH.OK).any()
    got, a = outs[1]
    path = pkg.write_motion_csv(str(tmp_path), got, a[2], a[3])
    with open(path, newline="") as fh:
        back = list(csv.DictReader(fh))
    rows = pkg.motion_table(got, a[2], a[3])
    assert len(back) == len(rows) == int(np.minimum(a[3], K).sum())
    for r, q in zip(rows, back):
        for k, v in r.items():
            assert (np.isnan(v) and np.isnan(float(q[k]))) or float(q[k]) == v, k
    # the single-frame interface: the keys, and one dict per contact
    res = s.predict(frames[3], contacts=K, motion={"reset": True})
    plain = s.predict(frames[3], contacts=K)
    assert set(res) == set(plain) | {"tracks", "motion", "motion_frame"} and "motion" not in plain
    assert len(res["motion"]) == len(res["contacts"]) == len(res["tracks"]) and all(r["status"] == MH.NO_PARENT for r in res["motion"])
    assert list(res["motion"][0])[0] == "contact" and list(res["motion"][0])[1:] == list(pkg.MOTION_NAMES)
    again = s.predict(frames[3], contacts=K, motion={})
    assert [r["parent_row"] for r in again["motion"]] == [r["parent_row"] for r in again["tracks"]]
    assert again["motion_frame"]["registered"] == sum(r["status"] == MH.OK for r in again["motion"])
    with pytest.raises(ValueError):
        s.predict(frames[3], motion={})
    s.close()
    assert s._motion is None
