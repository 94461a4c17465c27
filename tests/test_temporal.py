"""Temporal read-out (include/vistaf_temporal.h, temporal.TemporalReadout, FtpSensor.temporal): filtered depth, rate, touch state and events.

tests/temporal_helpers.py restates the definition (`numpy_temporal`, the reference of every GPU test), builds the streams and holds the bar:
the five state planes, both per-frame planes and every count, index, maximum, minimum, dwell, event and gap field must be equal, NaN pattern
included; the volume and its rate, which have a float64 sum behind them, must be within (2 N + 16) * 2^-53 of the reference relative to the
volume (for the rate: to the larger of the two volumes over the interval), N the frame's touch pixels.  The direct GPU tests hand the read-out
hand-made streams (no FTP session): 37 x 53 (an odd pixel count, every frame base misaligned: one pixel per thread) and 40 x 52 (a multiple of
4: four pixels per thread), seven frames of which the first and the fourth are skipped, and 131 x 127 x 3, whose 65 chunks take the frame
kernel round its loop twice.
"""
import csv
import ctypes
import os
import re

import numpy as np
import pytest

import temporal_helpers as TH
from temporal_helpers import R_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
SHAPES = {"37x53": (37, 53), "40x52": (40, 52)}
PARAMS = {"dyadic": TH.DYADIC, "general": TH.GENERAL}
CASES = [(s, p) for s in SHAPES for p in PARAMS]
_CASES, _REF = {}, {}


def _case(shape, params):
    key = (shape, params)
    if key not in _CASES:
        _CASES[key] = TH.big_stream() if shape == "big" else TH.stream(*SHAPES[shape], PARAMS[params])
    return _CASES[key]


def _reference(shape, params):
    key = (shape, params)
    if key not in _REF:
        _REF[key] = TH.reference(_case(shape, params))
    return _REF[key]


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_temporal_names_and_field_counts_follow_the_header(pkg):
    hdr = open(os.path.join(ROOT, "include", "vistaf_temporal.h")).read()
    idx = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define VISTAF_TEMPORAL_(\w+)\s+(\d+)\b", hdr)}
    assert sorted(idx.values()) == list(range(16))
    for name, i in idx.items():
        assert pkg.TEMPORAL_NAMES[i] == name
    assert list(pkg.TEMPORAL_NAMES) == list(pkg._lib.TEMPORAL_NAMES) == list(pkg.writers.TEMPORAL_FIELDS) == list(TH.NAMES)
    assert int(re.search(r"#define VISTAF_NTEMPORAL\s+(\d+)", hdr).group(1)) == pkg._lib.NTEMPORAL == TH.NTEMPORAL == 16
    ev = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define VISTAF_TEMPEV_(\w+)\s+(\d+)\b", hdr)}
    assert ev == pkg.TEMPORAL_EVENTS == pkg._lib.TEMPORAL_EVENTS == {"touch_began": TH.BEGAN, "touch_ended": TH.ENDED}
    for name in ("temporal", "TemporalReadout", "TEMPORAL_NAMES", "TEMPORAL_EVENTS", "temporal_table", "write_temporal_csv", "temporal_frame_record"):
        assert name in pkg.__all__ and hasattr(pkg, name)


def test_library_exports_exactly_the_declared_temporal_symbols(pkg):
    hdr = open(os.path.join(ROOT, "include", "vistaf_temporal.h")).read()
    declared = sorted(set(re.findall(r"\b(vistaf_temporal_\w+)\s*\(", hdr)))
    assert declared == sorted(["vistaf_temporal_create", "vistaf_temporal_update", "vistaf_temporal_state", "vistaf_temporal_reset",
                               "vistaf_temporal_destroy"])
    lib = pkg._lib.load()
    for name in declared:
        assert hasattr(lib, name), name
    assert sorted(pkg._lib.TEMPORAL_EXPORTS) == declared
    for other in ("vistaf_ftp.h", "vistaf_track.h", "vistaf_shape.h", "vistaf_taxel.h", "vistaf_thermal.h"):
        assert "vistaf_temporal" not in open(os.path.join(ROOT, "include", other)).read(), other      # its own header; the others are unchanged


def test_temporal_c_abi_refuses_bad_arguments_without_a_device(pkg):
    lib = pkg._lib.load()
    E_INVALID = -1
    h = ctypes.c_void_p()
    nan, inf = float("nan"), float("inf")
    good = dict(h=4, w=5, max_batch=2, alpha=0.5, on_mm=0.05, off_mm=0.02, frame_period_s=0.01)

    def create(out=None, **kw):
        a = dict(good, **kw)
        return lib.vistaf_temporal_create(a["h"], a["w"], a["max_batch"], a["alpha"], a["on_mm"], a["off_mm"], a["frame_period_s"],
                                          ctypes.byref(h) if out is None else out)
    assert lib.vistaf_temporal_create(4, 5, 2, 0.5, 0.05, 0.02, 0.01, None) == E_INVALID and b"out" in lib.vistaf_ftp_last_error()
    bad = [("alpha", v) for v in (nan, inf, -inf, 0.0, -0.5, 1.0000001, 2.0, 1e-60)] + \
          [("on_mm", v) for v in (nan, inf, -inf, 1e39)] + [("off_mm", v) for v in (nan, inf, -inf, -0.01)] + \
          [("frame_period_s", v) for v in (nan, inf, -inf, 0.0, -1.0)] + \
          [("h", 0), ("h", -1), ("h", 65537), ("w", 0), ("w", 65537), ("max_batch", 0), ("max_batch", -2), ("max_batch", 65536)]
    for name, v in bad:
        assert create(**{name: v}) == E_INVALID, (name, v)
        msg = lib.vistaf_ftp_last_error()
        assert not h.value and (name.encode() in msg or (name in ("h", "w") and b"frame size" in msg)), (name, v, msg)
    for on, off in ((0.02, 0.02), (0.02, 0.05), (0.05, 0.05 + 1e-12), (0.0, 0.0)):                   # equal after the rounding to float32 too
        assert create(on_mm=on, off_mm=off) == E_INVALID and b"on_mm" in lib.vistaf_ftp_last_error() and b"off_mm" in lib.vistaf_ftp_last_error()
    assert create(h=65536, w=32768) == E_INVALID and b"frame size" in lib.vistaf_ftp_last_error()    # h * w overflows an int
    assert create(alpha=1.0, off_mm=0.0) == 0 and h.value                                           # the ends of the ranges that are inside
    lib.vistaf_temporal_destroy(h)
    assert create() == 0 and h.value
    # create touches no device, so the checks of update run without one; nothing is launched for a refused call
    f32, mpp, rows, st = (ctypes.c_float * 64)(), (ctypes.c_double * 4)(), (ctypes.c_double * 64)(), (ctypes.c_int32 * 4)()
    assert lib.vistaf_temporal_update(None, f32, mpp, st, 1, rows, None, None, None) == E_INVALID and b"handle" in lib.vistaf_ftp_last_error()
    assert lib.vistaf_temporal_update(h, None, mpp, st, 1, rows, None, None, None) == E_INVALID and b"depth" in lib.vistaf_ftp_last_error()
    assert lib.vistaf_temporal_update(h, f32, None, st, 1, rows, None, None, None) == E_INVALID and b"mm_per_px" in lib.vistaf_ftp_last_error()
    assert lib.vistaf_temporal_update(h, f32, mpp, st, 1, None, None, None, None) == E_INVALID and b"rows" in lib.vistaf_ftp_last_error()
    for batch in (0, 3, -1):
        assert lib.vistaf_temporal_update(h, f32, mpp, None, batch, rows, None, None, None) == E_INVALID and b"batch" in lib.vistaf_ftp_last_error()
    a = ctypes.addressof(f32)
    a += (16 - a % 16) % 16                                                                         # h * w = 20 is a multiple of 4: 16-byte moves
    assert lib.vistaf_temporal_update(h, ctypes.c_void_p(a + 4), mpp, None, 1, rows, None, None, None) == E_INVALID and b"aligned" in lib.vistaf_ftp_last_error()
    assert lib.vistaf_temporal_update(h, ctypes.c_void_p(a), mpp, None, 1, rows, ctypes.c_void_p(a + 8), None, None) == E_INVALID
    assert lib.vistaf_temporal_update(h, ctypes.c_void_p(a), mpp, None, 1, rows, None, ctypes.c_void_p(a + 2), None) == E_INVALID
    assert lib.vistaf_temporal_reset(None) == E_INVALID and lib.vistaf_temporal_state(None, None, None, None, None, None, None) == E_INVALID
    assert lib.vistaf_temporal_reset(h) == 0
    lib.vistaf_temporal_destroy(h)
    lib.vistaf_temporal_destroy(None)


def test_readout_object_refuses_bad_arguments_and_needs_a_device_to_update(pkg):
    import torch
    for kw in (dict(alpha=0.0), dict(alpha=1.5), dict(on_mm=0.02, off_mm=0.02), dict(off_mm=-1.0), dict(frame_period_s=0.0), dict(max_batch=0)):
        with pytest.raises(ValueError):
            pkg.TemporalReadout(**dict(dict(h=8, w=8, max_batch=1, alpha=0.5, on_mm=0.05, off_mm=0.02, frame_period_s=0.01), **kw))
    rd = pkg.TemporalReadout(8, 8, 1, 0.5, 0.05, 0.02, 0.01)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):
            rd.update(np.zeros((1, 8, 8), np.float32), np.array([0.05]))
        with pytest.raises(RuntimeError, match="no CPU path"):
            rd.state()
    rd.reset()
    rd.close()
    rd.close()


def test_reference_alpha_one_is_the_depth_itself():
    c = _case("37x53", "dyadic")                         # depths on the 1/64 lattice: fp + (d - fp) is exact, as it is not for arbitrary floats
    rows, filt, touch, st = TH.numpy_temporal(c["depth"], c["mpp"], c["status"], 1.0, 0.5, 0.25, 1.0 / 32.0)
    d = np.where(np.isfinite(c["depth"]), c["depth"], np.float32(0.0)).astype(np.float32)
    for b in (1, 2, 4, 5, 6):
        assert TH.same_bits(filt[b], d[b]), b                                                         # bit for bit
    assert TH.same_bits(filt[3], d[2]) and TH.same_bits(filt[0], np.zeros_like(d[0]))                  # a skipped frame holds the state
    assert TH.same_bits(st["filt"].reshape(d[6].shape), d[6])
    assert np.array_equal(touch[2].ravel() != 0, d[2].ravel() >= np.float32(0.5))                     # every pixel came from touch = 0


def test_reference_constant_stream_has_constant_filter_and_zero_rate():
    rng = np.random.default_rng(5)
    plane = (rng.random((9, 11)) * 0.2).astype(np.float32)
    depth = np.repeat(plane[None], 6, axis=0)
    status = np.array([0, 0, 3, 0, 0, 0], np.int32)
    for prm in (TH.DYADIC, TH.GENERAL, dict(alpha=0.123, on_mm=0.1, off_mm=0.0, frame_period_s=0.004)):
        rows, filt, touch, st = TH.numpy_temporal(depth, np.full(6, 0.05), status, **prm)
        for b in range(6):
            assert TH.same_bits(filt[b], plane) and TH.same_bits(touch[b], touch[0]), b
        assert not st["rate"].any() and TH.same_bits(st["filt"].reshape(plane.shape), plane)
        ok = [0, 1, 3, 4, 5]
        n = rows[0, 0]
        assert n == (plane >= np.float32(prm["on_mm"])).sum() and (rows[ok, 0] == n).all()
        assert (rows[ok, 1] == [n, 0, 0, 0, 0]).all() and not rows[ok, 2:5].any() and (rows[ok, 5] == rows[0, 5]).all()
        assert np.isnan(rows[0, 6]) and not rows[ok[1:], 6].any() and (rows[:, 15] == [0, 0, 0, 1, 0, 0]).all()
        if n:
            assert (rows[ok, 9] == 0).all() and (rows[ok, 11] == 0).all() and rows[ok, 13].tolist() == [0, 1, 2, 3, 4]
            assert rows[ok, 14].tolist() == [TH.BEGAN, 0, 0, 0, 0]
            assert (st["dwell"][st["touch"] != 0] == 4).all() and (st["dwell"][st["touch"] == 0] == 5).all()


def test_reference_oscillation_between_the_thresholds_changes_no_state():
    on, off = np.float32(0.5), np.float32(0.25)
    depth = np.zeros((12, 1, 4), np.float32)
    depth[0, 0] = [0.0, 0.0, 1.0, 1.0]                                                                # pixels 2, 3 touch at once (f = d)
    swing = np.array([0.27, 0.49] * 6, np.float32)
    depth[1:, 0, 0], depth[1:, 0, 2] = swing[:11], swing[:11]                                         # one of each state swings inside the band
    depth[1:, 0, 3] = 1.0
    rows, filt, touch, st = TH.numpy_temporal(depth, np.full(12, 0.05), None, 1.0, float(on), float(off), 0.01)
    assert ((filt[1:, 0, [0, 2]] > off) & (filt[1:, 0, [0, 2]] < on)).all()                          # strictly between, in both states
    assert (touch[:, 0] == [0, 0, 1, 1]).all() and (rows[:, 0] == 2).all() and not rows[1:, 1:3].any()
    assert st["dwell"].tolist() == [12, 12, 11, 11] and rows[:, 14].tolist() == [TH.BEGAN] + [0] * 11
    assert st["hold"].tolist() == [0.0, 0.0, 1.0, 1.0]                                                # the largest raw depth since the touch began
    # the same swing with alpha 0.5 stays inside the band as well: the filter only averages values of the band
    rows, filt, touch, st = TH.numpy_temporal(depth, np.full(12, 0.05), None, 0.5, float(on), float(off), 0.01)
    assert (touch[5:, 0] == [0, 0, 1, 1]).all() and not rows[5:, 1:3].any()


def test_reference_events_and_dvolume_across_a_gap():
    depth = np.zeros((6, 1, 2), np.float32)
    depth[[1, 2], 0, 0] = 2.0
    status = np.array([0, 0, 7, 0, 0, 0], np.int32)                                                  # frame 2 is skipped
    rows, filt, touch, st = TH.numpy_temporal(depth, np.full(6, 0.1), status, 1.0, 0.5, 0.25, 0.5)
    assert rows[:, 14].tolist()[:2] == [0, TH.BEGAN] and np.isnan(rows[2, 14]) and rows[3:, 14].tolist() == [TH.ENDED, 0, 0]
    v = 2.0 * (0.1 * 0.1) / 1000.0
    assert rows[1, 5] == v and rows[1, 6] == v / 0.5 and rows[3, 5] == 0.0 and rows[3, 6] == (0.0 - v) / (2.0 * 0.5) and rows[3, 15] == 1
    assert np.isnan(rows[0, 6]) and np.isnan(rows[3, 7:14]).all() and rows[1, 7] == 2.0 and rows[1, 8] == 0 and rows[1, 9] == 4.0


def _hand_made():
    t = np.full((3, 16), np.nan)
    t[0] = [12, 3, 1, 7, 4, 1.5e-5, np.nan, 0.9, 417, 3.5, 418, -2.25, 12, 6, 1, 0]
    t[1, 15] = 0                                                                                      # a skipped frame
    t[2] = [0, 0, 12, 0, 0, 0.0, -1.5e-5 / 0.02, np.nan, np.nan, np.nan, np.nan, np.nan, np.nan, np.nan, 2, 1]
    return t


def test_temporal_table_and_csv_round_trip(pkg, tmp_path):
    t = _hand_made()
    rows = pkg.temporal_table(t)
    ints = ("frame", "skipped") + tuple(pkg.writers.TEMPORAL_INT_FIELDS)
    assert [(r["frame"], r["skipped"]) for r in rows] == [(0, 0), (1, 1), (2, 0)] and list(rows[0])[2:] == list(pkg.TEMPORAL_NAMES)
    for r in rows:
        assert all(isinstance(r[k], int) for k in ints) and all(isinstance(v, float) for k, v in r.items() if k not in ints)
    assert rows[0]["touch_pixels"] == 12 and rows[0]["argmax_index"] == 417 and rows[0]["min_rate_mm_per_s"] == -2.25 and rows[0]["events"] == 1
    assert np.isnan(rows[0]["dvolume_cm3_per_s"]) and rows[1]["touch_pixels"] == -1 and rows[1]["gap_frames"] == 0 and rows[1]["events"] == -1
    assert rows[2]["argmax_index"] == -1 and rows[2]["longest_dwell_frames"] == -1 and rows[2]["events"] == 2 and rows[2]["gap_frames"] == 1
    assert len(pkg.temporal_table(t[0])) == 1
    with pytest.raises(ValueError):
        pkg.temporal_table(t[:, :8])
    path = pkg.write_temporal_csv(str(tmp_path), t)
    with open(path, newline="") as f:
        back = list(csv.DictReader(f))
    assert len(back) == 3 and list(back[0]) == ["frame", "skipped"] + list(pkg.TEMPORAL_NAMES)
    for r, s in zip(rows, back):
        for k, v in r.items():
            got = float(s[k])
            assert (np.isnan(v) and np.isnan(got)) or got == v, k
    rec = pkg.temporal_frame_record(t[0])
    assert list(rec) == list(pkg.TEMPORAL_NAMES) and all(rec[k] == rows[0][k] for k in rec if k != "dvolume_cm3_per_s") and np.isnan(rec["dvolume_cm3_per_s"])
    with pytest.raises(ValueError):
        pkg.temporal_frame_record([1.0, 2.0])


# ---------------------------------------------------------------------------------------------------------------- GPU, direct
def _run(pkg, c, cuts=None, planes=True, reader=None, reset=False):
    """the stream of case c through one read-out, cut into updates of the given lengths; host arrays (rows, filtered, touch, state)"""
    import torch
    depth, mpp, status = c["depth"], c["mpp"], c["status"]
    B = depth.shape[0]
    cuts = cuts or [B]
    assert sum(cuts) == B
    rd = reader or pkg.TemporalReadout(*c["shape"], max(cuts), **c["params"])
    if reset:
        rd.reset()
    outs, lo = [], 0
    for n in cuts:
        outs.append(rd.update(depth[lo:lo + n], mpp[lo:lo + n], None if status is None else status[lo:lo + n], planes=planes))
        lo += n
    st = rd.state()
    torch.cuda.synchronize()
    rows = torch.cat([o["frames"] for o in outs]).cpu().numpy()
    filt = torch.cat([o["filtered"] for o in outs]).cpu().numpy() if planes else None
    touch = torch.cat([o["touch"] for o in outs]).cpu().numpy() if planes else None
    state = {k: v.cpu().numpy() for k, v in st.items()}
    if reader is None:
        rd.close()
    return rows, filt, touch, state


def _against_reference(got, want, c, what):
    rows, filt, touch, state = got
    wrows, wfilt, wtouch, wst = want
    assert rows.dtype == np.float64 and rows.shape == wrows.shape
    assert TH.exact_rows_equal(rows, wrows), (what, rows, wrows)
    worst, where = TH.worst_excess(rows, wrows, c["params"]["frame_period_s"])
    print(what, "largest error of the summed fields in units of the bar", worst, "at", where)
    assert worst <= 1.0, (what, worst, where)
    assert TH.same_bits(filt, wfilt) and TH.same_bits(touch, wtouch), what                            # NaN-free planes: bits
    for name, dtype in TH.STATE_PLANES:
        assert state[name].dtype == dtype and TH.same_bits(state[name].ravel(), wst[name]), (what, name)


def _same(a, b, planes=True):
    ok = TH.same_bits(a[0], b[0]) and all(TH.same_bits(a[3][k], b[3][k]) for k, _ in TH.STATE_PLANES)
    return ok and (not planes or (TH.same_bits(a[1], b[1]) and TH.same_bits(a[2], b[2])))


@pytest.mark.gpu
@pytest.mark.parametrize("shape,params", CASES)
def test_direct_stream_equals_numpy_temporal(pkg, shape, params):
    c = _case(shape, params)
    _against_reference(_run(pkg, c), _reference(shape, params), c, shape + " " + params)


@pytest.mark.gpu
def test_chunks_beyond_one_round_of_the_frame_kernel(pkg):
    c = _case("big", "dyadic")
    got = _run(pkg, c)
    _against_reference(got, _reference("big", "dyadic"), c, "131x127")
    assert _same(got, _run(pkg, c, cuts=[1, 2]))


@pytest.mark.gpu
@pytest.mark.parametrize("shape,params", [("37x53", "general"), ("40x52", "dyadic")])
def test_cut_invariance_handles_reset_and_planes(pkg, shape, params):
    c = _case(shape, params)
    whole = _run(pkg, c)
    for cuts in ([1, 6], [3, 4], [1] * 7):
        assert _same(whole, _run(pkg, c, cuts=cuts)), cuts                                            # rows, planes and state, bit for bit
    rd = pkg.TemporalReadout(*c["shape"], 7, **c["params"])
    first = _run(pkg, c, reader=rd)
    assert _same(whole, first)                                                                        # two handles, the same bits
    again = _run(pkg, c, reader=rd, reset=True)
    assert _same(first, again)                                                                        # reset, then the same stream
    on = _run(pkg, c, reader=rd)                                                                      # without reset the stream goes on: primed, touching
    assert not TH.same_bits(on[0], first[0]) and on[0][1, R_["touch_pixels"]] > 0 and on[0][0, R_["gap_frames"]] == 0
    want = TH.numpy_temporal(c["depth"], c["mpp"], c["status"], state=_reference(shape, params)[3], **c["params"])
    _against_reference(on, want, c, shape + " continued")
    rd.reset()
    zero = rd.state()
    assert all(not v.cpu().numpy().any() for v in zero.values())                                      # after reset, before the next update
    bare = _run(pkg, c, planes=False, reader=rd)
    assert bare[1] is None and _same(whole, bare, planes=False)                                       # planes=False: the same rows and state
    with pytest.raises(ValueError):
        rd.update(c["depth"][:, :-1], c["mpp"])
    with pytest.raises(ValueError):
        rd.update(c["depth"], c["mpp"][:3])
    with pytest.raises(ValueError):
        pkg.TemporalReadout(*c["shape"], 3, **c["params"]).update(c["depth"], c["mpp"])              # batch > max_batch
    rd.close()


# ---------------------------------------------------------------------------------------------------------------- GPU, through the session
@pytest.mark.gpu
def test_session_press_and_release(pkg):
    import torch
    n = 224
    scales = [0.0, 0.0, 0.5, 1.0, 1.0, 0.5, 0.0, 0.0, 0.0, 0.0]                                       # press and release of one synthetic bump
    nb = len(scales)
    frames = np.stack([pkg.synth.deformed_frame(n, 0, amp_scale=a) for a in scales])
    model, neg = pkg.load_calibration(os.path.join(G, "calibration_phase_to_height.json"))
    fm = pkg.load_force_calibration(os.path.join(G, "calibration_height_to_force.json"))["best_model"]
    s = pkg.FtpSensor(pkg.synth.reference_frame(n), pkg.synth.roi_circle(n), pkg.FtpConfig.scaled(n), model, neg, fm, max_batch=nb)
    with pytest.raises(RuntimeError):
        s.temporal()                                                                                  # no predict yet
    o = s.predict_batch(frames)
    before = {k: v.clone() for k, v in o.items()}
    plain = {k: v.clone() for k, v in s.contacts(8, index_plane=True).items()}
    sc, st, hm = o["scalars"].cpu().numpy(), o["status"].cpu().numpy(), o["height_map_mm"]
    assert (st == 0).all()
    peak = float(sc[:, pkg.SCALAR_NAMES.index("max_depth_mm")].max())
    prm = dict(alpha=0.5, on_mm=0.5 * peak, off_mm=0.25 * peak, frame_period_s=1.0 / 30.0)             # thresholds from the press itself
    got = s.temporal(planes=True, **prm)
    rd = pkg.TemporalReadout(n, n, nb, **prm)
    own = rd.update(hm, o["scalars"][:, pkg.SCALAR_NAMES.index("mm_per_px")], o["status"], planes=True)
    torch.cuda.synchronize()
    assert set(got) == {"frames", "filtered", "touch"} and tuple(got["frames"].shape) == (nb, 16)
    for k in got:
        assert TH.same_bits(got[k].cpu().numpy(), own[k].cpu().numpy()), k                            # the session hands over the predict's tensors
    rd.close()
    rows = got["frames"].cpu().numpy()
    c = dict(params=prm)
    want = TH.numpy_temporal(hm.cpu().numpy(), sc[:, pkg.SCALAR_NAMES.index("mm_per_px")], st, **prm)
    _against_reference((rows, got["filtered"].cpu().numpy(), got["touch"].cpu().numpy(), {k: v.cpu().numpy() for k, v in s._temporal.state().items()}),
                       want, c, "session")
    ev = want[0][:, R_["events"]].astype(int)
    print("touch pixels", want[0][:, 0].tolist(), "events", ev.tolist(), "peak", peak)
    began, ended = np.flatnonzero(ev & TH.BEGAN), np.flatnonzero(ev & TH.ENDED)
    assert len(began) == 1 and len(ended) == 1 and 2 <= began[0] <= 4 < ended[0]                       # while the bump is pressed; after it is let go
    assert np.array_equal(rows[:, R_["events"]].astype(int), ev)
    # the session is not disturbed: the predict's tensors and a following contacts() are what they were
    assert all(TH.same_bits(o[k].cpu().numpy(), before[k].cpu().numpy()) for k in o)
    after = s.contacts(8, index_plane=True)
    assert all(TH.same_bits(after[k].cpu().numpy(), plain[k].cpu().numpy()) for k in plain)
    first = s._temporal
    s.temporal(**prm)
    assert s._temporal is first                                                                       # reused, the stream goes on
    with pytest.raises(ValueError):
        s.temporal(**dict(prm, alpha=0.25))                                                           # changed parameters need reset=True
    s.temporal(reset=True, **dict(prm, alpha=0.25))
    assert s._temporal is not first and s._temporal.alpha == 0.25
    s.close()
    assert s._temporal is None


@pytest.mark.gpu
def test_predict_temporal_argument(pkg):
    n = 224
    model, neg = pkg.load_calibration(os.path.join(G, "calibration_phase_to_height.json"))
    fm = pkg.load_force_calibration(os.path.join(G, "calibration_height_to_force.json"))["best_model"]
    s = pkg.FtpSensor(pkg.synth.reference_frame(n), pkg.synth.roi_circle(n), pkg.FtpConfig.scaled(n), model, neg, fm, max_batch=1)
    frame = pkg.synth.deformed_frame(n, 0)
    plain = s.predict(frame)
    prm = dict(alpha=1.0, on_mm=0.5 * plain["max_depth_mm"], off_mm=0.25 * plain["max_depth_mm"], frame_period_s=0.02)
    res = s.predict(frame, temporal=prm)
    assert set(res) == set(plain) | {"temporal_frame"} and "temporal_frame" not in plain and set(s.predict(frame)) == set(plain)
    f = res["temporal_frame"]
    assert list(f) == list(pkg.TEMPORAL_NAMES) and isinstance(f["touch_pixels"], int) and f["touch_pixels"] >= 1
    assert f["events"] == TH.BEGAN and f["gap_frames"] == 0 and np.isnan(f["dvolume_cm3_per_s"])
    assert f["max_filtered_mm"] == plain["max_depth_mm"] and f["argmax_index"] == plain["argmax_depth_index"]    # alpha = 1: the depth itself
    again = s.predict(frame, temporal=prm)["temporal_frame"]                                          # the stream goes on: the same frame again
    assert again["events"] == 0 and again["touch_pixels"] == f["touch_pixels"] and again["max_rate_mm_per_s"] == 0.0 and again["longest_dwell_frames"] == 1
    assert again["dvolume_cm3_per_s"] == 0.0 and again["onset_pixels"] == 0
    s.close()
