"""Surface texture read-out (include_ext/vistaf_texture.h, contact_textures, FtpSensor.textures): roughness, lay and pitch of every contact.

The definition is restated in tests/texture_helpers.py: `numpy_textures` (form by lstsq) and `numpy_textures_ne` (normal equations), every sum
an fsum.  The device is held stage by stage (texture_helpers.hold_device: S1 form, S2 residual plane bit for bit, S3 sums within the
order-independent summation bound pushed through each field's expression, S4 decisions bit for bit on the device's own window) and end to
end on the decision fields (hold_end_to_end), which needs that no comparison of a case sits on its edge: `decision_margin` >= 1e-9 is
asserted on the CPU for every case.  Analytic ridges pin the numbers independently of the restatement.

The flat case (an 8 x 8 rectangle of constant depth 0.5, degree 0) is held against the normal-equation restatement: m = 64 makes its solve
exact, as the device's, so every residual is 0 and the row is flat; lstsq leaves one rounding of the mean (1.1e-16) in every residual, which
is a rough surface of that height, not a flat one."""
import csv
import ctypes
import json
import os
import re

import numpy as np
import pytest

import contacts_helpers as CH
import texture_helpers as TH
from abi_helpers import _hold_against, _prototypes
from texture_helpers import T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
HEADER = os.path.join(ROOT, "include_ext", "vistaf_texture.h")
E_INVALID = -1
MARGIN = 1e-9
EXACT_BY_NE = ("flat",)
_CASES, _REF = {}, {}


def _case(name):
    if not _CASES:
        _CASES.update(TH.cases())
    return _CASES[name]


def _reference(name):
    """(reference restatement, normal-equation restatement) of a case, computed once"""
    if name not in _REF:
        c = _case(name)
        ne = TH.numpy_textures_ne(c)
        _REF[name] = (ne if name in EXACT_BY_NE else TH.numpy_textures(c), ne)
    return _REF[name]


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_texture_names_and_signatures_follow_the_header(pkg):
    hdr = open(HEADER).read()
    idx = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define VISTAF_TEXTURE_(\w+)\s+(\d+)\b", hdr)}
    assert (idx.pop("min_lag"), idx.pop("max_lag")) == (pkg._lib.TEXTURE_MIN_LAG, pkg._lib.TEXTURE_MAX_LAG) == (2, 31)
    assert sorted(idx.values()) == list(range(34))
    for name, i in idx.items():
        assert pkg.TEXTURE_NAMES[i] == name
    assert list(pkg.TEXTURE_NAMES) == list(pkg._lib.TEXTURE_NAMES) == list(pkg.writers.TEXTURE_FIELDS) == list(TH.FIELDS)
    assert int(re.search(r"#define VISTAF_NTEXTURE\s+(\d+)", hdr).group(1)) == pkg._lib.NTEXTURE == TH.NTEXTURE == 40
    status = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define VISTAF_TEXTUREFORM_(\w+)\s+(\d+)\b", hdr)}
    assert status == pkg._lib.TEXTURE_FORM == pkg.texture.TEXTURE_FORM == {"ok": TH.OK, "none": TH.NONE, "flat": TH.FLAT}
    assert set(pkg.writers.TEXTURE_INT_FIELDS) == set(TH.INT_FIELDS)
    for name in ("texture", "TEXTURE_NAMES", "TextureWorkspace", "contact_textures", "textures_table", "write_textures_csv", "texture_frame_record"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    # the header is outside include/*.h, whose prototype count tests/test_abi_surface.py pins; the rule of that test, for these functions
    protos = _prototypes(hdr)
    table = pkg._lib.TEXTURE_SIGNATURES
    assert sorted(protos) == sorted(table) == ["vistaf_texture_measure", "vistaf_texture_workspace_bytes"]
    assert not set(table) & ({n for g in pkg._lib.SIGNATURES.values() for n in g} | set(pkg._lib.OUTLINE_SIGNATURES))
    _hold_against(protos, table, pkg._lib.load())
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other.endswith(".h"):
            assert "vistaf_texture" not in open(os.path.join(ROOT, "include", other)).read(), other


def test_texture_c_abi_refuses_with_the_arguments_name(pkg):
    lib = pkg._lib.load()
    err = lib.vistaf_ftp_last_error
    n = ctypes.c_size_t(1)
    assert lib.vistaf_texture_workspace_bytes(8, 8, 1, 8, 8, None) == E_INVALID and b"bytes" in err()
    for a, word in (((0, 8, 1, 8, 8), b"h "), ((8, 0, 1, 8, 8), b"w "), ((65536, 65536, 1, 8, 8), b"h * w"), ((8, 8, 0, 8, 8), b"max_batch"),
                    ((8, 8, -3, 8, 8), b"max_batch"), ((8, 8, 1, 0, 8), b"max_contacts"), ((8, 8, 1, 65, 8), b"max_contacts"),
                    ((8, 8, 1, 8, 1), b"max_lag"), ((8, 8, 1, 8, 32), b"max_lag")):
        n.value = 1
        assert lib.vistaf_texture_workspace_bytes(*a, ctypes.byref(n)) == E_INVALID and n.value == 0 and word in err(), a
    assert lib.vistaf_texture_workspace_bytes(8, 8, 2, 8, 8, ctypes.byref(n)) == 0
    assert n.value >= 2 * 8 * 9 * 17 * 12                                  # a float64 sum and an int32 count per row and half-plane lag
    assert pkg.texture.workspace_bytes(8, 8, 2, 8, 8) == n.value
    two = n.value
    assert lib.vistaf_texture_workspace_bytes(8, 8, 1, 8, 8, ctypes.byref(n)) == 0 and n.value <= two
    with pytest.raises(ValueError, match="max_lag"):
        pkg.texture.workspace_bytes(8, 8, 1, 8, 40)
    # measure: host memory stands in for the device's, every call is refused before any HIP call
    f64, f32, i32, i8 = (ctypes.c_double * 4096)(), (ctypes.c_float * 64)(), (ctypes.c_int32 * 64)(), (ctypes.c_int8 * 64)()
    raw = (ctypes.c_uint8 * 1024)()
    ws = (ctypes.addressof(raw) + 255) & ~255
    p = ctypes.addressof
    good = dict(dep=p(f32), idx=p(i8), tab=p(f64), cnt=p(i32), mpp=p(f64), eps=0.01, frac=0.5, deg=2, L=8, thr=0.2, pm=0.3, h=8, w=8, B=1, K=8,
                out=p(f64), res=p(f32), acf=p(f64), ws=ws, n=n.value)

    def call(**kw):
        a = dict(good, **kw)
        return lib.vistaf_texture_measure(a["dep"], a["idx"], a["tab"], a["cnt"], a["mpp"], a["eps"], a["frac"], a["deg"], a["L"], a["thr"], a["pm"],
                                          a["h"], a["w"], a["B"], a["K"], a["out"], a["res"], a["acf"], a["ws"], a["n"], None)
    nan, inf = float("nan"), float("inf")
    for kw, words in ((dict(dep=None), [b"d_depth_mm"]), (dict(idx=None), [b"d_contact_index"]), (dict(tab=None), [b"d_contacts"]),
                      (dict(cnt=None), [b"d_count"]), (dict(mpp=None), [b"d_mm_per_px"]), (dict(out=None), [b"d_textures"]),
                      (dict(res=None), [b"d_residual_mm"]), (dict(acf=None), [b"d_acf"]), (dict(ws=None), [b"d_workspace"]),
                      (dict(h=0), [b"h "]), (dict(w=-1), [b"w "]), (dict(h=65536, w=65536), [b"h * w"]), (dict(B=0), [b"batch"]),
                      (dict(K=0), [b"max_contacts"]), (dict(K=65), [b"max_contacts"]), (dict(L=1), [b"max_lag"]), (dict(L=32), [b"max_lag"]),
                      (dict(eps=nan), [b"depth_eps_mm"]), (dict(eps=inf), [b"depth_eps_mm"]), (dict(frac=-0.1), [b"eval_min_fraction"]),
                      (dict(frac=1.0), [b"eval_min_fraction"]), (dict(frac=nan), [b"eval_min_fraction"]), (dict(deg=-1), [b"form_degree"]),
                      (dict(deg=3), [b"form_degree"]), (dict(thr=0.0), [b"acf_threshold"]), (dict(thr=1.0), [b"acf_threshold"]),
                      (dict(thr=nan), [b"acf_threshold"]), (dict(pm=0.0), [b"peak_min"]), (dict(pm=1.5), [b"peak_min"]), (dict(pm=nan), [b"peak_min"]),
                      (dict(tab=p(f64) + 4), [b"d_contacts", b"aligned"]), (dict(res=p(f32) + 2), [b"d_residual_mm", b"aligned"]),
                      (dict(ws=ws + 128), [b"d_workspace", b"aligned"]), (dict(n=n.value - 1), [b"workspace_bytes"]), (dict(n=0), [b"workspace_bytes"]),
                      (dict(B=2), [b"workspace_bytes"])):                  # a workspace sized for one frame does not take two
        assert call(**kw) == E_INVALID, kw
        assert all(word in err() for word in words), (kw, err())


def _hand_table():
    t = np.full((2, 3, 40), np.nan)
    t[0, 0, :34] = [613, 0, 1.2, 0.01, -0.02, -0.1, 0.003, -0.05, 0.0127, 0.0141, -0.01, 1.52, 0.021, 0.0205, 0.0415, 901, 1033, 520, 0.064, 0.002,
                    0.866, 0.5, 0.9999, 289, 37, 1, 0.325, 1, 1, 1.84, 0.177, 1.363, 0.985, 9]
    t[0, 1, :2] = [5, 1]
    t[1, 0, :8] = [64, 2, 0.5, 0, 0, 0, 0, 0]
    t[1, 0, [8, 9, 12, 13, 14]] = 0.0
    t[1, 0, [15, 16]] = 540
    return t, np.array([2, 1], np.int32)


def test_texture_writers_round_trip(pkg, tmp_path):
    t, n = _hand_table()
    rows = pkg.textures_table(t, n)
    assert [(r["frame"], r["contact"]) for r in rows] == [(0, 0), (0, 1), (1, 0)]
    assert list(rows[0])[2:] == list(pkg.TEXTURE_NAMES)
    for r in rows:
        assert all(isinstance(r[k], int) for k in TH.INT_FIELDS) and all(isinstance(r[k], float) for k in TH.FIELDS if k not in TH.INT_FIELDS)
    assert rows[0]["eval_pixels"] == 613 and rows[0]["sal_lag_x"] == 1 and rows[0]["pitch_mm"] == 1.363 and rows[0]["profile_samples"] == 9
    assert rows[1]["form_status"] == 1 and rows[1]["grad_pixels"] == -1 and np.isnan(rows[1]["sq_mm"])
    assert rows[2]["form_status"] == 2 and rows[2]["sq_mm"] == 0.0 and rows[2]["sp_pixel"] == 540 and rows[2]["lobe_status"] == -1
    with pytest.raises(ValueError):
        pkg.textures_table(t[..., :20], n)
    path = pkg.write_textures_csv(str(tmp_path), t, n)
    back = list(csv.DictReader(open(path, newline="")))
    assert len(back) == 3 and list(back[0]) == ["frame", "contact"] + list(pkg.TEXTURE_NAMES)
    for r, q in zip(rows, back):
        for name in pkg.TEXTURE_NAMES:
            v = float(q[name])
            assert v == r[name] or (np.isnan(v) and np.isnan(r[name])), name
    acf = np.full((3, 5, 5), np.nan)
    acf[0, 2, 2] = 1.0
    acf[0, 2, 3] = acf[0, 2, 1] = 0.25
    rec = pkg.texture_frame_record(t[0], 2, acf)
    assert rec["contact_count"] == 2 and [r["contact"] for r in rec["textures"]] == [0, 1] and "frame" not in rec["textures"][0]
    assert rec["textures"][1]["sq_mm"] is None and rec["textures"][0]["str"] == 0.177
    assert rec["acf"][0][2] == [None, 0.25, 1.0, 0.25, None] and rec["acf"][1][0] == [None] * 5
    assert json.loads(json.dumps(rec)) == rec                             # nothing in it that JSON cannot hold
    assert "acf" not in pkg.texture_frame_record(t[0], 2)
    with pytest.raises(ValueError):
        pkg.texture_frame_record(t[0], 2, acf[:, :4])


def test_contact_textures_needs_a_device_or_refuses_bad_arguments(pkg):
    import torch
    if not torch.cuda.is_available():
        c = _case("flat")
        a, kw = TH.args(c)
        with pytest.raises(RuntimeError, match="no CPU path"):
            pkg.contact_textures(*a, **kw)
    with pytest.raises(ValueError, match="max_lag"):
        pkg.TextureWorkspace(8, 8, 1, 8, 1, device="cpu")


def test_both_restatements_agree_on_every_case():
    for name in TH.CASE_NAMES:
        c = _case(name)
        ref, ne = _reference(name)
        a, b = ref["textures"], ne["textures"]
        exact = [T[f] for f in TH.INT_FIELDS + ("sal_mm", "rmax_mm", "str")]
        assert np.array_equal(np.isnan(a), np.isnan(b)) and TH.same(a[..., exact], b[..., exact]), name
        assert np.isnan(a[..., 34:]).all() and np.array_equal(np.isnan(ref["residual"]), np.isnan(ne["residual"])), name
        assert np.array_equal(np.isnan(ref["acf"]), np.isnan(ne["acf"])), name
        # the two forms differ by rounding only, and the float fields with them: a residual by one float32 step at most (2^-23 of the peak)
        e = TH.form_distance(c, b, a)
        assert max(4.0 * e, 64.0 * TH.ULP) < 1e-9, (name, e)
        peak = np.nanmax(np.abs(c["tab"][..., TH.C_PEAK]))
        both = ~np.isnan(ref["residual"])
        assert np.abs(ref["residual"][both].astype(np.float64) - ne["residual"][both]).max(initial=0.0) <= 2.0 ** -23 * peak, name
        fl = [T[f] for f in ("sa_mm", "sq_mm", "sp_mm", "sv_mm", "sdq", "coherence", "pitch_mm", "pitch_acf")]
        assert np.allclose(a[..., fl], b[..., fl], rtol=1e-5, atol=1e-12, equal_nan=True), name


def test_expected_statuses_and_nan_patterns():
    def rows(name, b=0):
        return _reference(name)[0]["textures"][b]
    sm = rows("small_degree_2")
    # a 3 x 20 bar: measured, but rows of lags beyond dy = 2 do not exist: most lags invalid, the lobe open
    assert sm[0, T["eval_pixels"]] == 60 and sm[0, T["form_status"]] == TH.OK and sm[0, T["lobe_status"]] == 1
    assert sm[0, T["acf_valid_lags"]] < 0.5 * 17 * 17
    # a single pixel, five pixels (m < 6), a one-row line under degree 2 (v is 0 on all of it: the floor refuses): no form
    for k, m in ((1, 1), (2, 5), (3, 22)):
        assert sm[k, T["eval_pixels"]] == m and sm[k, T["form_status"]] == TH.NONE and np.isnan(sm[k, 2:]).all()
    res = _reference("small_degree_2")[0]["residual"][0]
    assert np.isnan(res[30, 28:50]).all() and np.isnan(res[10, 30]) and not np.isnan(res[4, 4:24]).any()
    line = rows("small_degree_0")[3]                                        # the same line with degree 0 is measured
    assert line[T["form_status"]] == TH.OK and line[T["eval_pixels"]] == 22 and line[T["sq_mm"]] > 0 and line[T["grad_pixels"]] == 0
    assert np.isnan(line[[T["sdq"], T["sdr"], T["grad_dir_x"], T["grad_dir_y"], T["coherence"], T["pitch_mm"]]]).all()
    assert line[T["profile_samples"]] == 1 and line[T["acf_valid_lags"]] > 0 and line[T["lobe_status"]] == 1
    flat = rows("flat")[0]
    assert flat[T["eval_pixels"]] == 64 and flat[T["form_status"]] == TH.FLAT and flat[T["form_c0"]] == 0.5
    assert all(flat[T[n]] == 0.0 for n in ("sa_mm", "sq_mm", "sp_mm", "sv_mm", "sz_mm")) and flat[T["sp_pixel"]] == flat[T["sv_pixel"]] == 10 * TH.W + 10
    assert np.isnan(flat[[T["ssk"], T["sku"]]]).all() and np.isnan(flat[T["grad_pixels"]:]).all()
    assert (_reference("flat")[0]["residual"][0, 10:18, 10:18] == 0.0).all() and np.isnan(_reference("flat")[0]["acf"]).all()
    te = _reference("table_edges")[0]["textures"]
    assert np.isnan(te[0, 2]).all() and np.isnan(te[1]).all() and not np.isnan(te[2, :, 0]).any()          # count 2, count 0, count 7 > K
    assert np.isnan(_reference("table_edges")[0]["residual"][0, 2:10, 30:41]).all()                          # row 2 of the plane is nobody's there
    assert te[3, 0, T["form_status"]] == TH.OK and te[3, 1, T["form_status"]] == TH.NONE                     # NaN depths: left out; inf: no form
    assert list(te[4, :2, T["eval_pixels"]]) == [0, 0] and list(te[4, :2, T["form_status"]]) == [TH.NONE, TH.NONE]      # no box
    nb = _reference("neighbours_and_ring")[0]
    # two contacts one pixel apart: a pair across them does not count, so no lag of row 0 has more pairs than its own 16 x 19 pixels give
    assert nb["aux"][(0, 0)]["N"].max() == 16 * 19 and nb["aux"][(0, 0)]["N"][8, 9] == 15 * 19
    e = _reference("frame_edge")[0]["textures"][0, 0]
    assert e[T["form_status"]] == TH.OK and e[T["acf_valid_lags"]] > 0
    assert rows("lag_31")[0, T["acf_valid_lags"]] < 63 * 63 and rows("lag_2")[0, T["acf_valid_lags"]] == 25


@pytest.mark.parametrize("phi", TH.RIDGE_PHIS)
def test_restatement_meets_the_analytic_conditions(phi):
    _analytic(_reference("ridges_%g" % phi)[0]["textures"][0, 0], phi)


def _analytic(row, phi):
    s = TH.CAP["s"]
    ang = np.degrees(np.arctan2(row[T["grad_dir_y"]], row[T["grad_dir_x"]]))
    off = abs((ang - phi + 90.0) % 180.0 - 90.0)
    print("phi", phi, "pitch/s", row[T["pitch_mm"]] / s, "direction off by", off, "coherence", row[T["coherence"]], "sq",
          row[T["sq_mm"]] / (0.02 / np.sqrt(2.0)), "sal/s", row[T["sal_mm"]] / s)
    assert abs(row[T["pitch_mm"]] / s - 6.0) <= 0.5
    assert off <= 5.0
    assert row[T["coherence"]] >= 0.95
    assert abs(row[T["sq_mm"]] - 0.02 / np.sqrt(2.0)) <= 0.01 * 0.02 / np.sqrt(2.0)
    assert row[T["lobe_status"]] == 1 and row[T["sal_mm"]] / s <= 2.0


def _analytic_others(short, noise):
    assert np.isnan(short[T["pitch_mm"]]) and np.isnan(short[T["pitch_acf"]]) and short[T["form_status"]] == TH.OK       # L = 4: no pitch
    print("white noise coherence", noise[T["coherence"]])
    assert noise[T["coherence"]] < 0.2 and np.isnan(noise[T["pitch_mm"]])


def test_restatement_short_window_and_white_noise():
    _analytic_others(_reference("ridges_30_lag_4")[0]["textures"][0, 0], _reference("white_noise")[0]["textures"][0, 0])


def _native():
    """(case, reference restatement, forms of the normal-equation restatement) of the native-size case, computed once"""
    if "native" not in _REF:
        c = TH.native_case()
        _REF["native"] = (c, TH.numpy_textures(c), TH.numpy_textures_ne(c, forms_only=True))
    return _REF["native"]


def test_no_decision_of_any_case_sits_on_its_edge():
    for name in TH.CASE_NAMES:
        margin = TH.decision_margin(_case(name), _reference(name)[0])
        print(name, "decision margin", margin)
        assert margin >= MARGIN, (name, margin)
    c, ref, _ = _native()
    margin = TH.decision_margin(c, ref)
    print("native decision margin", margin)
    assert margin >= MARGIN


# ---------------------------------------------------------------------------------------------------------------- GPU, direct
def _measure(pkg, c, ws=None):
    import torch
    a, kw = TH.args(c)
    out = pkg.contact_textures(*a, ws, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("name", TH.CASE_NAMES)
def test_direct_case_is_held_stage_by_stage_and_end_to_end(pkg, name):
    c = _case(name)
    ref, ne = _reference(name)
    got = _measure(pkg, c)
    TH.hold_device(c, got, ref, ne)
    TH.hold_end_to_end(c, got, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("phi", TH.RIDGE_PHIS)
def test_analytic_ridges_on_the_device(pkg, phi):
    _analytic(_measure(pkg, _case("ridges_%g" % phi))["textures"][0, 0], phi)


@pytest.mark.gpu
def test_short_window_and_white_noise_on_the_device(pkg):
    _analytic_others(_measure(pkg, _case("ridges_30_lag_4"))["textures"][0, 0], _measure(pkg, _case("white_noise"))["textures"][0, 0])


@pytest.mark.gpu
def test_batch_equals_frames_one_by_one_and_two_calls_give_the_same_bits(pkg):
    c = _case("five_frames")
    ws = pkg.TextureWorkspace(TH.H, TH.W, 5, c["K"], c["L"])
    whole, again = _measure(pkg, c, ws), _measure(pkg, c, ws)
    for k in ("textures", "residual", "acf"):
        assert TH.same_bits(whole[k], again[k]), k                          # every bit, NaNs included
    for b in range(5):
        one = {k: (v[b:b + 1] if isinstance(v, np.ndarray) else v) for k, v in c.items()}
        got = _measure(pkg, one, ws)
        for k in ("textures", "residual", "acf"):
            assert TH.same_bits(got[k], whole[k][b:b + 1]), (b, k)
    ws.close()
    alone = _measure(pkg, c)                                                # a workspace made for the call
    assert all(TH.same_bits(alone[k], whole[k]) for k in whole)
    a, kw = TH.args(c)
    with pytest.raises(ValueError):
        pkg.contact_textures(*a, **dict(kw, max_lag=32))
    with pytest.raises(ValueError):
        pkg.contact_textures(*a, **dict(kw, form_degree=3))
    with pytest.raises(ValueError):
        pkg.contact_textures(a[0], a[1], a[2][:, :, :8], *a[3:], **kw)


@pytest.mark.gpu
def test_native_size_strip_and_disc(pkg):
    c, ref, ne = _native()
    got = _measure(pkg, c)
    TH.hold_device(c, got, ref, ne)
    TH.hold_end_to_end(c, got, ref)
    t = got["textures"][0]
    assert t[0, T["eval_pixels"]] > 30000 and t[1, T["eval_pixels"]] == 3300 and list(t[:2, T["form_status"]]) == [TH.OK, TH.OK]
    assert t[1, T["lobe_status"]] == 1 and t[1, T["acf_valid_lags"]] == 5 * 33                              # three rows: dy = -2..2 only
    assert np.isnan(t[2:]).all()


# ---------------------------------------------------------------------------------------------------------------- GPU, through the session
def _session(pkg, n, max_batch):
    model, neg = pkg.load_calibration(os.path.join(G, "calibration_phase_to_height.json"))
    fm = pkg.load_force_calibration(os.path.join(G, "calibration_height_to_force.json"))["best_model"]
    return pkg.FtpSensor(pkg.synth.reference_frame(n), pkg.synth.roi_circle(n), pkg.FtpConfig.scaled(n), model, neg, fm, max_batch=max_batch)


@pytest.mark.gpu
def test_session_textures_are_held_on_the_gpu_planes_and_leave_predict_alone(pkg):
    import torch
    n, nb, K = 224, 4, 8
    frames = CH.multi_contact_batch(pkg, n, 0, nb)
    s, plain = _session(pkg, n, nb), _session(pkg, n, nb)
    with pytest.raises(RuntimeError):
        s.textures()                                       # no predict yet
    o = s.predict_batch(frames)
    before = {k: v.clone() for k, v in o.items()}
    r = s.textures(K)
    first = s._textures
    assert s.textures(K)["textures"].shape == r["textures"].shape and s._textures is first                # reused
    assert tuple(s.textures(K, max_lag=4)["acf"].shape) == (nb, K, 9, 9) and s._textures is not first      # rebuilt for another window
    with pytest.raises(TypeError):
        s.textures(K, lag=4)
    torch.cuda.synchronize()
    assert set(r) == {"contacts", "count", "contact_index", "textures", "residual", "acf"}
    assert tuple(r["textures"].shape) == (nb, K, 40) and tuple(r["residual"].shape) == (nb, n, n) and tuple(r["acf"].shape) == (nb, K, 17, 17)
    want = plain.predict_batch(frames)
    torch.cuda.synchronize()
    for k in before:                                       # predict's outputs: bit-equal with and without the read-out
        assert torch.equal(o[k].contiguous().view(torch.uint8), before[k].contiguous().view(torch.uint8)), k
        assert torch.equal(o[k].contiguous().view(torch.uint8), want[k].contiguous().view(torch.uint8)), k
    c = {"depth": o["height_map_mm"].cpu().numpy(), "index": r["contact_index"].cpu().numpy(), "tab": r["contacts"].cpu().numpy(),
         "count": r["count"].cpu().numpy(), "mpp": o["scalars"][:, 6].cpu().numpy(), "eps": s.config.depth_eps_mm, "frac": 0.5, "K": K,
         "degree": 2, "L": 8, "thr": 0.2, "peak_min": 0.3}
    got = {k: r[k].cpu().numpy() for k in ("textures", "residual", "acf")}
    s.close()
    plain.close()
    assert s._textures is None
    TH.hold_device(c, got, TH.numpy_textures(c), TH.numpy_textures_ne(c, forms_only=True))
    used = ~np.isnan(got["textures"][..., 0])
    assert used.sum() == np.minimum(c["count"], K).sum() >= nb
    assert (got["textures"][..., T["form_status"]][used] == TH.OK).any()


@pytest.mark.gpu
def test_predict_textures_argument(pkg):
    n = 224
    s = _session(pkg, n, 1)
    frame = CH.multi_contact_frame(pkg, n, 2)
    with_contacts = s.predict(frame, contacts=4)
    res = s.predict(frame, contacts=4, textures=dict(max_lag=6, form_degree=1))
    assert set(res) == set(with_contacts) | {"textures"} and "textures" not in with_contacts
    assert len(res["textures"]) == len(res["contacts"]) >= 1
    for tx, ct in zip(res["textures"], res["contacts"]):
        assert list(tx)[0] == "contact" and list(tx)[1:] == list(pkg.TEXTURE_NAMES)
        assert isinstance(tx["form_status"], int) and 0 <= tx["eval_pixels"] <= ct["contact_pixels"]
        if tx["form_status"] == 0:
            assert tx["form_c3"] == tx["form_c4"] == tx["form_c5"] == 0.0 and tx["sq_mm"] > 0.0
    assert len(s.predict(frame, contacts=4, textures={})["textures"]) == len(res["contacts"])
    with pytest.raises(ValueError):
        s.predict(frame, textures={})
    s.close()
