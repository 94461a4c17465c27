"""Indenter match read-out (include_ext/vistaf_match.h, TemplateBank, contact_matches, FtpSensor.matches): which known object touches, where, how turned.

The definition is restated in tests/match_helpers.py: `ref_bank` (plain Python floats; the library's host bank must equal it bit for bit) and
`numpy_matches` (patch bit for bit, sums in np.longdouble, every float field within a rounding bound written out there from the reference's own
sums, none of them measured off the device).  The inputs are three analytic indenters (ball, ridge, T) evaluated analytically in the rotated
frame: 24 cases (two banks x two scales x three shapes x two angles).  On every one of them the winner leads every other (template, rotation,
shift) by at least 2.2e-2 against a bound near 1e-13, which is asserted on the reference before any device comparison, so every integer field
is held exactly."""
import csv
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest

import contacts_helpers as CH
import match_helpers as MH
from abi_helpers import _hold_against, _prototypes, _same_bits
from match_helpers import F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
HEADER = os.path.join(ROOT, "include_ext", "vistaf_match.h")
E_INVALID = -1
SYM = [s for _, _, s in MH.SHAPES]
_BANKS, _FRAMES, _REFS = {}, {}, {}


def _bank(pkg, name):
    """the banks of the tests, built once (host only)"""
    if name not in _BANKS:
        if name in ("small", "large"):
            cfg = MH.SMALL if name == "small" else MH.LARGE
            _BANKS[name] = pkg.TemplateBank(MH.templates(cfg["P"], cfg["pitch"]), [0, 1, 2], SYM, cfg["pitch"], rotations=cfg["R"])
        elif name == "m16":           # M exactly 16: two templates without symmetry over R = 8
            tp = np.stack([MH.template_of(MH.tee, 9, 0.1), MH.template_of(_wedge, 9, 0.1)])
            _BANKS[name] = pkg.TemplateBank(tp, [4, 9], [1, 1], 0.1, rotations=8)
        elif name == "m1":            # M = 1: the ball alone
            _BANKS[name] = pkg.TemplateBank(MH.template_of(MH.ball, 9, 0.1)[None], [7], [0], 0.1, rotations=12)
        elif name == "twins":         # the same template twice under two classes
            tp = np.stack([MH.template_of(MH.ball, 9, 0.1)] * 2)
            _BANKS[name] = pkg.TemplateBank(tp, [3, 5], [0, 0], 0.1, rotations=12)
    return _BANKS[name]


def _wedge(u, v):
    return np.where((np.abs(u) <= 0.4) & (np.abs(v) <= 0.2), 0.5 * (u + 0.4) / 0.8, 0.0)


def _frames(name):
    if name not in _FRAMES:
        _FRAMES[name] = MH.frames24(MH.SMALL if name == "small" else MH.LARGE)
    return _FRAMES[name]


def _reference(pkg, name):
    """the reference of one bank's 12 frames, computed once and left unchanged"""
    if name not in _REFS:
        fr, cfg = _frames(name), MH.SMALL if name == "small" else MH.LARGE
        _REFS[name] = MH.numpy_matches(fr["depth"], fr["index"], fr["contacts"], fr["count"], fr["mm_per_px"], _bank(pkg, name), max_shift=cfg["m"])
    return _REFS[name]


def _assert_gap(ref):
    """no case may be skipped for failing this: the winner's lead over every other (t, r, s) exceeds twice the rounding bound"""
    for rows in ref["rows"]:
        for row in rows:
            if row is not None and row.rec[0] == MH.OK:
                assert row.gap > 2.0 * row.bound, (row.gap, row.bound)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_match_names_and_signatures_follow_the_header(pkg):
    hdr = open(HEADER).read()
    idx = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define VISTAF_MATCH_(\w+)\s+(\w+)\b", hdr) if m.group(2).isdigit()}
    consts = {k: idx.pop(k) for k in ("header_ints", "min_p", "max_p", "max_r", "max_t", "max_symmetry", "max_shift", "max_rows")}
    L = pkg._lib
    assert consts == {"header_ints": L.MATCH_HEADER_INTS, "min_p": L.MATCH_MIN_P, "max_p": L.MATCH_MAX_P, "max_r": L.MATCH_MAX_R, "max_t": L.MATCH_MAX_T,
                      "max_symmetry": L.MATCH_MAX_SYMMETRY, "max_shift": L.MATCH_MAX_SHIFT, "max_rows": L.MATCH_MAX_ROWS}
    assert consts == {"header_ints": 16, "min_p": 5, "max_p": 33, "max_r": 64, "max_t": 64, "max_symmetry": 8, "max_shift": 8, "max_rows": 2048}
    assert int(re.search(r"#define VISTAF_MATCH_MAGIC\s+(0x[0-9a-f]+)", hdr).group(1), 16) == L.MATCH_MAGIC
    assert sorted(idx.values()) == list(range(23))
    for name, i in idx.items():
        assert pkg.MATCH_NAMES[i] == name
    assert list(pkg.MATCH_NAMES) == list(L.MATCH_NAMES) == list(pkg.writers.MATCH_FIELDS) == list(MH.FIELDS)
    assert int(re.search(r"#define VISTAF_NMATCH\s+(\d+)", hdr).group(1)) == L.NMATCH == MH.NMATCH == 24
    status = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define VISTAF_MATCHST_(\w+)\s+(\d+)\b", hdr)}
    assert status == L.MATCH_STATUS == pkg.match.MATCH_STATUS == {"ok": MH.OK, "no_pixels": MH.NO_PIXELS, "no_scale": MH.NO_SCALE, "no_support": MH.NO_SUPPORT}
    flags = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define VISTAF_MATCHFL_(\w+)\s+(\d+)\b", hdr)}
    assert flags == L.MATCH_FLAGS == {"clipped": MH.CLIPPED, "border_shift": MH.BORDER_SHIFT, "weak": MH.WEAK, "ambiguous": MH.AMBIGUOUS}
    assert set(pkg.writers.MATCH_INT_FIELDS) == set(MH.INT_FIELDS)
    for name in ("match", "MATCH_NAMES", "TemplateBank", "MatchWorkspace", "contact_matches", "matches_table", "write_matches_csv", "match_frame_record"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    # the header is outside include/*.h, whose prototype count tests/test_abi_surface.py pins; the rule of that test, for these functions
    protos = _prototypes(hdr)
    table = L.MATCH_SIGNATURES
    assert sorted(protos) == sorted(table) == ["vistaf_match_bank_bytes", "vistaf_match_build_bank", "vistaf_match_measure", "vistaf_match_workspace_bytes"]
    assert not set(table) & ({n for g in L.SIGNATURES.values() for n in g} | set(L.OUTLINE_SIGNATURES) | set(L.TEXTURE_SIGNATURES))
    _hold_against(protos, table, L.load())
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other.endswith(".h"):
            assert "vistaf_match" not in open(os.path.join(ROOT, "include", other)).read(), other


@pytest.mark.parametrize("name", ["small", "large"])
def test_bank_equals_the_plain_loop_restatement_bit_for_bit(pkg, name):
    cfg = MH.SMALL if name == "small" else MH.LARGE
    bank, tps = _bank(pkg, name), MH.templates(cfg["P"], cfg["pitch"])
    assert (bank.T, bank.P, bank.R) == (3, cfg["P"], cfg["R"])
    assert (bank.M, bank.D, bank.Dp) == ((19, 49, 52) if name == "small" else (37, 197, 200))
    assert list(bank.header[:7]) == [pkg._lib.MATCH_MAGIC, 3, bank.P, bank.R, bank.M, bank.D, bank.Dp] and not bank.header[10:].any()
    assert bank.header[8:10].view(np.float64)[0] == cfg["pitch"] == bank.template_mm_per_px
    for r in range(bank.R):                                                    # within one unit in the last place of 1
        th = (2.0 * math.pi * r) / bank.R
        assert abs(bank.cossin[r, 0] - math.cos(th)) <= 2.0 ** -52 and abs(bank.cossin[r, 1] - math.sin(th)) <= 2.0 ** -52
    want = MH.ref_bank(tps.tolist(), SYM, bank.R, bank.cossin.tolist())        # fed the bank's own table
    assert (want["M"], want["D"], want["Dp"]) == (bank.M, bank.D, bank.Dp)
    for field in ("rowtab", "disc", "mu", "norm", "rows"):
        got = getattr(bank, field)
        assert got.shape == want[field].shape and got.dtype == want[field].dtype, field
        assert np.array_equal(got.view(np.uint8), want[field].view(np.uint8)), field
    assert list(bank.klass) == [0, 1, 2] and list(bank.symmetry) == SYM
    assert not bank.rows[:, bank.D:].any()                                     # the padding of every row
    # the layout: the sections end where the library's size says
    assert bank.nbytes == bank.offsets["end"] == MH.layout_bytes(bank.T, bank.P, bank.R, bank.M, bank.D) == pkg.match.bank_bytes(3, bank.P, bank.R, SYM)
    assert bank.offsets["rows"] % 256 == 0 and bank.host.ctypes.data % 8 == 0
    rows = bank.rows[:, :bank.D]
    assert np.abs(rows.sum(axis=1)).max() < 1e-13 and np.abs((rows * rows).sum(axis=1) - 1.0).max() < 1e-13


def test_match_c_abi_refuses_with_the_arguments_name(pkg):
    lib = pkg._lib.load()
    err = lib.vistaf_ftp_last_error
    n = ctypes.c_size_t(1)
    i32p = ctypes.POINTER(ctypes.c_int32)
    sym = (ctypes.c_int32 * 3)(0, 2, 1)
    assert lib.vistaf_match_bank_bytes(3, 9, 12, sym, None) == E_INVALID and b"bytes" in err()
    assert lib.vistaf_match_bank_bytes(3, 9, 12, None, ctypes.byref(n)) == E_INVALID and b"symmetry" in err()
    for a, s, word in (((0, 9, 12), (0, 2, 1), b"T "), ((65, 9, 12), (0, 2, 1), b"T "), ((3, 8, 12), (0, 2, 1), b"P "), ((3, 3, 12), (0, 2, 1), b"P "),
                       ((3, 35, 12), (0, 2, 1), b"P "), ((3, 9, 0), (0, 2, 1), b"R "), ((3, 9, 65), (0, 2, 1), b"R "), ((3, 9, 12), (0, 5, 1), b"R % symmetry"),
                       ((3, 9, 12), (0, 9, 1), b"symmetry"), ((3, 9, 12), (-1, 2, 1), b"symmetry")):
        n.value = 1
        assert lib.vistaf_match_bank_bytes(*a, (ctypes.c_int32 * 3)(*s), ctypes.byref(n)) == E_INVALID and n.value == 0 and word in err(), (a, s, err())
    many = (ctypes.c_int32 * 64)(*([1] * 64))
    assert lib.vistaf_match_bank_bytes(64, 9, 64, many, ctypes.byref(n)) == E_INVALID and b"M" in err() and b"2048" in err()      # 64 * 64 rows
    assert lib.vistaf_match_bank_bytes(3, 9, 12, sym, ctypes.byref(n)) == 0 and n.value == MH.layout_bytes(3, 9, 12, 19, 49)
    with pytest.raises(ValueError, match="P must be odd"):
        pkg.match.bank_bytes(3, 10, 12, [0, 2, 1])
    # build: NULLs, sizes, a short bank, a flat template by its index
    tp = MH.templates(9, 0.1)
    buf = (ctypes.c_double * (n.value // 8 + 1))()
    fp = tp.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    kl = (ctypes.c_int32 * 3)(0, 1, 2)
    build = lib.vistaf_match_build_bank
    assert build(None, kl, sym, 3, 9, 12, 0.1, buf, n.value) == E_INVALID and b"templates" in err()
    assert build(fp, None, sym, 3, 9, 12, 0.1, buf, n.value) == E_INVALID and b"klass" in err()
    assert build(fp, kl, None, 3, 9, 12, 0.1, buf, n.value) == E_INVALID and b"symmetry" in err()
    assert build(fp, kl, sym, 3, 9, 12, 0.1, None, n.value) == E_INVALID and b"h_bank" in err()
    assert build(fp, kl, sym, 3, 10, 12, 0.1, buf, n.value) == E_INVALID and b"P " in err()
    assert build(fp, kl, (ctypes.c_int32 * 3)(0, 5, 1), 3, 9, 12, 0.1, buf, n.value) == E_INVALID and b"R % symmetry" in err()
    assert build(fp, (ctypes.c_int32 * 3)(0, -2, 2), sym, 3, 9, 12, 0.1, buf, n.value) == E_INVALID and b"klass[1]" in err()
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        assert build(fp, kl, sym, 3, 9, 12, bad, buf, n.value) == E_INVALID and b"template_mm_per_px" in err()
    assert build(fp, kl, sym, 3, 9, 12, 0.1, buf, n.value - 8) == E_INVALID and b"bank_bytes" in err()
    assert build(fp, kl, sym, 3, 9, 12, 0.1, ctypes.addressof(buf) + 4, n.value) == E_INVALID and b"h_bank" in err() and b"aligned" in err()
    flat = tp.copy()
    flat[1] = 0.25
    assert build(flat.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), kl, sym, 3, 9, 12, 0.1, buf, n.value) == E_INVALID and b"templates[1]" in err() and b"flat" in err()
    flat[1] = tp[1]
    flat[2, 4, 4] = np.inf
    assert build(flat.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), kl, sym, 3, 9, 12, 0.1, buf, n.value) == E_INVALID and b"templates[2]" in err()
    assert build(fp, kl, sym, 3, 9, 12, 0.1, buf, n.value) == 0
    with pytest.raises(ValueError, match=r"templates\[0\]"):
        pkg.TemplateBank(np.zeros((1, 9, 9), np.float32), [0], [0], 0.1)
    with pytest.raises(ValueError):
        pkg.TemplateBank(tp, [0, 1], SYM, 0.1)
    # workspace
    w = ctypes.c_size_t(1)
    assert lib.vistaf_match_workspace_bytes(40, 48, 1, 2, 9, 2, 19, None) == E_INVALID and b"bytes" in err()
    for a, word in (((0, 48, 1, 2, 9, 2, 19), b"h "), ((40, 0, 1, 2, 9, 2, 19), b"w "), ((65536, 65536, 1, 2, 9, 2, 19), b"h * w"), ((40, 48, 0, 2, 9, 2, 19), b"max_batch"),
                    ((40, 48, 1, 0, 9, 2, 19), b"max_contacts"), ((40, 48, 1, 65, 9, 2, 19), b"max_contacts"), ((40, 48, 1, 2, 8, 2, 19), b"P "),
                    ((40, 48, 1, 2, 9, -1, 19), b"max_shift"), ((40, 48, 1, 2, 9, 9, 19), b"max_shift"), ((40, 48, 1, 2, 9, 2, 0), b"M "), ((40, 48, 1, 2, 9, 2, 2049), b"M ")):
        w.value = 1
        assert lib.vistaf_match_workspace_bytes(*a, ctypes.byref(w)) == E_INVALID and w.value == 0 and word in err(), a
    assert lib.vistaf_match_workspace_bytes(40, 48, 2, 2, 9, 2, 19, ctypes.byref(w)) == 0
    assert w.value >= 2 * 2 * (25 * 20 + 19 * 20) and pkg.match.workspace_bytes(40, 48, 2, 2, 9, 2, 19) == w.value
    two = w.value
    assert lib.vistaf_match_workspace_bytes(40, 48, 1, 2, 9, 2, 19, ctypes.byref(w)) == 0 and w.value <= two
    # measure: host memory stands in for the device's, every call is refused before any HIP call
    f64, f32, i32, i8 = (ctypes.c_double * 4096)(), (ctypes.c_float * 4096)(), (ctypes.c_int32 * 64)(), (ctypes.c_int8 * 4096)()
    raw = (ctypes.c_uint8 * (w.value + 512))()
    ws = (ctypes.addressof(raw) + 255) & ~255
    p = ctypes.addressof
    hdr = ctypes.cast(buf, i32p)
    good = dict(dep=p(f32), idx=p(i8), tab=p(f64), cnt=p(i32), mpp=p(f64), bank=p(buf), nb=n.value, hdr=hdr, eps=0.01, m=2, minpix=6, acs=0.7, acm=0.05,
                h=40, w=48, B=1, K=2, out=p(f64), sc=p(f64), pat=p(f32), ws=ws, n=w.value)

    def call(**kw):
        a = dict(good, **kw)
        return lib.vistaf_match_measure(a["dep"], a["idx"], a["tab"], a["cnt"], a["mpp"], a["bank"], a["nb"], a["hdr"], a["eps"], a["m"], a["minpix"], a["acs"],
                                        a["acm"], a["h"], a["w"], a["B"], a["K"], a["out"], a["sc"], a["pat"], a["ws"], a["n"], None)
    nan, inf = float("nan"), float("inf")
    wrong = (ctypes.c_int32 * 16)(*list(hdr[:16]))
    wrong[0] = 7
    sizes = (ctypes.c_int32 * 16)(*list(hdr[:16]))
    sizes[5] = 50
    other = (ctypes.c_int32 * 16)(*list(hdr[:16]))
    other[4] = 20                                                          # a plausible header of another bank: its size is not bank_bytes
    for kw, words in ((dict(dep=None), [b"d_depth_mm"]), (dict(idx=None), [b"d_contact_index"]), (dict(tab=None), [b"d_contacts"]), (dict(cnt=None), [b"d_count"]),
                      (dict(mpp=None), [b"d_mm_per_px"]), (dict(bank=None), [b"d_bank"]), (dict(hdr=None), [b"h_bank_header"]), (dict(out=None), [b"d_matches"]),
                      (dict(sc=None), [b"d_scores"]), (dict(pat=None), [b"d_patches"]), (dict(ws=None), [b"d_workspace"]), (dict(hdr=wrong), [b"h_bank_header"]),
                      (dict(hdr=sizes), [b"h_bank_header"]), (dict(hdr=other), [b"bank_bytes"]), (dict(nb=n.value - 8), [b"bank_bytes"]), (dict(nb=0), [b"bank_bytes"]),
                      (dict(h=0), [b"h "]), (dict(w=-1), [b"w "]), (dict(h=65536, w=65536), [b"h * w"]), (dict(B=0), [b"batch"]), (dict(K=0), [b"max_contacts"]),
                      (dict(K=65), [b"max_contacts"]), (dict(m=-1), [b"max_shift"]), (dict(m=9), [b"max_shift"]), (dict(eps=nan), [b"depth_eps_mm"]),
                      (dict(eps=inf), [b"depth_eps_mm"]), (dict(minpix=0), [b"min_pixels"]), (dict(acs=nan), [b"accept_score"]), (dict(acs=inf), [b"accept_score"]),
                      (dict(acm=nan), [b"accept_margin"]), (dict(tab=p(f64) + 4), [b"d_contacts", b"aligned"]), (dict(bank=p(buf) + 4), [b"d_bank", b"aligned"]),
                      (dict(pat=p(f32) + 2), [b"d_patches", b"aligned"]), (dict(ws=ws + 128), [b"d_workspace", b"aligned"]), (dict(n=w.value - 1), [b"workspace_bytes"]),
                      (dict(n=0), [b"workspace_bytes"]), (dict(B=2), [b"workspace_bytes"]), (dict(m=3), [b"workspace_bytes"])):
        assert call(**kw) == E_INVALID, kw
        assert all(word in err() for word in words), (kw, err())


@pytest.mark.parametrize("name", ["small", "large"])
def test_restatement_meets_the_analytic_truth_on_the_24_cases(pkg, name):
    fr, ref, bank = _frames(name), _reference(pkg, name), _bank(pkg, name)
    _assert_gap(ref)
    rows = [ref["rows"][b][0] for b in range(12)]
    assert min(r.gap for r in rows) >= 2.2e-2 and max(r.bound for r in rows) < 2e-12
    assert np.isnan(ref["matches"][:, 1]).all() and np.isnan(ref["patches"][:, 1]).all()          # count == 1: row 1 is not in use
    for b, (t, ang, (x, y)) in enumerate(fr["truth"]):
        rec = ref["matches"][b, 0]
        assert rec[F["status"]] == MH.OK and rec[F["template"]] == t and rec[F["class"]] == rec[F["label"]] == t and rec[F["flags"]] == 0
        if SYM[t]:
            per = 2.0 * math.pi / SYM[t]
            d = abs(rec[F["angle_rad"]] - ang % per)
            assert min(d, per - d) <= math.pi / bank.R, (b, rec[F["angle_rad"]], ang)
        else:
            assert rec[F["angle_rad"]] == 0.0 and rec[F["rotation"]] == 0 and rec[F["rot_contrast"]] == 0.0
        rho = bank.template_mm_per_px / fr["mm_per_px"][b]
        assert abs(rec[F["x_px"]] - x) <= rho and abs(rec[F["y_px"]] - y) <= rho                    # one template pixel
        assert 0.45 < rec[F["scale"]] < 0.65 and rec[F["score"]] > 0.8 and rec[F["margin"]] > 0.1 and rec[F["second_class"]] != t


def _hand_table():
    t = np.full((2, 3, 24), np.nan)
    t[0, 0, :23] = [0, 2, 1, 1, 1, 4, 2, -1, 0.93, 1.0552, 22.28, 17.67, 0.1, -0.05, 2, 0.71, 0.22, 0.31, 0.489, 0.017, 0.0396, 141, 49]
    t[0, 1, 0] = 1
    t[1, 0, 0], t[1, 0, 22] = 3, 0
    return t, np.array([2, 1], np.int32)


def test_match_writers_round_trip(pkg, tmp_path):
    t, n = _hand_table()
    rows = pkg.matches_table(t, n)
    assert [(r["frame"], r["contact"]) for r in rows] == [(0, 0), (0, 1), (1, 0)]
    assert list(rows[0])[2:] == list(pkg.MATCH_NAMES)
    for r in rows:
        assert all(isinstance(r[k], int) for k in MH.INT_FIELDS) and all(isinstance(r[k], float) for k in MH.FIELDS if k not in MH.INT_FIELDS)
    assert rows[0]["template"] == 1 and rows[0]["shift_y"] == -1 and rows[0]["score"] == 0.93 and rows[0]["support_pixels"] == 141
    assert rows[1]["status"] == 1 and rows[1]["label"] == -1 and rows[1]["valid_shifts"] == -1 and np.isnan(rows[1]["score"])
    assert rows[2]["status"] == 3 and rows[2]["valid_shifts"] == 0
    with pytest.raises(ValueError):
        pkg.matches_table(t[..., :20], n)
    path = pkg.write_matches_csv(str(tmp_path), t, n)
    back = list(csv.DictReader(open(path, newline="")))
    assert len(back) == 3 and list(back[0]) == ["frame", "contact"] + list(pkg.MATCH_NAMES)
    for r, q in zip(rows, back):
        for name in pkg.MATCH_NAMES:
            v = float(q[name])
            assert v == r[name] or (np.isnan(v) and np.isnan(r[name])), name
    sc = np.full((3, 2), np.nan)
    sc[0] = [0.71, 0.93]
    rec = pkg.match_frame_record(t[0], 2, sc)
    assert rec["contact_count"] == 2 and [r["contact"] for r in rec["matches"]] == [0, 1] and "frame" not in rec["matches"][0]
    assert rec["matches"][1]["score"] is None and rec["matches"][0]["margin"] == 0.22
    assert rec["scores"] == [[0.71, 0.93], [None, None]]
    assert json.loads(json.dumps(rec)) == rec                             # nothing in it that JSON cannot hold
    assert "scores" not in pkg.match_frame_record(t[0], 2)
    with pytest.raises(ValueError):
        pkg.match_frame_record(t[0], 2, sc[:2])


def test_contact_matches_needs_a_device_and_predict_needs_contacts(pkg):
    import torch
    fr, bank = _frames("small"), _bank(pkg, "small")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):
            pkg.contact_matches(fr["depth"], fr["index"], fr["contacts"], fr["count"], fr["mm_per_px"], MH.EPS, bank)
    with pytest.raises(ValueError, match="max_shift"):
        pkg.MatchWorkspace(40, 48, 1, 2, 9, 9, 19, device="cpu")
    blank = object.__new__(pkg.FtpSensor)                                  # the check comes before anything of the session is touched
    with pytest.raises(ValueError, match="contacts=K"):
        pkg.FtpSensor.predict(blank, None, matches=dict(bank=bank))
    with pytest.raises(ValueError, match="bank"):
        pkg.FtpSensor.predict(blank, None, contacts=2, matches=dict(max_shift=2))


# ---------------------------------------------------------------------------------------------------------------- GPU
def _measure(pkg, fr, bank, ws=None, eps=MH.EPS, **kw):
    import torch
    out = pkg.contact_matches(fr["depth"], fr["index"], fr["contacts"], fr["count"], fr["mm_per_px"], eps, bank, ws, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _ref(fr, bank, **kw):
    return MH.numpy_matches(fr["depth"], fr["index"], fr["contacts"], fr["count"], fr["mm_per_px"], bank, **kw)


def _pick(fr, sel):
    return {k: (v[sel] if isinstance(v, np.ndarray) else [v[i] for i in sel]) for k, v in fr.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["small", "large"])
def test_the_24_cases_on_the_device(pkg, name):
    """small: M = 19, D = 49, 25 shifts -- all three tile tails at once; large: M = 37, D = 197, 49 shifts"""
    cfg = MH.SMALL if name == "small" else MH.LARGE
    fr, ref = _frames(name), _reference(pkg, name)
    _assert_gap(ref)
    got = _measure(pkg, fr, _bank(pkg, name), max_shift=cfg["m"])
    assert got["matches"].shape == (12, 2, 24) and got["scores"].shape == (12, 2, 3) and got["patches"].shape == (12, 2) + (cfg["P"] + 2 * cfg["m"],) * 2
    MH.hold_device(got, ref)
    assert list(got["matches"][:, 0, F["template"]]) == [t for t, _, _ in fr["truth"]]


@pytest.mark.gpu
def test_tiles_m16_m1_and_a_single_shift(pkg):
    fr = _pick(_frames("small"), [4, 0, 2])                                # the T at 60 degrees, the ball, the ridge; rho = 1
    b16, b1 = _bank(pkg, "m16"), _bank(pkg, "m1")
    assert b16.M == 16 and b1.M == 1
    ref = _ref(fr, b16, max_shift=2)
    _assert_gap(ref)
    got = _measure(pkg, fr, b16, max_shift=2)
    MH.hold_device(got, ref)
    assert got["matches"][0, 0, F["class"]] == 4
    ref = _ref(fr, b1, max_shift=2)
    _assert_gap(ref)
    got = _measure(pkg, fr, b1, max_shift=2)
    MH.hold_device(got, ref)
    m = got["matches"][:, 0]
    assert (m[:, F["template"]] == 0).all() and (m[:, F["second_class"]] == -1).all() and np.isnan(m[:, F["margin"]]).all()
    assert (m[:, F["label"]][m[:, F["score"]] >= 0.7] == 7).all() and m[1, F["label"]] == 7
    # m = 0: one shift, no BORDER_SHIFT, no refinement of the position
    small = _bank(pkg, "small")
    ref = _ref(fr, small, max_shift=0)
    _assert_gap(ref)
    got = _measure(pkg, fr, small, max_shift=0)
    MH.hold_device(got, ref)
    m = got["matches"][:, 0]
    assert got["patches"].shape[2:] == (9, 9) and (m[:, F["valid_shifts"]] == 1).all() and not (m[:, F["flags"]].astype(int) & MH.BORDER_SHIFT).any()
    assert (m[:, F["shift_x"]] == 0).all() and (m[:, F["offset_x_mm"]] == 0).all() and (m[:, F["offset_y_mm"]] == 0).all()
    assert np.array_equal(m[:, F["x_px"]], fr["contacts"][:, 0, MH.C_CX]) and np.array_equal(m[:, F["y_px"]], fr["contacts"][:, 0, MH.C_CY])


@pytest.mark.gpu
@pytest.mark.parametrize("m", [4, 5, 6, 7, 8])
def test_every_count_of_shift_tiles_per_wave(pkg, m):
    """k_match_score is instantiated per number of 16-shift tiles a wave owns: 1 up to m = 3 (the cases above), then 2 (m = 4: three waves;
    m = 5: four), 3, 4 and 5 (m = 8, 289 shifts in 19 tiles, the last wave's last tile empty)"""
    fr, bank = _pick(_frames("small"), [4, 0, 2]), _bank(pkg, "small")
    ref = _ref(fr, bank, max_shift=m)
    _assert_gap(ref)
    got = _measure(pkg, fr, bank, max_shift=m)
    MH.hold_device(got, ref)
    assert got["patches"].shape[2:] == (9 + 2 * m,) * 2 and (got["matches"][:, 0, F["valid_shifts"]] > 25).all()
    assert list(got["matches"][:, 0, F["template"]]) == [2, 0, 1] and not (got["matches"][:, 0, F["flags"]].astype(int) & MH.BORDER_SHIFT).any()


@pytest.mark.gpu
def test_a_negative_eps_counts_the_disc_and_not_the_padding(pkg):
    """D = 49 of the small bank is padded to Dp = 52 and D = 197 of the large one to 200; the zero operands of the padding are no samples"""
    for name, m in (("small", 2), ("large", 3)):
        fr, bank = _pick(_frames(name), [0, 2]), _bank(pkg, name)
        ref = _ref(fr, bank, eps=-1.0, max_shift=m)
        _assert_gap(ref)
        got = _measure(pkg, fr, bank, eps=-1.0, max_shift=m)
        MH.hold_device(got, ref)
        assert (got["matches"][:, 0, F["support_pixels"]] == bank.D).all() and (got["matches"][:, 0, F["valid_shifts"]] == (2 * m + 1) ** 2).all()


def _edge_frames():
    """eight frames of 40 x 48 with K = 3 (see test_table_edges)"""
    K, s = 3, 0.1
    depth, index, tabs, cnt, mpp = [], [], [], [], []

    def add(d, ix, count=None, scale=s, edit=None):
        tab, n = MH.table_of(d, ix, K)
        if edit:
            edit(tab)
        depth.append(d); index.append(ix); tabs.append(tab); cnt.append(n if count is None else count); mpp.append(scale)
    ball = MH.contact_depth(MH.ball, 0.0, s)
    one = np.where(ball > 0, 0, -1).astype(np.int8)
    add(ball, one, count=0)                                                # 0: count == 0
    two = MH.contact_depth(MH.ball, 0.0, s, centre=(35.4, 28.7)) + ball    # 1: count > K; row 1 has a NaN centroid, row 2 is two pixels
    ix = np.where(ball > 0, 0, -1).astype(np.int8)
    ix[two > ball] = 1
    two[3, 40] = two[3, 41] = np.float32(0.5)
    ix[3, 40] = ix[3, 41] = 2

    def nan_centroid(tab):
        tab[1, MH.C_CX] = np.nan
    add(two, ix, count=7, edit=nan_centroid)
    corner = MH.contact_depth(MH.ball, 0.0, s, centre=(1.4, 0.8))          # 2: a contact in the frame corner
    add(corner, np.where(corner > 0, 0, -1).astype(np.int8))
    ix = one.copy()                                                        # 3: one ball cut in two contacts that touch
    ix[(ball > 0) & (np.arange(MH.W)[None, :] > 22)] = 1
    add(ball, ix)
    bad = ball.copy()                                                      # 4: a NaN and an Inf depth inside the contact
    bad[17, 22], bad[18, 24], bad[16, 21] = np.nan, np.inf, -np.inf
    add(bad, one)
    add(ball, one, scale=np.nan)                                           # 5: no scale
    add(ball, one, scale=0.0)                                              # 6: no scale either
    tiny = np.zeros_like(ball)                                             # 7: a two-pixel contact under min_pixels = 6
    tiny[20, 30] = tiny[20, 31] = np.float32(0.5)
    add(tiny, np.where(tiny > 0, 0, -1).astype(np.int8))
    return dict(depth=np.stack(depth), index=np.stack(index), contacts=np.stack(tabs), count=np.array(cnt, np.int32), mm_per_px=np.array(mpp))


@pytest.mark.gpu
def test_table_edges(pkg):
    fr, bank = _edge_frames(), _bank(pkg, "small")
    ref = _ref(fr, bank, max_shift=2, min_pixels=6)
    got = _measure(pkg, fr, bank, max_shift=2, min_pixels=6)
    MH.hold_device(got, ref)
    m, st, fl = got["matches"], got["matches"][..., F["status"]], got["matches"][..., F["flags"]]
    assert np.isnan(m[0]).all() and np.isnan(got["patches"][0]).all() and np.isnan(got["scores"][0]).all()               # count == 0
    assert list(st[1]) == [MH.OK, MH.NO_PIXELS, MH.NO_SUPPORT]                                                             # count = 7 > K = 3
    assert np.isnan(m[1, 1, 1:]).all() and np.isnan(got["patches"][1, 1]).all() and np.isnan(got["scores"][1, 1]).all()
    assert m[1, 2, F["valid_shifts"]] == 0 and np.isnan(np.delete(m[1, 2], [F["status"], F["valid_shifts"]])).all() and not np.isnan(got["patches"][1, 2]).any()
    assert st[2, 0] == MH.OK and int(fl[2, 0]) & MH.CLIPPED and (got["patches"][2, 0][:3, :3] == 0).all()               # outside counts as 0
    assert not int(fl[1, 0]) & MH.CLIPPED
    assert list(st[3, :2]) == [MH.OK, MH.OK]                                                                               # isolation: the neighbour's depth is not there
    assert (got["patches"][3, 0][:, 10:] == 0).all() and got["patches"][3, 0][:, :7].max() > 0.2                         # x > 22 belongs to row 1
    assert (got["patches"][3, 1][:, :3] == 0).all() and got["patches"][3, 1][:, 6:].max() > 0.2
    assert st[4, 0] == MH.OK and np.isfinite(got["patches"][4, 0]).all() and np.isfinite(m[4, 0, :23]).all()               # NaN, Inf count as 0
    assert st[5, 0] == st[6, 0] == MH.NO_SCALE and np.isnan(m[5, 0, 1:]).all() and np.isnan(m[5, 1:]).all() and np.isnan(got["patches"][5]).all()
    assert st[7, 0] == MH.NO_SUPPORT and m[7, 0, F["valid_shifts"]] == 0 and np.isnan(got["scores"][7, 0]).all()
    assert got["patches"][7, 0].max() > 0                                                                                  # the patch of a NO_SUPPORT row is written


@pytest.mark.gpu
def test_decision_ambiguous_twins_and_a_weak_match(pkg):
    fr = _pick(_frames("small"), [0, 2])                                   # the ball and the ridge at rho = 1
    twins = _bank(pkg, "twins")
    ref = _ref(fr, twins, max_shift=2)
    got = _measure(pkg, fr, twins, max_shift=2)
    MH.hold_device(got, ref, exact_template=False)                         # the two rows tie: which of them wins is the tie rule's (the smallest t)
    m = got["matches"][:, 0]
    for b in range(2):
        assert int(m[b, F["flags"]]) & MH.AMBIGUOUS and m[b, F["label"]] == -1 and m[b, F["template"]] == 0 and m[b, F["class"]] == 3
        assert m[b, F["second_class"]] == 5 and abs(m[b, F["margin"]]) <= ref["rows"][b][0].tol["margin"]
    assert m[0, F["score"]] > 0.99 and not int(m[0, F["flags"]]) & MH.WEAK
    small = _bank(pkg, "small")
    ref = _ref(fr, small, max_shift=2, accept_score=1.01)
    got = _measure(pkg, fr, small, max_shift=2, accept_score=1.01)
    MH.hold_device(got, ref)
    m = got["matches"][:, 0]
    assert (m[:, F["flags"]].astype(int) & MH.WEAK).all() and (m[:, F["label"]] == -1).all() and list(m[:, F["class"]]) == [0, 1]


@pytest.mark.gpu
def test_same_bits_alone_in_a_batch_and_twice(pkg):
    cfg, bank = MH.SMALL, _bank(pkg, "small")
    fr = _pick(_frames("small"), [4, 1, 8, 3, 11])
    ws = pkg.MatchWorkspace(MH.H, MH.W, 5, 2, bank.P, cfg["m"], bank.M)
    whole, again = _measure(pkg, fr, bank, ws, max_shift=cfg["m"]), _measure(pkg, fr, bank, ws, max_shift=cfg["m"])
    for k in whole:
        assert _same_bits(whole[k], again[k]), k                           # every bit, NaNs included
    for b in range(5):
        got = _measure(pkg, _pick(fr, [b]), bank, ws, max_shift=cfg["m"])
        for k in whole:
            assert _same_bits(got[k], whole[k][b:b + 1]), (b, k)
    ws.close()
    alone = _measure(pkg, fr, bank, max_shift=cfg["m"])                    # a workspace made for the call
    assert all(_same_bits(alone[k], whole[k]) for k in whole)
    with pytest.raises(ValueError):
        _measure(pkg, fr, bank, max_shift=9)
    with pytest.raises(ValueError):
        _measure(pkg, fr, bank, min_pixels=0)
    with pytest.raises(TypeError):
        _measure(pkg, fr, None)


# ---------------------------------------------------------------------------------------------------------------- GPU, through the session
def _session(pkg, n, max_batch):
    model, neg = pkg.load_calibration(os.path.join(G, "calibration_phase_to_height.json"))
    fm = pkg.load_force_calibration(os.path.join(G, "calibration_height_to_force.json"))["best_model"]
    return pkg.FtpSensor(pkg.synth.reference_frame(n), pkg.synth.roi_circle(n), pkg.FtpConfig.scaled(n), model, neg, fm, max_batch=max_batch)


@pytest.mark.gpu
def test_session_matches_and_predict_argument_equal_contact_matches(pkg):
    import torch
    n, K = 224, 4
    s = _session(pkg, n, 1)
    frame = CH.multi_contact_frame(pkg, n, 2)
    with pytest.raises(RuntimeError):
        s.matches(_bank(pkg, "small"))                                     # no predict yet
    with_contacts = s.predict(frame, contacts=K)
    pitch = 3.0 * float(s._scalar("mm_per_px")[0].item())                 # templates three sensor pixels to the template pixel
    bank = pkg.TemplateBank(MH.templates(9, 0.1), [0, 1, 2], SYM, pitch, rotations=12)
    r = s.matches(bank, K, max_shift=2)
    first = s._matches
    again = s.matches(bank, K, max_shift=2)
    assert s._matches is first                                             # the workspace is reused
    assert s.matches(bank, K, max_shift=1)["patches"].shape[2:] == (11, 11) and s._matches is not first
    with pytest.raises(TypeError):
        s.matches(bank, K, shift=2)
    direct = pkg.contact_matches(s._last_out["height_map_mm"], r["contact_index"], r["contacts"], r["count"], s._scalar("mm_per_px"), s.config.depth_eps_mm,
                                 bank, max_shift=2)
    torch.cuda.synchronize()
    assert set(r) == {"contacts", "count", "contact_index", "matches", "scores", "patches"}
    for k in ("matches", "scores", "patches"):
        assert _same_bits(r[k].cpu().numpy(), direct[k].cpu().numpy()) and _same_bits(again[k].cpu().numpy(), direct[k].cpu().numpy()), k
    used = int(r["count"][0].item())
    assert used >= 1 and (r["matches"][0, :used, 0].cpu().numpy() == MH.OK).any()
    res = s.predict(frame, contacts=K, matches=dict(bank=bank, max_shift=2))
    assert set(res) == set(with_contacts) | {"matches"} and len(res["matches"]) == len(res["contacts"]) == used
    table = pkg.matches_table(direct["matches"].cpu().numpy(), r["count"].cpu().numpy())
    for mt, want in zip(res["matches"], table):
        assert list(mt)[0] == "contact" and list(mt)[1:] == list(pkg.MATCH_NAMES) and isinstance(mt["status"], int)
        for name in pkg.MATCH_NAMES:
            assert mt[name] == want[name] or (isinstance(mt[name], float) and math.isnan(mt[name]) and math.isnan(want[name])), name
    with pytest.raises(ValueError):
        s.predict(frame, matches=dict(bank=bank))
    s.close()
    assert s._matches is None
