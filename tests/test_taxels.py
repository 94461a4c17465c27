"""Taxel read-out (include/vistaf_taxel.h, taxels.TaxelReadout, FtpSensor.taxels): per-cell depth, volume, force share and the frame's wrench.

The definition is restated twice in tests/taxels_helpers.py: `numpy_taxels` (a loop per taxel, sums through math.fsum) is the reference,
`numpy_taxels_vec` (np.add.at) checks it.  The bar on a float field is (2 N + 16) * 2^-53 of the field's scale, N the frame's number of
contact pixels -- derived in the helper's docstring from the error of a sum of N non-negative terms in any order; pixel counts, maxima,
arg-max indices, active taxels, the peak taxel and the NaN pattern must be equal.  The direct GPU tests hand the read-out hand-made planes
(no FTP session), base shape 37 x 53, five frames: empty, one bump, several bumps with pixels at eps and one float32 step above and a
plateau that ties the maximum across cells, a frame with status != 0 full of garbage, and bumps on a noisy floor with negative pixels.
"""
import csv
import ctypes
import math
import os
import re

import numpy as np
import pytest

import contacts_helpers as CH
import taxels_helpers as TH
from taxels_helpers import F_, T_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
CASE_NAMES = ("grid_4x5", "polar_3x8", "whole_frame", "per_pixel", "checkerboard", "holes_unused", "strip_3x1100", "big_1182_grid_16x16")
_CASES, _REF = {}, {}


def _case(name):
    if not _CASES:
        _CASES.update(TH.cases())
    return _CASES[name]


def _reference(name):
    if name not in _REF:
        _REF[name] = TH.numpy_taxels(*TH.args(_case(name)))
    return _REF[name]


def _within_bar(got, want, c, what):
    assert got[0].dtype == np.float64 and got[1].dtype == np.float64
    assert TH.exact_equal(got, want), what
    worst, where = TH.worst_excess(got, want, c["mpp"], c["map"].shape)
    print(what, "largest error in units of the bar", worst, "at", where)
    assert worst <= 1.0, (what, worst, where)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_taxel_names_and_field_counts_follow_the_header(pkg):
    hdr = open(os.path.join(ROOT, "include", "vistaf_taxel.h")).read()
    idx = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define VISTAF_TAXEL_(\w+)\s+(\d+)\b", hdr)}
    assert sorted(idx.values()) == list(range(10))
    for name, i in idx.items():
        assert pkg.TAXEL_NAMES[i].lower() == name
    fidx = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define VISTAF_TAXELFRAME_(\w+)\s+(\d+)\b", hdr)}
    assert sorted(fidx.values()) == list(range(8))
    for name, i in fidx.items():
        assert pkg.TAXEL_FRAME_NAMES[i].lower() == name
    assert list(pkg.TAXEL_NAMES) == list(pkg._lib.TAXEL_NAMES) == list(pkg.writers.TAXEL_FIELDS) == list(TH.FIELDS)
    assert list(pkg.TAXEL_FRAME_NAMES) == list(pkg._lib.TAXEL_FRAME_NAMES) == list(pkg.writers.TAXEL_FRAME_FIELDS) == list(TH.FRAME_FIELDS)
    assert int(re.search(r"#define VISTAF_NTAXEL\s+(\d+)", hdr).group(1)) == pkg._lib.NTAXEL == TH.NTAXEL == 12
    assert int(re.search(r"#define VISTAF_NTAXELFRAME\s+(\d+)", hdr).group(1)) == pkg._lib.NTAXELFRAME == TH.NFRAME == 8
    assert int(re.search(r"#define VISTAF_TAXEL_NONE\s+(\w+)", hdr).group(1), 16) == pkg._lib.TAXEL_NONE == pkg.taxels.NONE == TH.NONE == 0xFFFF
    for name in ("TaxelLayout", "TaxelReadout", "TAXEL_NAMES", "TAXEL_FRAME_NAMES", "grid_layout", "polar_layout", "from_map", "taxels_table",
                 "write_taxels_csv", "taxels"):
        assert name in pkg.__all__ and hasattr(pkg, name)


def test_library_exports_exactly_the_declared_taxel_symbols(pkg):
    hdr = open(os.path.join(ROOT, "include", "vistaf_taxel.h")).read()
    declared = sorted(set(re.findall(r"\b(vistaf_taxel_\w+)\s*\(", hdr)))
    assert declared == sorted(["vistaf_taxel_create", "vistaf_taxel_measure", "vistaf_taxel_layout_info", "vistaf_taxel_destroy"])
    lib = pkg._lib.load()
    for name in declared:
        assert hasattr(lib, name), name
    assert sorted(pkg._lib.TAXEL_EXPORTS) == declared
    for other in ("vistaf_ftp.h", "vistaf_track.h", "vistaf_shape.h"):
        assert "vistaf_taxel" not in open(os.path.join(ROOT, "include", other)).read(), other      # its own header; the others are unchanged


def test_taxel_c_abi_refuses_bad_arguments_without_a_device(pkg):
    lib = pkg._lib.load()
    E_INVALID = -1
    lay = (ctypes.c_uint16 * 16)(*range(16))
    h = ctypes.c_void_p()
    nan, inf = float("nan"), float("inf")
    assert lib.vistaf_taxel_create(4, 4, 1, lay, 16, 0.0, 0.0, None) == E_INVALID and b"null" in lib.vistaf_ftp_last_error()
    assert lib.vistaf_taxel_create(4, 4, 1, None, 16, 0.0, 0.0, ctypes.byref(h)) == E_INVALID and b"null" in lib.vistaf_ftp_last_error()
    for a in ((0, 4, 1, lay, 16, 0.0, 0.0), (4, 0, 1, lay, 16, 0.0, 0.0), (-1, 4, 1, lay, 16, 0.0, 0.0), (65537, 1, 1, lay, 16, 0.0, 0.0),
              (1, 65537, 1, lay, 16, 0.0, 0.0),
              (65536, 65536, 1, lay, 16, 0.0, 0.0), (65536, 32768, 1, lay, 16, 0.0, 0.0),          # h * w overflows an int; refused before the plane is read
              (4, 4, 0, lay, 16, 0.0, 0.0), (4, 4, -2, lay, 16, 0.0, 0.0), (4, 4, 65536, lay, 16, 0.0, 0.0),
              (4, 4, 1, lay, 0, 0.0, 0.0), (4, 4, 1, lay, 65536, 0.0, 0.0), (4, 4, 1, lay, -1, 0.0, 0.0),
              (4, 4, 1, lay, 16, nan, 0.0), (4, 4, 1, lay, 16, 0.0, inf), (4, 4, 1, lay, 16, -inf, 0.0),
              (4, 4, 1, lay, 15, 0.0, 0.0)):                                                           # the value 15 is neither below 15 nor NONE
        assert lib.vistaf_taxel_create(*a, ctypes.byref(h)) == E_INVALID, a[:3] + a[4:]
        assert not h.value and lib.vistaf_ftp_last_error()
    lay[7] = 0xFFFE
    assert lib.vistaf_taxel_create(4, 4, 1, lay, 16, 0.0, 0.0, ctypes.byref(h)) == E_INVALID and b"layout value" in lib.vistaf_ftp_last_error()
    lay[7] = 0xFFFF                                                                                    # NONE is legal, and so is a taxel (7) without pixels
    assert lib.vistaf_taxel_create(4, 4, 2, lay, 16, 1.5, 1.5, ctypes.byref(h)) == 0 and h.value
    info = (ctypes.c_double * 64)()
    assert lib.vistaf_taxel_layout_info(None, info) == E_INVALID and lib.vistaf_taxel_layout_info(h, None) == E_INVALID
    assert lib.vistaf_taxel_layout_info(h, info) == 0
    got = np.array(info).reshape(16, 4)
    assert got[6].tolist()[:3] == [1.0, 2.0, 1.0] and got[7, 0] == 0.0 and np.isnan(got[7, 1:]).all() and np.isnan(got[:, 3]).all()
    # create touches no device, so the checks of measure run without one; nothing is launched for a refused call
    f32, buf, st = (ctypes.c_float * 32)(), (ctypes.c_double * 512)(), (ctypes.c_int32 * 2)()
    assert lib.vistaf_taxel_measure(None, f32, buf, buf, st, 0.01, 1, buf, buf, None) == E_INVALID and b"null" in lib.vistaf_ftp_last_error()
    for a in ((None, buf, buf, st, 0.01, 1, buf, buf), (f32, None, buf, st, 0.01, 1, buf, buf), (f32, buf, buf, st, 0.01, 1, None, buf),
              (f32, buf, buf, st, 0.01, 1, buf, None)):
        assert lib.vistaf_taxel_measure(h, *a, None) == E_INVALID and b"null" in lib.vistaf_ftp_last_error()
    for batch in (0, 3, -1):
        assert lib.vistaf_taxel_measure(h, f32, buf, None, None, 0.01, batch, buf, buf, None) == E_INVALID and b"batch" in lib.vistaf_ftp_last_error()
    for eps in (nan, inf, -inf):
        assert lib.vistaf_taxel_measure(h, f32, buf, None, None, eps, 1, buf, buf, None) == E_INVALID and b"depth_eps_mm" in lib.vistaf_ftp_last_error()
    lib.vistaf_taxel_destroy(h)
    lib.vistaf_taxel_destroy(None)


def test_layout_objects_refuse_bad_arguments(pkg):
    m = np.zeros((4, 5), np.uint16)
    for bad in (lambda: pkg.TaxelLayout(m, 0, (0, 0)), lambda: pkg.TaxelLayout(m, 65536, (0, 0)), lambda: pkg.TaxelLayout(m, 1, (np.nan, 0)),
                lambda: pkg.TaxelLayout(m + 3, 3, (0, 0)), lambda: pkg.TaxelLayout(m[0], 1, (0, 0)), lambda: pkg.TaxelLayout(m, 2, (0, 0), ["a"]),
                lambda: pkg.grid_layout(4, 5, 5, 1), lambda: pkg.grid_layout(4, 5, 0, 1), lambda: pkg.polar_layout(4, 5, (2, 2, 0), 1, 1),
                lambda: pkg.polar_layout(4, 5, (2, 2, 2), 0, 4), lambda: pkg.from_map(m.astype(np.float32)), lambda: pkg.from_map(m.astype(np.int64) + 70000)):
        with pytest.raises(ValueError):
            bad()
    lay = pkg.from_map(np.array([[0, -1, 3], [0xFFFF, 1, 1]]))
    assert lay.n_taxels == 4 and lay.origin == (1.0, 0.5) and lay.map.tolist() == [[0, 0xFFFF, 3], [0xFFFF, 1, 1]] and lay.map.dtype == np.uint16
    assert pkg.from_map(np.array([[2]]), origin=(5, 6), n_taxels=7, names=list("abcdefg")).names[6] == "g"
    with pytest.raises(ValueError):
        pkg.TaxelReadout(lay, 0)                                    # the library's own refusal


@pytest.mark.parametrize("h,w,rows,cols", [(37, 53, 4, 5), (224, 224, 8, 8), (10, 7, 10, 7), (9, 100, 1, 33)])
def test_grid_layout_cells(pkg, h, w, rows, cols):
    lay = pkg.grid_layout(h, w, rows, cols)
    assert lay.n_taxels == rows * cols and lay.shape == (h, w) and lay.origin == ((w - 1) / 2.0, (h - 1) / 2.0) and len(lay.names) == rows * cols
    assert np.array_equal(lay.map, TH.grid_map(h, w, rows, cols))                     # every pixel in the expected cell
    for r in range(rows):
        for c in range(cols):
            ys, xs = np.nonzero(lay.map == r * cols + c)
            assert ys.size == (ys.max() - ys.min() + 1) * (xs.max() - xs.min() + 1)   # a full rectangle
            assert h // rows <= ys.max() - ys.min() + 1 <= -(-h // rows) and w // cols <= xs.max() - xs.min() + 1 <= -(-w // cols)
    assert lay.names[cols - 1] == "r0c%d" % (cols - 1) and lay.names[-1] == "r%dc%d" % (rows - 1, cols - 1)
    # with a circle: the outside is NONE, the inside keeps its cell, the cells partition the disc
    circle = (w // 2, h // 2, min(h, w) // 2 - 1) if min(h, w) > 4 else (w // 2, h // 2, 1)
    disc = np.array([[(x - circle[0]) ** 2 + (y - circle[1]) ** 2 <= circle[2] ** 2 for x in range(w)] for y in range(h)])
    lc = pkg.grid_layout(h, w, rows, cols, roi_circle=circle)
    assert lc.origin == (float(circle[0]), float(circle[1]))
    assert (lc.map[~disc] == TH.NONE).all() and np.array_equal(lc.map[disc], lay.map[disc])
    info = pkg.TaxelReadout(lc, 1).layout_info()
    assert info[:, 0].sum() == disc.sum()


@pytest.mark.parametrize("h,w,circle,rings,sectors", [(37, 53, TH.CIRCLE, 3, 8), (64, 64, (31.5, 31.5, 30.0), 4, 12), (21, 30, (25, 3, 9.5), 2, 5),
                                                      (15, 15, (7, 7, 7), 1, 1)])
def test_polar_layout_cells(pkg, h, w, circle, rings, sectors):
    lay = pkg.polar_layout(h, w, circle, rings, sectors)
    want = TH.polar_map(h, w, circle, rings, sectors)
    assert lay.n_taxels == rings * sectors and lay.origin == (float(circle[0]), float(circle[1]))
    assert np.array_equal(lay.map, want)                                              # every pixel in the expected cell
    cx, cy, r = circle
    disc = np.array([[(x - cx) ** 2 + (y - cy) ** 2 <= r * r for x in range(w)] for y in range(h)])
    assert np.array_equal(lay.map != TH.NONE, disc)                                   # the outside is NONE, the cells partition the disc
    info = pkg.TaxelReadout(lay, 1).layout_info()
    assert info[:, 0].sum() == disc.sum() and info.shape == (rings * sectors, 4)
    # rings of equal radial width: every pixel of ring i lies between i r / rings and (i + 1) r / rings
    yy, xx = np.nonzero(disc)
    d = np.hypot(xx - cx, yy - cy)
    ring = lay.map[yy, xx] // sectors
    assert (d >= ring * r / rings - 1e-9).all() and (d <= (ring + 1) * r / rings + 1e-9).all()
    assert len(np.unique(lay.map[disc] % sectors)) == sectors


def test_layout_info_equals_the_hosts_counts_and_centres(pkg):
    for name, (m, T, origin) in TH.layouts().items():
        rd = pkg.TaxelReadout(pkg.TaxelLayout(m, T, origin), 1)
        info = rd.layout_info()
        rd.close()
        for t in range(T):
            ys, xs = np.nonzero(m == t)
            assert info[t, 0] == ys.size, (name, t)
            if ys.size:
                assert info[t, 1] == xs.sum() / xs.size and info[t, 2] == ys.sum() / ys.size, (name, t)
            else:
                assert np.isnan(info[t, 1]) and np.isnan(info[t, 2])
        assert np.isnan(info[:, 3]).all()
    assert (pkg.TaxelReadout(pkg.TaxelLayout(*TH.layouts()["holes_unused"]), 1).layout_info()[[1, 3, 4, 6, 8], 0] == 0).all()


@pytest.mark.parametrize("name", CASE_NAMES)
def test_both_restatements_agree(name):
    c = _case(name)
    want = _reference(name)
    _within_bar(TH.numpy_taxels_vec(*TH.args(c)), want, c, name)
    tax, frm = want
    assert tax.shape == (c["depth"].shape[0], c["T"], 12) and frm.shape == (c["depth"].shape[0], 8) and np.isnan(tax[..., 10:]).all()
    if name in TH.layouts():
        assert np.isnan(tax[3]).all() and np.isnan(frm[3]).all()                       # status 2
        assert frm[0, F_["active_taxels"]] == 0 and np.isnan(frm[0, F_["cop_x"]]) and (tax[0, :, T_["force_N"]] == 0).all()
        plateau = c["map"][15:23, 20:28]                                               # the tie goes to the lowest taxel
        assert frm[2, F_["peak_taxel"]] == plateau[plateau != TH.NONE].min() and (tax[2, :, T_["max_depth_mm"]] == np.float32(0.75)).sum() >= (2 if c["T"] > 1 else 1)
        d2, e32 = np.nan_to_num(c["depth"][2]), np.float32(TH.EPS)
        assert TH.frame_contact_pixels(tax)[2] == (d2 > e32)[c["map"] != TH.NONE].sum()
        if name == "whole_frame":                                                      # the pixels one step above eps count, the 11 at eps do not
            assert tax[2, 0, 0] == (d2 > e32).sum() == (d2 >= e32).sum() - 11 and (d2 == np.nextafter(e32, np.float32(1))).sum() == 28
            assert tax[2, 0, T_["argmax_index"]] == 15 * TH.W + 20


def test_without_force_only_forces_pressures_and_moments_change():
    c = _case("grid_4x5")
    (t0, f0), (t1, f1) = _reference("grid_4x5"), TH.numpy_taxels(*TH.args(c, force=False))
    ok = [0, 1, 2, 4]
    assert np.isnan(t1[ok][..., [8, 9]]).all() and np.isnan(f1[ok][:, [2, 5, 6]]).all()
    keep_t, keep_f = [0, 1, 2, 3, 4, 5, 6, 7, 10, 11], [0, 1, 3, 4, 7]
    assert np.array_equal(t0[..., keep_t], t1[..., keep_t], equal_nan=True) and np.array_equal(f0[:, keep_f], f1[:, keep_f], equal_nan=True)


def _hand_made():
    t = np.full((3, 2, 12), np.nan)
    t[0, 0, :10] = [12, 0.03, 1.5e-5, 0.02, 0.9, 417, 10.25, 7.5, 0.75, 12.5]
    t[0, 1, :10] = [0, 0.0, 0.0, 0.0, 0.0, np.nan, np.nan, np.nan, 0.0, 0.0]
    t[2, 0, :10] = [0, 0.0, 0.0, np.nan, 0.0, np.nan, np.nan, np.nan, np.nan, np.nan]      # a taxel without pixels, no force given
    t[2, 1, :10] = [3, 0.0075, 1e-6, 0.5, 0.6, 5, 1.0, 2.0, np.nan, np.nan]
    return t                                                                              # frame 1: status != 0, all NaN


def test_taxels_table_and_csv_round_trip(pkg, tmp_path):
    t = _hand_made()
    rows = pkg.taxels_table(t)
    assert [(r["frame"], r["taxel"]) for r in rows] == [(0, 0), (0, 1), (2, 0), (2, 1)]
    assert list(rows[0])[2:] == list(pkg.TAXEL_NAMES)
    for r in rows:
        assert all(isinstance(r[k], int) for k in ("frame", "taxel", "contact_pixels", "argmax_index"))
        assert all(isinstance(v, float) for k, v in r.items() if k not in ("frame", "taxel", "contact_pixels", "argmax_index"))
    assert rows[0]["contact_pixels"] == 12 and rows[0]["argmax_index"] == 417 and rows[0]["pressure_kPa"] == 12.5
    assert rows[1]["argmax_index"] == -1 and np.isnan(rows[1]["centroid_x"]) and rows[1]["force_N"] == 0.0
    assert np.isnan(rows[2]["mean_depth_mm"]) and np.isnan(rows[3]["force_N"]) and rows[3]["contact_pixels"] == 3
    assert len(pkg.taxels_table(t[2])) == 2 and pkg.taxels_table(t[1]) == []
    with pytest.raises(ValueError):
        pkg.taxels_table(t[:, :, :8])
    path = pkg.write_taxels_csv(str(tmp_path), t)
    with open(path, newline="") as f:
        back = list(csv.DictReader(f))
    assert len(back) == 4 and list(back[0]) == ["frame", "taxel"] + list(pkg.TAXEL_NAMES)
    for r, s in zip(rows, back):
        for k, v in r.items():
            got = float(s[k])
            assert (np.isnan(v) and np.isnan(got)) or got == v, k
    rec = pkg.taxel_frame_record([3, 1.5e-5, 0.75, 10.0, 7.0, 0.1, -0.2, 1])
    assert list(rec) == list(pkg.TAXEL_FRAME_NAMES) and rec["active_taxels"] == 3 and rec["peak_taxel"] == 1 and isinstance(rec["peak_taxel"], int)
    assert pkg.taxel_frame_record([0, 0.0, 0.5, np.nan, np.nan, np.nan, np.nan, np.nan])["peak_taxel"] == -1
    with pytest.raises(ValueError):
        pkg.taxel_frame_record([1.0, 2.0])


def test_measure_needs_a_device(pkg):
    import torch
    rd = pkg.TaxelReadout(pkg.grid_layout(8, 8, 2, 2), 1)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):
            rd.measure(np.zeros((1, 8, 8), np.float32), np.array([0.05]), 0.01)
    rd.close()
    rd.close()


# ---------------------------------------------------------------------------------------------------------------- GPU, direct
def _measure(pkg, c, force=True, status=True, frames=None, reader=None, max_batch=None):
    import torch
    sel = slice(None) if frames is None else frames
    depth = c["depth"][sel]
    rd = reader or pkg.TaxelReadout(pkg.TaxelLayout(c["map"], c["T"], c["origin"]), max_batch or depth.shape[0])
    out = rd.measure(depth, c["mpp"][sel], c["eps"], force_N=c["force"][sel] if force else None, status=c["status"][sel] if status else None)
    torch.cuda.synchronize()
    if reader is None:
        rd.close()
    return out["taxels"].cpu().numpy(), out["frame"].cpu().numpy()


def _bits_equal(a, b):
    return all(np.array_equal(x.view(np.int64), y.view(np.int64)) for x, y in zip(a, b))


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_direct_case_equals_numpy_taxels(pkg, name):
    c = _case(name)
    got = _measure(pkg, c)
    assert got[0].shape == (c["depth"].shape[0], c["T"], 12) and got[1].shape == (c["depth"].shape[0], 8)
    _within_bar(got, _reference(name), c, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["grid_4x5", "per_pixel", "holes_unused"])
def test_without_force_and_without_status(pkg, name):
    c = _case(name)
    full = _measure(pkg, c)
    # force NULL: NaN forces, pressures and moments, nothing else changes
    got = _measure(pkg, c, force=False)
    _within_bar(got, TH.numpy_taxels(*TH.args(c, force=False)), c, name + " without force")
    keep_t, keep_f, ok = [0, 1, 2, 3, 4, 5, 6, 7, 10, 11], [0, 1, 3, 4, 7], [0, 1, 2, 4]
    assert np.isnan(got[0][ok][..., [8, 9]]).all() and np.isnan(got[1][ok][:, [2, 5, 6]]).all()
    assert _bits_equal((got[0][..., keep_t].copy(), got[1][:, keep_f].copy()), (full[0][..., keep_t].copy(), full[1][:, keep_f].copy()))
    # status NULL: every frame counts as OK (the frames whose status is 0 here: the garbage frame is what status is for)
    sub = {k: (v[ok] if k in ("depth", "mpp", "force", "status") else v) for k, v in c.items()}
    got = _measure(pkg, sub, status=False)
    _within_bar(got, TH.numpy_taxels(*TH.args(sub, status=False)), sub, name + " without status")
    assert _bits_equal(got, (full[0][ok], full[1][ok]))
    bad = dict(sub, status=np.array([1, 0, -3, 0], np.int32))       # any non-zero status
    got = _measure(pkg, bad)
    assert np.isnan(got[0][[0, 2]]).all() and np.isnan(got[1][[0, 2]]).all() and _bits_equal((got[0][[1, 3]], got[1][[1, 3]]), (full[0][[1, 4]], full[1][[1, 4]]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["grid_4x5", "polar_3x8", "per_pixel", "checkerboard"])
def test_batch_equals_frames_one_by_one_and_two_calls_give_the_same_bits(pkg, name):
    c = _case(name)
    rd = pkg.TaxelReadout(pkg.TaxelLayout(c["map"], c["T"], c["origin"]), 5)
    whole, again = _measure(pkg, c, reader=rd), _measure(pkg, c, reader=rd)
    assert _bits_equal(whole, again)                                                   # every bit, NaNs included
    assert _bits_equal(whole, _measure(pkg, c))                                        # and from another handle
    for b in range(5):
        one = _measure(pkg, c, frames=slice(b, b + 1), reader=rd)
        assert _bits_equal(one, (whole[0][b:b + 1], whole[1][b:b + 1])), b
    with pytest.raises(ValueError):
        _measure(pkg, c, max_batch=2)                                                  # batch > max_batch
    with pytest.raises(ValueError):
        rd.measure(c["depth"][:, :-1], c["mpp"], c["eps"])
    with pytest.raises(ValueError):
        rd.measure(c["depth"], c["mpp"][:3], c["eps"])
    with pytest.raises(ValueError):
        rd.measure(c["depth"], c["mpp"], float("nan"))
    rd.close()


@pytest.mark.gpu
def test_large_taxels_equal_across_batches_too(pkg):
    c = _case("big_1182_grid_16x16")                                                   # every taxel is spread over the waves of a workgroup
    whole = _measure(pkg, c)
    one = _measure(pkg, c, frames=slice(1, 2))
    assert _bits_equal(one, (whole[0][1:], whole[1][1:]))
    assert whole[1][0, F_["active_taxels"]] > 20 and whole[0][..., 0].max() > 5000


# ---------------------------------------------------------------------------------------------------------------- GPU, through the session
def _session(pkg, n, max_batch):
    model, neg = pkg.load_calibration(os.path.join(G, "calibration_phase_to_height.json"))
    fm = pkg.load_force_calibration(os.path.join(G, "calibration_height_to_force.json"))["best_model"]
    return pkg.FtpSensor(pkg.synth.reference_frame(n), pkg.synth.roi_circle(n), pkg.FtpConfig.scaled(n), model, neg, fm, max_batch=max_batch)


@pytest.mark.gpu
def test_session_taxels_add_up_to_the_frame_scalars(pkg):
    import torch
    n, nb = 224, 6
    s = _session(pkg, n, nb + 1)
    frames = np.concatenate([CH.multi_contact_batch(pkg, n, 0, nb), pkg.synth.reference_frame(n)[None]])     # last: the reference itself
    o = s.predict_batch(frames)
    lay = pkg.grid_layout(n, n, 8, 8)
    r = s.taxels(lay)
    torch.cuda.synchronize()
    assert set(r) == {"taxels", "frame"} and tuple(r["taxels"].shape) == (nb + 1, 64, 12) and tuple(r["frame"].shape) == (nb + 1, 8)
    tax, frm = r["taxels"].cpu().numpy(), r["frame"].cpu().numpy()
    hm, sc, st = o["height_map_mm"].cpu().numpy(), o["scalars"].cpu().numpy(), o["status"].cpu().numpy()
    eps = s.config.depth_eps_mm
    s.close()
    assert (st == 0).all() and not (np.nan_to_num(hm, nan=0.0) < 0).any()             # the sums below need a map without negative pixels
    # the device rows are the definition on the device's own planes
    c = dict(depth=hm, map=lay.map, T=64, origin=lay.origin, mpp=sc[:, 6], force=sc[:, 3], status=st, eps=eps)
    _within_bar((tax, frm), TH.numpy_taxels(*TH.args(c)), c, "session")
    T = 64
    for b in range(nb):
        mm = float(sc[b, 6])
        vol, frc = math.fsum(tax[b, :, T_["volume_cm3"]]), math.fsum(tax[b, :, T_["force_N"]])
        print(b, "volume", vol, sc[b, 0], "rel", abs(vol - sc[b, 0]) / sc[b, 0], "force", frc, sc[b, 3], "rel", abs(frc - sc[b, 3]) / abs(sc[b, 3]))
        assert sc[b, 0] > 0 and abs(vol - sc[b, 0]) <= 2.0 ** -22 * sc[b, 0]           # the frame scalar is a float32-rounded sum
        assert float(tax[b, :, T_["contact_pixels"]].sum()) * (mm * mm) == sc[b, 1]  # contact_area_mm2 / mm_per_px^2, exactly
        assert abs(frc - sc[b, 3]) <= T * 2.0 ** -52 * abs(sc[b, 3]) and frm[b, F_["force_N"]] == sc[b, 3]
        peak = int(frm[b, F_["peak_taxel"]])
        assert peak == lay.map.ravel()[int(sc[b, 4])] and tax[b, peak, T_["max_depth_mm"]] == sc[b, 2]
        assert tax[b, peak, T_["argmax_index"]] == sc[b, 4]
    b = nb                                                                              # the reference frame as deformed: no contact
    assert frm[b, F_["active_taxels"]] == 0 and np.isnan(frm[b, F_["cop_x"]]) and np.isnan(frm[b, F_["cop_y"]]) and np.isnan(frm[b, F_["peak_taxel"]])
    assert (tax[b, :, T_["contact_pixels"]] == 0).all() and (tax[b, :, T_["force_N"]] == 0).all()


@pytest.mark.gpu
def test_taxels_leave_the_predict_path_alone(pkg):
    import torch
    n, nb = 224, 4
    a, other = CH.multi_contact_batch(pkg, n, 0, nb), pkg.synth.deformed_batch(n, 0, nb)

    def snap(o):
        return {k: v.clone() for k, v in o.items()}

    def equal(x, y):
        return all(torch.equal(x[k].contiguous().view(torch.uint8), y[k].contiguous().view(torch.uint8)) for k in x)
    s1, s2 = _session(pkg, n, nb), _session(pkg, n, nb)
    lay, polar = pkg.grid_layout(n, n, 8, 8), pkg.polar_layout(n, n, pkg.synth.roi_circle(n), 3, 8)
    with pytest.raises(RuntimeError):
        s1.taxels(lay)                                   # no predict yet
    o = s1.predict_batch(a)
    before = snap(o)
    plain = snap(s1.contacts(8, index_plane=True))
    got = snap(s1.taxels(lay))
    first = s1._taxels
    assert equal(snap(s1.taxels(lay)), got) and s1._taxels is first                             # reused
    assert tuple(s1.taxels(polar)["taxels"].shape) == (nb, 24, 12) and s1._taxels is not first  # rebuilt for another layout
    with pytest.raises(ValueError):
        s1.taxels(pkg.grid_layout(n, n + 1, 2, 2))
    torch.cuda.synchronize()
    assert equal(o, before)
    assert equal(snap(s1.contacts(8, index_plane=True)), plain)                                # a following contacts() is what it was
    after, fresh = snap(s1.predict_batch(other)), s2.predict_batch(other)
    torch.cuda.synchronize()
    assert equal(after, fresh)
    assert equal(s1.contacts(8, index_plane=True), s2.contacts(8, index_plane=True))
    s1.close()
    assert s1._taxels is None
    s2.close()


@pytest.mark.gpu
def test_predict_taxels_argument(pkg):
    n = 224
    s = _session(pkg, n, 1)
    frame = CH.multi_contact_frame(pkg, n, 2)
    lay = pkg.polar_layout(n, n, pkg.synth.roi_circle(n), 3, 8)
    plain = s.predict(frame)
    res = s.predict(frame, taxels=lay)
    assert set(res) == set(plain) | {"taxels", "taxel_frame"} and "taxels" not in plain and "taxel_frame" not in plain
    assert set(s.predict(frame)) == set(plain)
    assert isinstance(res["taxels"], np.ndarray) and res["taxels"].shape == (24, 12) and res["taxels"].dtype == np.float64
    assert list(res["taxel_frame"]) == list(pkg.TAXEL_FRAME_NAMES)
    f = res["taxel_frame"]
    assert isinstance(f["active_taxels"], int) and f["active_taxels"] >= 1 and f["force_N"] == res["force_N"]
    assert f["peak_taxel"] == lay.map.ravel()[res["argmax_depth_index"]] and res["taxels"][f["peak_taxel"], T_["max_depth_mm"]] == res["max_depth_mm"]
    s.close()
