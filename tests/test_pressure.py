"""Pressure read-out (include/vistaf_pressure.h, PressureReadout, FtpSensor.pressure): the contact pressure map of an elastic skin.

The definition is restated twice in tests/pressure_helpers.py: `numpy_pressure` (np.fft.rfft2 / irfft2, float64) and `matmul_pressure`
(explicit DFT matrices from longdouble angles, np.matmul).  The CPU tests pin the model against closed forms -- the limits of S, Hertz's
contact on a half-space, the Winkler foundation a thin layer tends to -- with the figures the restatement gives and a margin of 2.  The
direct GPU tests hand the read-out hand-made planes and tables (no FTP session): 37 x 53 with pad 11 (48 x 64), 40 x 52 with pad 1
(41 x 53, odd Pw), 16 x 16 without padding, each as two batches of three frames that together hold an empty frame, a bump with NaN patches
and negative pixels, several bumps with pixels at eps and one float32 step above, and a frame of status 2 full of infinities; and 151 x 203
with pad 32, B = 2.  The plane is asked to lie within  2^-23 |ref| + max(16 e, 1e-12) peak  of `numpy_pressure`, e being the largest
distance, relative to a frame's peak, between the two restatements over these very cases (measured: 3.3e-14, so the floor decides).  The
tables are compared with math.fsum on the device's own plane.
"""
import csv
import ctypes
import math
import os
import re

import numpy as np
import pytest

import pressure_helpers as PH
from pressure_helpers import FR, R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
FLOOR = 1e-12
_CASES, _REF = {}, {}
CASE_NAMES = tuple("%dx%d_%s" % (h, w, ab) for h, w, _ in PH.SIZES for ab in "ab") + ("%dx%d" % PH.BIG[:2],)
MODEL_NAMES = tuple(PH.MODELS)


def _case(name):
    if not _CASES:
        _CASES.update(PH.cases())
    return _CASES[name]


def _reference(name, model):
    """(numpy_pressure, e of the case) computed once"""
    if (name, model) not in _REF:
        c, pad = _case(name)
        E, nu, t = PH.MODELS[model]
        a = PH.numpy_pressure(c["depth"], c["mpp"], c["eps"], pad, E, nu, t, c["status"])
        b = PH.matmul_pressure(c["depth"], c["mpp"], c["eps"], pad, E, nu, t, c["status"])
        e = 0.0
        for f in range(a.shape[0]):
            peak = np.abs(a[f]).max()
            if peak > 0.0:
                e = max(e, float(np.abs(a[f] - b[f]).max() / peak))
            else:
                assert not b[f].any()
        _REF[(name, model)] = (a, e)
    return _REF[(name, model)]


def _e():
    return max(_reference(n, m)[1] for n in CASE_NAMES for m in MODEL_NAMES)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_pressure_names_follow_the_header(pkg):
    hdr = open(os.path.join(ROOT, "include", "vistaf_pressure.h")).read()
    idx = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define VISTAF_PRESSURE_(\w+)\s+(\d+)\b", hdr)}
    assert sorted(idx.values()) == list(range(13))
    for name, i in idx.items():
        assert pkg.PRESSURE_NAMES[i].lower() == name
    assert list(pkg.PRESSURE_NAMES) == list(pkg._lib.PRESSURE_NAMES) == list(pkg.writers.PRESSURE_FIELDS) == list(PH.FIELDS)
    fidx = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define VISTAF_PRESSUREFRAME_(\w+)\s+(\d+)\b", hdr)}
    assert sorted(fidx.values()) == list(range(12))
    for name, i in fidx.items():
        assert pkg.PRESSURE_FRAME_NAMES[i].lower() == name
    assert list(pkg.PRESSURE_FRAME_NAMES) == list(pkg.writers.PRESSURE_FRAME_FIELDS) == list(PH.FRAME_FIELDS)
    assert int(re.search(r"#define VISTAF_NPRESSURE\s+(\d+)", hdr).group(1)) == pkg._lib.NPRESSURE == PH.NROW == 16
    assert int(re.search(r"#define VISTAF_NPRESSUREFRAME\s+(\d+)", hdr).group(1)) == pkg._lib.NPRESSUREFRAME == PH.NFRAME == 12
    ftp = open(os.path.join(ROOT, "include", "vistaf_ftp.h")).read()
    for name, i in zip(("X0", "Y0", "X1", "Y1"), PH.BBOX):
        assert int(re.search(r"#define VISTAF_CONTACT_BBOX_%s\s+(\d+)" % name, ftp).group(1)) == i
    for name in ("PressureReadout", "PRESSURE_NAMES", "PRESSURE_FRAME_NAMES", "pressure_table", "write_pressure_csv", "pressure_frame_record"):
        assert name in pkg.__all__ and hasattr(pkg, name)


def test_library_exports_every_declared_pressure_symbol(pkg):
    hdr = open(os.path.join(ROOT, "include", "vistaf_pressure.h")).read()
    declared = sorted(set(re.findall(r"\b(vistaf_pressure_\w+)\s*\(", hdr)))
    assert declared == sorted(["vistaf_pressure_create", "vistaf_pressure_measure", "vistaf_pressure_destroy"])
    lib = pkg._lib.load()
    for name in declared:
        assert hasattr(lib, name), name
    assert sorted(pkg._lib.PRESSURE_EXPORTS) == declared
    for other in ("vistaf_ftp.h", "vistaf_taxel.h", "vistaf_motion.h", "vistaf_cloud.h"):
        assert "vistaf_pressure" not in open(os.path.join(ROOT, "include", other)).read(), other      # its own header; the others are unchanged


def test_pressure_c_abi_refuses_null_and_bad_arguments(pkg):
    lib = pkg._lib.load()
    E_INVALID = -1
    inf = float("inf")
    buf = (ctypes.c_double * 64)()
    f32 = (ctypes.c_float * 16)()
    i8 = (ctypes.c_int8 * 16)()
    cnt = (ctypes.c_int32 * 2)()
    lib.vistaf_pressure_destroy(None)
    assert lib.vistaf_pressure_create(8, 8, 1, 4, 8, 1.0, 0.45, inf, None) == E_INVALID
    h = ctypes.c_void_p()
    for args in ((0, 8, 1, 4, 8, 1.0, 0.45, inf), (8, 0, 1, 4, 8, 1.0, 0.45, inf), (4097, 8, 1, 4, 8, 1.0, 0.45, inf), (8, 8, 0, 4, 8, 1.0, 0.45, inf),
                 (8, 8, 65536, 4, 8, 1.0, 0.45, inf), (8, 8, 1, -1, 8, 1.0, 0.45, inf), (8, 8, 1, 65, 8, 1.0, 0.45, inf), (8, 8, 1, 4, -1, 1.0, 0.45, inf),
                 (8, 8, 1, 4, 4097, 1.0, 0.45, inf), (8, 8, 1, 4, 8, 0.0, 0.45, inf), (8, 8, 1, 4, 8, -1.0, 0.45, inf), (8, 8, 1, 4, 8, inf, 0.45, inf),
                 (8, 8, 1, 4, 8, float("nan"), 0.45, inf), (8, 8, 1, 4, 8, 1.0, -0.01, inf), (8, 8, 1, 4, 8, 1.0, 0.5, inf), (8, 8, 1, 4, 8, 1.0, float("nan"), inf),
                 (8, 8, 1, 4, 8, 1.0, 0.45, 0.0), (8, 8, 1, 4, 8, 1.0, 0.45, -1.0), (8, 8, 1, 4, 8, 1.0, 0.45, -inf), (8, 8, 1, 4, 8, 1.0, 0.45, float("nan"))):
        assert lib.vistaf_pressure_create(*args, ctypes.byref(h)) == E_INVALID, args
        assert not h.value and lib.vistaf_ftp_last_error()
    # create touches no device, so the checks of measure run without one; nothing is launched or allocated for a refused call
    assert lib.vistaf_pressure_create(4, 4, 2, 2, 3, 1.0, 0.49, 2.0, ctypes.byref(h)) == 0 and h.value
    good = [f32, i8, buf, cnt, buf, buf, cnt, 0.01, 1, f32, buf, buf]
    assert lib.vistaf_pressure_measure(None, *good, None) == E_INVALID and b"null" in lib.vistaf_ftp_last_error()
    for i in (0, 4, 9, 11):
        args = list(good)
        args[i] = None
        assert lib.vistaf_pressure_measure(h, *args, None) == E_INVALID, i
        assert b"null" in lib.vistaf_ftp_last_error()
    for drop in ((1,), (2,), (3,), (10,), (1, 2, 3), (1, 2, 3, 10)):           # all four or none; none only with max_contacts 0
        args = list(good)
        for i in drop:
            args[i] = None
        assert lib.vistaf_pressure_measure(h, *args, None) == E_INVALID, drop
    for batch in (0, 3, -1):
        args = list(good)
        args[8] = batch
        assert lib.vistaf_pressure_measure(h, *args, None) == E_INVALID and b"batch" in lib.vistaf_ftp_last_error()
    for eps in (float("nan"), inf, -inf):
        args = list(good)
        args[7] = eps
        assert lib.vistaf_pressure_measure(h, *args, None) == E_INVALID and b"depth_eps_mm" in lib.vistaf_ftp_last_error()
    for i, off in ((0, 2), (3, 2), (6, 2), (9, 2), (2, 4), (4, 4), (5, 4), (10, 4), (11, 4)):
        args = list(good)
        args[i] = ctypes.c_void_p(ctypes.addressof(buf) + off)
        assert lib.vistaf_pressure_measure(h, *args, None) == E_INVALID and b"aligned" in lib.vistaf_ftp_last_error(), i
    lib.vistaf_pressure_destroy(h)
    assert lib.vistaf_pressure_create(4, 4, 2, 0, 0, 1.0, 0.0, inf, ctypes.byref(h)) == 0 and h.value
    assert lib.vistaf_pressure_measure(h, *good, None) == E_INVALID                     # a handle of max_contacts 0 takes no contact arguments
    lib.vistaf_pressure_destroy(h)


def test_pressure_scratch_size_is_the_last_carved_pointer(pkg):
    lib = pkg._lib.load()
    for B, h, w, pad in ((1, 16, 16, 1), (3, 37, 53, 11), (2, 151, 203, 32), (256, 224, 224, 32), (8, 1182, 1182, 32)):
        names = ctypes.create_string_buffer(32 * 8)
        off, size, align = ((ctypes.c_size_t * 8)() for _ in range(3))
        total = ctypes.c_size_t()
        n = lib.vistaf_ftp_test_scratch_regions(b"pressure", B, h, w, pad, 8, names, off, size, align, ctypes.byref(total))
        assert n == 2
        Ph, Wh = h + pad, (w + pad) // 2 + 1
        assert [names.raw[32 * i:32 * i + 32].split(b"\0")[0] for i in range(n)] == [b"rows", b"spectrum"]
        assert size[0] == B * h * Wh * 16 and size[1] == B * Ph * Wh * 16          # complex128 planes; the third one is the first
        assert off[0] == 0 and off[1] >= size[0] and off[1] % 256 == 0 and off[1] - size[0] < 256
        assert total.value == off[1] + size[1]
        assert size[1] >= B * h * w * 4                                             # the float32 depth plane parked there before stage 2


def test_pressure_readout_needs_a_device_or_refuses_bad_arguments(pkg):
    import torch
    for kw in (dict(max_contacts=65), dict(max_contacts=-1), dict(pad_px=-1), dict(E_mpa=0.0), dict(nu=0.5), dict(thickness_mm=0.0)):
        with pytest.raises(ValueError):
            pkg.PressureReadout(8, 8, 1, **kw)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            pkg.PressureReadout(8, 8, 1)


def test_pressure_table_and_csv_round_trip(pkg, tmp_path):
    rows = np.full((2, 3, 16), np.nan)
    rows[0, 0, :13] = np.arange(13) + 0.5
    rows[0, 0, [0, 6]] = (12, 7)
    rows[1, 0, :13] = 1.0
    rows[1, 1, :13] = 2.0
    rows[1, 1, 11] = np.nan
    tab = pkg.pressure_table(rows, [1, 5])
    assert [(r["frame"], r["contact"]) for r in tab] == [(0, 0), (1, 0), (1, 1)]
    assert list(tab[0])[2:] == list(pkg.PRESSURE_NAMES) and tab[0]["pixels"] == 12 and tab[0]["peak_index"] == 7 and isinstance(tab[0]["pixels"], int)
    path = pkg.write_pressure_csv(str(tmp_path), rows, [1, 5])
    with open(path, newline="") as fh:
        back = list(csv.DictReader(fh))
    assert len(back) == 3
    for r, q in zip(tab, back):
        for k, v in r.items():
            assert (isinstance(v, float) and np.isnan(v) and np.isnan(float(q[k]))) or float(q[k]) == v, k
    f = np.full(12, np.nan)
    f[11] = 2
    rec = pkg.pressure_frame_record(f)
    assert list(rec) == list(pkg.PRESSURE_FRAME_NAMES) and rec["status"] == 2 and rec["contacts"] == -1 and np.isnan(rec["scale"])
    with pytest.raises(ValueError):
        pkg.pressure_frame_record(np.zeros(11))
    with pytest.raises(ValueError):
        pkg.pressure_table(np.zeros((2, 3, 12)), [1, 1])


def test_S_has_the_winkler_and_the_half_space_limits():
    for nu in (0.0, 0.3, 0.45, 0.49):
        x = 1e-3 if nu <= 0.45 else 1e-4      # the next term of the series is of order x^2 / (1 - 2 nu): 2.2e-6 at nu = 0.45, 1.5e-5 at 0.49
        assert abs(float(PH.layer_S(x, nu)) / (x * (1.0 - 2.0 * nu) / (2.0 * (1.0 - nu) ** 2)) - 1.0) <= 1e-5, nu
        # 1 - S = (4 x^2 + 4 x + 10 - 24 nu + 16 nu^2) exp(-2x) / (3 - 4 nu) to first order: below 7e-15 at x = 20 for every nu <= 0.49
        # (6e-15 at nu = 0.45: S is 1 to a few units of the last place there, not bit for bit), below 2^-54 from x = 25 on
        assert (np.abs(PH.layer_S(np.array([20.0, 21.0, 22.5]), nu) - 1.0) <= 1e-14).all()
        assert (PH.layer_S(np.array([25.0, 100.0, 400.0, 1e4]), nu) == 1.0).all()
        # G(q) t / M -> 1 as q t -> 0, G -> Es q / 2 beyond: the two foundations the layer lies between
        E, t = 0.7, 1.3
        assert abs(float(PH.gain(1e-6 / t, E, nu, t)) / float(PH.gain(0.0, E, nu, t)) - 1.0) <= 1e-5
        assert abs(float(PH.gain(0.0, E, nu, t)) / (PH.winkler_modulus(E, nu) / t) - 1.0) <= 4 * PH.U2      # the same product, rounded in another order
        assert float(PH.gain(30.0 / t, E, nu, t)) == float(PH.gain(30.0 / t, E, nu, math.inf))


@pytest.mark.parametrize("n,s,measured", [(97, 0.3, 3.09e-3), (193, 0.15, 7.02e-4)])
def test_hertz_contact_on_a_half_space(n, s, measured):
    """E = 0.5, nu = 0.45, ball R = 6 mm, contact radius a = 2.4 mm, the exact surface displacement inside and outside the contact, centre
    at n // 2, pad = n.  The constant the half-space leaves open is removed as the mean difference over r < 0.8 a.  Measured: largest error
    over r < 0.8 a of 3.09e-3 p0 at n = 97, 0.3 mm/px, and of 7.03e-4 p0 at n = 193, 0.15 mm/px; asserted with a margin of 2."""
    E, nu, a = 0.5, 0.45, 2.4
    u, p, p0 = PH.hertz(n, s, E, nu, 6.0, a)
    got = PH.numpy_pressure(u[None].astype(np.float32), [s], 0.0, n, E, nu, math.inf)[0] / 1000.0
    m = PH.radius_mm(n, s) < 0.8 * a
    d = got - p
    err = float(np.abs(d[m] - d[m].mean()).max() / p0)
    print("n", n, "error over r < 0.8 a, in p0:", err)
    assert err <= 2.0 * measured


@pytest.mark.parametrize("t,measured", [(0.05, 1.36e-3), (0.2, 2.08e-2)])
def test_a_thin_layer_is_a_winkler_foundation(t, measured):
    """u = 0.5 exp(-(r / 4 mm)^2), 97 x 97 at 0.3 mm/px, pad 97.  Measured: max |p - M u / t| / max p = 1.36e-3 at t = 0.05 and 2.08e-2 at
    t = 0.2 (margin 2); the padded plane's sum equals M / t times the volume to 1e-6 (measured 2e-16)."""
    E, nu, n, s = 0.5, 0.45, 97, 0.3
    u = PH.gaussian_dent(n, s).astype(np.float32)
    full = PH.numpy_pressure(u[None], [s], 0.0, n, E, nu, t, full=True)[0] / 1000.0
    M = PH.winkler_modulus(E, nu)
    err = float(np.abs(full[:n, :n] - M * u.astype(np.float64) / t).max() / full.max())
    tot = float(full.sum() / (M / t * u.astype(np.float64).sum()) - 1.0)
    print("t", t, "distance to the Winkler foundation:", err, "sum:", tot)
    assert err <= 2.0 * measured and abs(tot) <= 1e-6


def test_a_flat_punch_loads_its_rim_and_a_ball_its_middle():
    n, s, E, nu, a = 97, 0.3, 0.5, 0.45, 2.4
    r = PH.radius_mm(n, s)
    mask = r <= a
    ball, _, _ = PH.hertz(n, s, E, nu, 6.0, a)
    punch = np.where(mask, 0.4, 0.4 * (2.0 / np.pi) * np.arcsin(np.minimum(a / np.maximum(r, a), 1.0)))      # the flat punch's exact surface
    index, tab, count = PH.disc_contact(mask)
    rows = {}
    for name, u in (("ball", ball), ("punch", punch)):
        p = PH.numpy_pressure(u[None].astype(np.float32), [s], 0.0, n, E, nu, math.inf).astype(np.float32)
        rows[name] = PH.tables(p, [s], 1, E, index, tab, count, [1.0])[0][0, 0]
        print(name, dict(zip(PH.FIELDS, rows[name])))
    assert rows["ball"][R["pixels"]] == rows["punch"][R["pixels"]] == mask.sum()
    assert rows["punch"][R["edge_share"]] > rows["ball"][R["edge_share"]]
    assert rows["punch"][R["peak_over_mean"]] > rows["ball"][R["peak_over_mean"]]
    for name in rows:
        assert abs(rows[name][R["offset_x_mm"]]) <= 1e-6 and abs(rows[name][R["offset_y_mm"]]) <= 1e-6      # a symmetric load sits on its centroid
        assert rows[name][R["force_N"]] == 1.0


def test_cases_are_what_they_claim():
    for name in CASE_NAMES:
        c, pad = _case(name)
        B, h, w = c["depth"].shape
        assert B == (2 if name == "%dx%d" % PH.BIG[:2] else 3) and c["index"].dtype == np.int8 and len(set(c["mpp"])) == B
        for b, kind in enumerate(c["kinds"]):
            d = c["depth"][b]
            if kind == "empty":
                assert not d.any() and c["count"][b] == 0
            if kind == "bump":
                assert np.isnan(d).any() and (d < 0).any() and c["count"][b] == 1 and np.isnan(d[c["index"][b] < 0]).any()
            if kind == "multi":
                assert c["count"][b] == 5 > PH.K and set(np.unique(c["index"][b])) == {-1, 0, 1, 2, 3}
                e32 = np.float32(c["eps"])
                assert d[0, 0] == e32 and d[0, 1] == np.nextafter(e32, np.float32(1)) and PH.clean(d, c["eps"])[0, 0] == 0 and PH.clean(d, c["eps"])[0, 1] > 0
            if kind == "bad":
                assert np.isinf(d).all() and c["status"][b] == 2
    kinds = {k for n in CASE_NAMES[:2] for k in _case(n)[0]["kinds"]}
    assert kinds == {"empty", "bump", "multi", "bad"}
    h, w, pad = PH.SIZES[0]
    assert ((h + pad) % 16, (w + pad) % 2) == (0, 0)
    h, w, pad = PH.SIZES[1]
    assert (w + pad) % 2 == 1 and all(v % 16 for v in (h, w, h + pad, (w + pad) // 2 + 1))


# ---------------------------------------------------------------------------------------------------------------- GPU, direct
def _measure(pkg, c, pad, model, frames=slice(None), force=True, reader=None, K=PH.K):
    import torch
    E, nu, t = PH.MODELS[model]
    B, h, w = c["depth"].shape
    pr = reader or pkg.PressureReadout(h, w, B, K, pad, E, nu, t)
    kw = dict(contact_index=c["index"][frames], contacts=c["tab"][frames], count=c["count"][frames]) if K else {}
    o = pr.measure(c["depth"][frames], c["mpp"][frames], c["eps"], force_N=c["force"][frames] if force else None, status=c["status"][frames], **kw)
    torch.cuda.synchronize()
    out = (o["pressure_kpa"].cpu().numpy(), o["rows"].cpu().numpy() if K else None, o["frame"].cpu().numpy())
    if reader is None:
        pr.close()
    return out


def _check_tables(c, model, p, rows, frame, force=True):
    E = PH.MODELS[model][0]
    B, h, w = p.shape
    want, wantf, terms = PH.tables(p, c["mpp"], PH.K, E, c["index"], c["tab"], c["count"], c["force"] if force else None, c["status"])
    assert np.array_equal(np.isnan(rows), np.isnan(want)) and np.array_equal(np.isnan(frame), np.isnan(wantf))
    for name in PH.EXACT:
        assert np.array_equal(rows[..., R[name]], want[..., R[name]], equal_nan=True), name
    for name in PH.FRAME_EXACT:
        assert np.array_equal(frame[:, FR[name]], wantf[:, FR[name]], equal_nan=True), name
    sc = PH.row_scales(want, wantf, c["mpp"], h, w)
    worst = 0.0
    for b in range(B):
        for k in range(PH.K):
            if (b, k) not in terms:
                continue
            tol = (2 * terms[(b, k)] + 16) * PH.U2
            for name in PH.FIELDS:
                g, v = rows[b, k, R[name]], want[b, k, R[name]]
                if np.isnan(v):
                    continue
                worst = max(worst, abs(g - v) / (tol * sc[b, k, R[name]]) if sc[b, k, R[name]] else float(g != v))
                assert abs(g - v) <= tol * sc[b, k, R[name]], (b, k, name, g, v)
        if b in terms:
            tol = (2 * terms[b] + 16) * PH.U2
            for name in PH.FRAME_FIELDS:
                g, v = frame[b, FR[name]], wantf[b, FR[name]]
                if not np.isnan(v):
                    assert abs(g - v) <= tol * abs(v), (b, name, g, v)
            if force and wantf[b, FR["contacts"]] > 0:
                tot = rows[b, :int(wantf[b, FR["contacts"]]), R["force_N"]].sum()
                assert abs(tot - c["force"][b]) <= 64 * 2.0 ** -52 * c["force"][b], (b, tot)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("model", MODEL_NAMES)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_direct_case_equals_numpy_pressure(pkg, name, model):
    c, pad = _case(name)
    ref, _ = _reference(name, model)
    e = _e()
    p, rows, frame = _measure(pkg, c, pad, model)
    assert p.dtype == np.float32 and np.isfinite(p).all()
    for b in range(p.shape[0]):
        peak = np.abs(ref[b]).max()
        d = np.abs(p[b].astype(np.float64) - ref[b])
        bar = 2.0 ** -23 * np.abs(ref[b]) + max(16.0 * e, FLOOR) * peak
        print(name, model, "frame", b, c["kinds"][b], "peak kPa", peak, "largest distance / peak", d.max() / peak if peak else d.max(),
              "without the float32 step", np.maximum(d - 2.0 ** -23 * np.abs(ref[b]), 0).max() / peak if peak else 0.0, "e", e)
        assert (d <= bar).all(), (b, float((d - bar).max()))
        if c["status"][b] != 0 or c["kinds"][b] == "empty":
            assert not p[b].any()
    worst = _check_tables(c, model, p, rows, frame)
    print(name, model, "tables: largest distance in units of the bar", worst)
    bad = c["status"] != 0
    assert np.isnan(rows[bad]).all() and np.isnan(np.delete(frame[bad], FR["status"], axis=1)).all() and (frame[bad, FR["status"]] == 2).all()
    assert np.isnan(rows[..., 13:]).all()


@pytest.mark.gpu
def test_same_bits_alone_first_last_and_again_and_without_the_force(pkg):
    name = "40x52_b"
    c, pad = _case(name)
    B, h, w = c["depth"].shape
    E, nu, t = PH.MODELS["layer"]
    pr = pkg.PressureReadout(h, w, B, PH.K, pad, E, nu, t)
    whole = _measure(pkg, c, pad, "layer", reader=pr)
    again = _measure(pkg, c, pad, "layer", reader=pr)
    assert all(PH.same_bits(a, b) for a, b in zip(whole, again))
    for b in range(B):                                                         # alone: first and last of its batch
        one = _measure(pkg, c, pad, "layer", frames=slice(b, b + 1), reader=pr)
        assert all(PH.same_bits(a[b:b + 1], o) for a, o in zip(whole, one)), b
    order = np.array([2, 0, 1])                                                # every frame in another position; the bad frame last
    sh = {k: (v[order] if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    moved = _measure(pkg, sh, pad, "layer", reader=pr)
    assert all(PH.same_bits(a[order], m) for a, m in zip(whole, moved))
    assert not whole[0][1].any() and c["status"][1] == 2                       # the bad frame's plane is zero ...
    clean = dict(c, depth=c["depth"].copy())
    clean["depth"][1] = 0.0
    other = _measure(pkg, clean, pad, "layer", reader=pr)
    assert all(PH.same_bits(a, o) for a, o in zip(whole, other))               # ... and its infinities reach no other frame
    # without the frame force only FORCE_N, SCALE and E_EFFECTIVE_MPA change, to NaN
    p, rows, frame = _measure(pkg, c, pad, "layer", force=False, reader=pr)
    assert PH.same_bits(p, whole[0])
    used = ~np.isnan(whole[1][..., 0])
    assert np.isnan(rows[..., R["force_N"]]).all() and not np.isnan(whole[1][..., R["force_N"]][used]).any()
    assert np.isnan(frame[:, [FR["scale"], FR["E_effective_MPa"]]]).all()
    keep = [i for i in range(16) if i != R["force_N"]]
    fkeep = [i for i in range(12) if i not in (FR["scale"], FR["E_effective_MPa"])]
    assert PH.same_bits(rows[..., keep], whole[1][..., keep]) and PH.same_bits(frame[:, fkeep], whole[2][:, fkeep])
    _check_tables(c, "layer", p, rows, frame, force=False)
    pr.close()
    # the plane and the frame row only
    p0, none, frame0 = _measure(pkg, c, pad, "layer", K=0)
    assert none is None and PH.same_bits(p0, whole[0])
    want = PH.tables(p0, c["mpp"], 0, E, force=c["force"], status=c["status"])[1]
    assert np.array_equal(np.isnan(frame0), np.isnan(want)) and (frame0[c["status"] == 0, FR["contacts"]] == 0).all()
    ok = ~np.isnan(want)
    assert (np.abs(frame0[ok] - want[ok]) <= (2 * h * w + 16) * PH.U2 * np.abs(want[ok])).all()
    with pytest.raises(ValueError):
        pkg.PressureReadout(h, w, 2, PH.K, pad, E, nu, t).measure(c["depth"], c["mpp"], c["eps"], contact_index=c["index"], contacts=c["tab"],
                                                               count=c["count"])      # batch > max_batch


# ---------------------------------------------------------------------------------------------------------------- GPU, through the session
@pytest.mark.gpu
def test_session_pressure_through_the_public_interface(pkg, tmp_path):
    import contacts_helpers as CH
    n, K = 224, 4
    frames = CH.multi_contact_batch(pkg, n, 0, 6)
    model, neg = pkg.load_calibration(os.path.join(G, "calibration_phase_to_height.json"))
    fm = pkg.load_force_calibration(os.path.join(G, "calibration_height_to_force.json"))["best_model"]
    ref = pkg.synth.reference_frame(n)
    s = pkg.FtpSensor(ref, pkg.synth.roi_circle(n), pkg.FtpConfig.scaled(n), model, neg, fm, max_batch=1)
    with pytest.raises(RuntimeError):
        s.pressure(K)                                    # no predict yet
    skin = dict(E_mpa=0.5, nu=0.45, thickness_mm=3.0)
    seen = 0
    for i in range(6):
        res = s.predict(frames[i], contacts=K, pressure=skin)
        assert res["pressure_kpa"].shape == (n, n) and res["pressure_kpa"].dtype == np.float32
        assert len(res["pressure"]) == len(res["contacts"]) == min(res["contact_count"], K)
        fr = res["pressure_frame"]
        assert list(fr) == list(pkg.PRESSURE_FRAME_NAMES) and fr["status"] == 0 and fr["contacts"] == len(res["contacts"])
        for r, q in zip(res["pressure"], res["contacts"]):
            assert list(r)[0] == "contact" and list(r)[1:] == list(pkg.PRESSURE_NAMES)
            assert r["pixels"] == q["pixels"]                                  # the footprint the contacts table measured
        if res["pressure"] and res["contact_count"] <= K:
            seen += 1
            tot = sum(r["force_N"] for r in res["pressure"])
            assert abs(tot - res["force_N"]) <= 64 * 2.0 ** -52 * abs(res["force_N"]), (i, tot, res["force_N"])
            assert abs(fr["E_effective_MPa"] - fr["scale"] * skin["E_mpa"]) <= 1e-15 * abs(fr["E_effective_MPa"])
        print("frame", i, "contacts", res["contact_count"], "force_N", res["force_N"], "frame row", fr)
    assert seen >= 3
    with pytest.raises(ValueError):
        s.pressure(K, E_mpa=0.6)                         # a changed skin needs reset=True
    raw = s.pressure(K, reset=True, E_mpa=0.6)
    assert tuple(raw["pressure"].shape) == (1, K, 16) and tuple(raw["pressure_frame"].shape) == (1, 12) and tuple(raw["pressure_kpa"].shape) == (1, n, n)
    path = pkg.write_pressure_csv(str(tmp_path), raw["pressure"].cpu().numpy(), raw["count"].cpu().numpy())
    with open(path, newline="") as fh:
        assert len(list(csv.DictReader(fh))) == min(int(raw["count"][0]), K)
    flat = s.predict(ref, contacts=K, pressure=dict(skin, reset=True))     # the reference frame fed as deformed: nothing touches
    assert flat is not None and flat["pressure"] == [] and flat["contact_count"] == 0 and flat["pressure_frame"]["contacts"] == 0
    assert np.isnan(flat["pressure_frame"]["cop_x"]) and np.isnan(flat["pressure_frame"]["cop_y"])
    plain = s.predict(frames[1])
    assert "pressure_kpa" not in plain and set(s.predict(frames[1], pressure=skin)) == set(plain) | {"pressure_kpa", "pressure_frame"}
    s.close()
    assert s._pressure is None
