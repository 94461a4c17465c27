"""Per-contact read-out (vistaf_ftp_contacts / FtpSensor.contacts): one record per 8-connected component of the blob filter's kept mask.

The definition is restated in NumPy in tests/contacts_helpers.py (`numpy_contacts`).  GPU tests: the table against that restatement on the
GPU's own planes (strict: only the new kernels are between them), against the oracle path (the project's bar for frame scalars), the
invariants that tie the table to the frame scalars, capacity, an empty frame, reproducibility, and no side effect on the predict path.
The rule for a frame whose status is not VISTAF_FRAME_OK (count 0, NaN rows) is asserted on the pair batch's featureless-reference sample
only when that sample does come back with such a status; no recipe is known to force one.
"""
import ctypes
import csv
import json
import os
import re

import numpy as np
import pytest

from oracle import ftp_oracle as O

import contacts_helpers as H
from contacts_helpers import F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
RTOL = 1e-4                 # the project's bar for frame scalars against the oracle (tests/test_gpu_parity.py)
ULP32 = 2.0 ** -23
K = 8


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_contact_names_follow_the_header(pkg):
    hdr = open(os.path.join(ROOT, "include", "vistaf_ftp.h")).read()
    idx = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define VISTAF_CONTACT_(\w+)\s+(\d+)\b", hdr)}
    expect = {"PIXELS": "pixels", "CONTACT_PIXELS": "contact_pixels", "AREA_MM2": "contact_area_mm2", "VOLUME_CM3": "volume_cm3",
              "MAX_DEPTH_MM": "max_depth_mm", "ARGMAX_INDEX": "argmax_index", "CENTROID_X": "centroid_x", "CENTROID_Y": "centroid_y",
              "FORCE_N": "force_N", "BBOX_X0": "bbox_x0", "BBOX_Y0": "bbox_y0", "BBOX_X1": "bbox_x1", "BBOX_Y1": "bbox_y1"}
    assert sorted(idx) == sorted(expect)
    assert sorted(idx.values()) == list(range(13))
    assert len(pkg.CONTACT_NAMES) == 13
    for cname, i in idx.items():
        assert pkg.CONTACT_NAMES[i] == expect[cname]
    assert list(pkg.CONTACT_NAMES) == list(pkg.writers.CONTACT_FIELDS) == list(H.FIELDS)
    assert int(re.search(r"#define VISTAF_NCONTACT\s+(\d+)", hdr).group(1)) == pkg._lib.NCONTACT == 16
    assert int(re.search(r"#define VISTAF_MAX_CONTACTS\s+(\d+)", hdr).group(1)) == pkg._lib.MAX_CONTACTS == 64


def test_c_abi_refuses_a_null_handle_and_null_outputs(pkg):
    lib = pkg._lib.load()
    buf = (ctypes.c_double * 16)()
    cnt = (ctypes.c_int32 * 1)()
    assert lib.vistaf_ftp_contacts(None, 1, 8, buf, cnt, None, None) == -1
    assert b"null" in lib.vistaf_ftp_last_error()
    assert lib.vistaf_ftp_contacts(None, 1, 8, None, None, None, None) == -1


def _hand_made():
    c = np.full((3, 2, 16), np.nan)
    c[0, 0, :13] = [40, 38, 1.5, 2e-3, 0.75, 1234, 10.25, 20.5, 0.125, 5, 6, 15, 26]
    c[0, 1, :13] = [7, 0, 0.0, 0.0, 0.009, 77, np.nan, np.nan, 0.0, 1, 1, 3, 3]        # no pixel above eps: NaN centroid
    c[2, 0, :13] = [9, 9, 0.3, 1e-4, 0.5, 99, 3.0, 4.0, 0.01, 2, 3, 4, 5]
    c[2, 1, :13] = [8, 8, 0.2, 9e-5, 0.4, 55, 1.0, 2.0, 0.009, 0, 0, 2, 2]
    return c, np.array([2, 0, 5], np.int32)       # frame 1: no contact (NaN rows); frame 2: five contacts, two written


def test_contacts_table_and_csv_round_trip(pkg, tmp_path):
    c, n = _hand_made()
    rows = pkg.contacts_table(c, n)
    assert [(r["frame"], r["contact"]) for r in rows] == [(0, 0), (0, 1), (2, 0), (2, 1)]
    assert list(rows[0])[2:] == list(pkg.CONTACT_NAMES)
    assert rows[0]["pixels"] == 40 and isinstance(rows[0]["pixels"], int) and rows[0]["argmax_index"] == 1234
    assert rows[0]["centroid_x"] == 10.25 and rows[0]["bbox_y1"] == 26 and np.isnan(rows[1]["centroid_x"])
    one = pkg.contacts_table(c[2], n[2])
    assert len(one) == 2 and one[1]["volume_cm3"] == 9e-5
    with pytest.raises(ValueError):
        pkg.contacts_table(c[:, :, :5], n)
    path = pkg.write_contacts_csv(str(tmp_path), c, n)
    with open(path, newline="") as f:
        back = list(csv.DictReader(f))
    assert len(back) == 4 and list(back[0]) == ["frame", "contact"] + list(pkg.CONTACT_NAMES)
    for r, s in zip(rows, back):
        for k, v in r.items():
            got = float(s[k])
            assert (np.isnan(v) and np.isnan(got)) or got == v, k
    rec = pkg.contacts_record(c, n)
    assert rec["contact_count"] == [2, 0, 5] and len(rec["contacts"]) == 4 and rec["contacts"][1]["centroid_x"] is None
    json.loads(json.dumps(rec, allow_nan=False))


def test_result_record_keeps_the_reference_keys(pkg):
    """the contact table is never merged into the reference's schemas"""
    res = {"estimated_grating_period_px": 12.0, "mm_per_px": 0.1, "volume_cm3": 1.0, "contact_area_mm2": 2.0, "max_depth_mm": 3.0, "force_N": 4.0,
           "contacts": [{"pixels": 1}], "contact_count": 1}
    rec = pkg.result_record(res, {"type": "linear0", "params": {"a": 1.0}}, "r", "d", "o", "f")
    assert "contacts" not in rec and "contact_count" not in rec and len(rec) == 13


# ---------------------------------------------------------------------------------------------------------------- GPU
def _cal(pkg):
    model, neg = pkg.load_calibration(os.path.join(G, "calibration_phase_to_height.json"))
    fm = pkg.load_force_calibration(os.path.join(G, "calibration_height_to_force.json"))["best_model"]
    return model, neg, fm


class Case:
    """one predict and its K = 8 table, read back to the host"""

    def __init__(self, pkg, sensor, out, cfg, fm, refs=None, frames=None, circle=None):
        import torch
        self.pkg, self.sensor, self.out, self.cfg, self.fm, self.refs, self.frames, self.circle = pkg, sensor, out, cfg, fm, refs, frames, circle
        self.tab = sensor.contacts(K, index_plane=True)
        torch.cuda.synchronize()
        self.B = int(out["status"].shape[0])
        self.h, self.w = sensor.h, sensor.w
        self.hm = out["height_map_mm"].cpu().numpy()
        self.scal = out["scalars"].cpu().numpy()
        self.status = out["status"].cpu().numpy()
        self.kept = sensor.intermediate("kept", self.B, torch.uint8).view(self.B, self.h, self.w).cpu().numpy().astype(bool)
        self.rows = self.tab["contacts"].cpu().numpy()
        self.count = self.tab["count"].cpu().numpy()
        self.index = self.tab["contact_index"].cpu().numpy()

    def force(self, v):
        return O.predict_force_from_volume(self.fm, v)


def _case_224(pkg, mode):
    n, nb = 224, 16
    cal = _cal(pkg)
    cfg = pkg.FtpConfig.scaled(n) if mode == "scaled" else pkg.FtpConfig.as_shipped()
    ref = pkg.synth.reference_frame(n)
    frames = np.concatenate([H.multi_contact_batch(pkg, n, 0, nb), ref[None]])       # last frame: the reference itself, no contact
    sensor = pkg.FtpSensor(ref, pkg.synth.roi_circle(n), cfg, cal[0], cal[1], cal[2], max_batch=nb + 1)
    return Case(pkg, sensor, sensor.predict_batch(frames), cfg, cal[2], refs=ref, frames=frames, circle=pkg.synth.roi_circle(n))


def _case_odd(pkg):
    h, w, circle = 151, 203, (98, 74, 66)
    cal = _cal(pkg)
    cfg = pkg.FtpConfig.scaled(160)
    ref, frames = H.odd_size_frames(h, w, circle, 65.83619546657023 * 160 / 1182, 6)
    sensor = pkg.FtpSensor(ref, circle, cfg, cal[0], cal[1], cal[2], max_batch=6)
    return Case(pkg, sensor, sensor.predict_batch(frames), cfg, cal[2], refs=ref, frames=frames, circle=circle)


def _case_native(pkg):
    n = 1182
    cal = _cal(pkg)
    cfg = pkg.FtpConfig.as_shipped()
    ref = pkg.synth.reference_frame(n, config=7)
    frames = np.stack([H.multi_contact_frame(pkg, n, 2), H.multi_contact_frame(pkg, n, 3)])
    sensor = pkg.FtpSensor(ref, pkg.synth.roi_circle(n), cfg, cal[0], cal[1], cal[2], max_batch=2)
    return Case(pkg, sensor, sensor.predict_batch(frames), cfg, cal[2], refs=ref, frames=frames, circle=pkg.synth.roi_circle(n))


def _case_pairs(pkg):
    n, nb = 224, 8
    cal = _cal(pkg)
    cfg = pkg.FtpConfig.scaled(n)
    periods = [pkg.synth.NATIVE_PERIOD_PX * n / pkg.synth.NATIVE_CROP, 11.3]          # two grating periods: per-pair mm_per_px
    refs = np.stack([pkg.synth._base(n, 0.0, np.random.default_rng(770000 + b), periods[b % 2]) for b in range(nb)])
    defs = np.stack([H.multi_contact_frame(pkg, n, 20 + b, periods[b % 2]) for b in range(nb)])
    refs[5] = 90                                                                      # featureless reference: its status is not pinned
    sensor = pkg.FtpSensor(None, pkg.synth.roi_circle(n), cfg, cal[0], cal[1], cal[2], max_batch=nb, frame_shape=(n, n))
    return Case(pkg, sensor, sensor.predict_pairs(refs, defs), cfg, cal[2], refs=refs, frames=defs, circle=pkg.synth.roi_circle(n))


_BUILDERS = {"224-scaled": lambda p: _case_224(p, "scaled"), "224-shipped": lambda p: _case_224(p, "shipped"), "151x203": _case_odd,
             "1182-shipped": _case_native, "pairs-224": _case_pairs}
_CASES = {}


def _get(pkg, name):
    if name not in _CASES:
        _CASES[name] = _BUILDERS[name](pkg)
    return _CASES[name]


ALL = list(_BUILDERS)


def _assert_no_contact(c, b):
    assert c.count[b] == 0
    assert np.isnan(c.rows[b]).all()
    assert (c.index[b] == -1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_table_equals_numpy_on_the_gpu_planes(pkg, name):
    c = _get(pkg, name)
    assert c.rows.shape == (c.B, K, 16) and c.count.shape == (c.B,) and c.index.shape == (c.B, c.h, c.w)
    import torch
    assert np.array_equal(c.sensor.masks(0)["contact_kept_by_depth"], c.kept[0])
    counts = []
    for b in range(c.B):
        if c.status[b] != 0:
            _assert_no_contact(c, b)
            continue
        mm = float(c.scal[b, 6])
        want, masks = H.numpy_contacts(c.hm[b], c.kept[b], mm, c.cfg.depth_eps_mm, c.force)
        got = c.rows[b]
        n = len(want)
        counts.append(n)
        print(name, "frame", b, "contacts", n, "peaks", np.round(want[:, F["max_depth_mm"]], 4))
        assert c.count[b] == n
        m = min(n, K)
        assert np.isnan(got[m:]).all() and np.isnan(got[:m, 13:]).all()
        for f in ("pixels", "contact_pixels", "bbox_x0", "bbox_y0", "bbox_x1", "bbox_y1", "max_depth_mm", "argmax_index", "contact_area_mm2"):
            assert np.array_equal(got[:m, F[f]], want[:m, F[f]]), (b, f, got[:m, F[f]], want[:m, F[f]])
        for k in range(m):
            v, v0 = got[k, F["volume_cm3"]], want[k, F["volume_cm3"]]
            print("   row", k, "volume", v, "numpy", v0, "centroid", got[k, 6:8], "numpy", want[k, 6:8])
            assert abs(v - v0) <= ULP32 * abs(v0), (b, k, v, v0)
            for f in ("centroid_x", "centroid_y"):
                a, a0 = got[k, F[f]], want[k, F[f]]
                assert (np.isnan(a) and np.isnan(a0)) or abs(a - a0) <= 1e-10, (b, k, f, a, a0)
            fN = got[k, F["force_N"]]
            assert abs(fN - c.force(float(v))) <= 1e-12 * max(1.0, abs(fN)), (b, k)
        assert np.array_equal(c.index[b], H.numpy_index_plane(masks, (c.h, c.w), K)), b
    if name.startswith("224"):
        assert max(counts) >= 3 and 1 in counts and counts[-1] == 0
    if name == "pairs-224":
        assert len({round(float(v), 6) for v in c.scal[c.status == 0, 6]}) >= 2          # the pairs do bring their own mm_per_px


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["224-scaled", "224-shipped"])
def test_table_against_the_oracle_path(pkg, name):
    c = _get(pkg, name)
    cal = _cal(pkg)
    rs = O.make_reference_state(c.refs, *c.circle, c.cfg)
    seen = []
    for b in range(c.B):
        o = O.process_frame(c.frames[b], rs, c.cfg, cal[0], cal[1], force_model=cal[2])
        want, masks = H.numpy_contacts(o["height_map_mm_crop"], o["contact_kept_by_depth"], o["mm_per_px"], c.cfg.depth_eps_mm, c.force)
        n = len(want)
        seen.append(n)
        assert c.count[b] == n, b
        got = c.rows[b]
        m = min(n, K)
        for f in ("pixels", "bbox_x0", "bbox_y0", "bbox_x1", "bbox_y1"):
            assert np.array_equal(got[:m, F[f]], want[:m, F[f]]), (b, f)
        if n:
            assert got[0, F["argmax_index"]] == want[0, F["argmax_index"]] == o["argmax_depth_index"]
        hm = np.nan_to_num(o["height_map_mm_crop"], nan=0.0).astype(np.float64)
        peak = float(hm.max())
        yy, xx = np.mgrid[0:c.h, 0:c.w]
        for k in range(m):
            for f in ("max_depth_mm", "volume_cm3", "contact_area_mm2"):
                assert abs(got[k, F[f]] - want[k, F[f]]) <= RTOL * max(abs(want[k, F[f]]), 1e-9), (b, k, f, got[k, F[f]], want[k, F[f]])
            # centroid: a per-pixel error of 1e-4 * peak (the map's bar) moves sum(x d) / sum(d) by at most 1e-4 peak sum|x - cx| / sum d
            comp = masks[k] & (np.nan_to_num(o["height_map_mm_crop"], nan=0.0) > np.float32(c.cfg.depth_eps_mm))
            sd = hm[comp].sum()
            for f, coord in (("centroid_x", xx), ("centroid_y", yy)):
                bound = RTOL * peak * np.abs(coord[comp] - want[k, F[f]]).sum() / sd + 1e-9
                print(name, b, k, f, got[k, F[f]], want[k, F[f]], "bound", bound)
                assert abs(got[k, F[f]] - want[k, F[f]]) <= bound, (b, k, f)
    assert max(seen) >= 3 and 1 in seen and seen[-1] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_invariants_tie_the_table_to_the_frame_scalars(pkg, name):
    c = _get(pkg, name)
    big = c.sensor.contacts(64)
    rows64, cnt64 = big["contacts"].cpu().numpy(), big["count"].cpu().numpy()
    for b in range(c.B):
        if c.status[b] != 0:
            continue
        assert not (np.nan_to_num(c.hm[b], nan=0.0) < 0).any()          # the invariants need a map without negative pixels
        n = int(cnt64[b])
        assert n <= 64 and n == c.count[b]
        r, s = rows64[b, :n], c.scal[b]
        mm = float(s[6])
        assert float(r[:, F["contact_pixels"]].sum()) * (mm * mm) == s[1]
        if n == 0:
            assert s[0] == 0.0 and s[1] == 0.0
            continue
        assert r[:, F["max_depth_mm"]].max() == r[0, F["max_depth_mm"]] == s[2]
        assert r[0, F["argmax_index"]] == s[4]
        key = [(-r[k, F["max_depth_mm"]], r[k, F["argmax_index"]]) for k in range(n)]
        assert key == sorted(key)
        vs = float(r[:, F["volume_cm3"]].sum())
        print(name, b, "sum of volumes", vs, "frame", s[0], "rel", abs(vs - s[0]) / s[0])
        assert abs(vs - s[0]) <= (n + 1) * ULP32 * s[0]


@pytest.mark.gpu
def test_capacity_truncates_and_says_so(pkg):
    c = _get(pkg, "224-shipped")
    b = int(np.argmax(c.count))
    assert c.count[b] >= 3
    import torch
    for k in (1, 2):
        t = c.sensor.contacts(k, index_plane=True)
        assert t["contacts"].shape == (c.B, k, 16)
        assert torch.equal(t["count"], c.tab["count"])
        assert torch.equal(t["contacts"].view(torch.int64), c.tab["contacts"][:, :k].contiguous().view(torch.int64))
        idx = t["contact_index"].cpu().numpy()
        assert np.array_equal(idx, np.where(c.index < k, c.index, -1))
        assert (idx[b][c.index[b] >= k] == -1).all() and (c.index[b] >= k).any()
    with pytest.raises(ValueError):
        c.sensor.contacts(0)
    with pytest.raises(ValueError):
        c.sensor.contacts(65)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["224-scaled", "224-shipped"])
def test_reference_frame_as_deformed_has_no_contact(pkg, name):
    c = _get(pkg, name)
    b = c.B - 1
    assert c.status[b] == 0 and not c.kept[b].any()
    _assert_no_contact(c, b)
    assert (c.count[:b] >= 1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["224-scaled", "1182-shipped"])
def test_two_reads_and_a_second_predict_give_the_same_bits(pkg, name):
    import torch
    c = _get(pkg, name)

    def same(t):
        return all(torch.equal(t[k].view(torch.uint8), c.tab[k].view(torch.uint8)) for k in ("contacts", "count", "contact_index"))
    assert same(c.sensor.contacts(K, index_plane=True))
    assert same(c.sensor.contacts(K, index_plane=True))
    c.sensor.predict_batch(c.frames)
    assert same(c.sensor.contacts(K, index_plane=True))


@pytest.mark.gpu
def test_contacts_leave_the_predict_path_alone(pkg):
    import torch
    n, nb = 224, 4
    cal = _cal(pkg)
    cfg = pkg.FtpConfig.scaled(n)
    ref = pkg.synth.reference_frame(n)
    a, other = H.multi_contact_batch(pkg, n, 0, nb), pkg.synth.deformed_batch(n, 0, nb)

    def snap(o):
        return {k: v.clone() for k, v in o.items()}

    def equal(x, y):
        return all(torch.equal(torch.nan_to_num(x[k], nan=-7.0) if x[k].is_floating_point() else x[k],
                               torch.nan_to_num(y[k], nan=-7.0) if y[k].is_floating_point() else y[k]) for k in x)
    s1 = pkg.FtpSensor(ref, pkg.synth.roi_circle(n), cfg, cal[0], cal[1], cal[2], max_batch=nb)
    with pytest.raises(RuntimeError):
        s1.contacts()                                    # no predict yet
    buf, cnt = torch.empty((nb, K, 16), dtype=torch.float64, device="cuda"), torch.empty((nb,), dtype=torch.int32, device="cuda")
    assert pkg._lib.load().vistaf_ftp_contacts(s1._h, nb, K, buf.data_ptr(), cnt.data_ptr(), None, None) == -3      # VISTAF_E_STATE: before any predict
    o = s1.predict_batch(a)
    before = snap(o)
    planes = {p: s1.intermediate(p, nb, torch.uint8).clone() for p in ("kept", "depth", "labels", "peak_bits")}
    assert pkg._lib.load().vistaf_ftp_contacts(s1._h, nb - 1, K, buf.data_ptr(), cnt.data_ptr(), None, None) == -3  # another batch than the predict's
    s1.contacts(K, index_plane=True)
    s1.contacts(64)
    torch.cuda.synchronize()
    assert equal(o, before)
    for p, v in planes.items():
        assert torch.equal(s1.intermediate(p, nb, torch.uint8), v), p
    after = snap(s1.predict_batch(other))
    s2 = pkg.FtpSensor(ref, pkg.synth.roi_circle(n), cfg, cal[0], cal[1], cal[2], max_batch=nb)
    fresh = s2.predict_batch(other)
    torch.cuda.synchronize()
    assert equal(after, fresh)
    assert torch.equal(s1.contacts(K)["contacts"].view(torch.int64), s2.contacts(K)["contacts"].view(torch.int64))


@pytest.mark.gpu
def test_single_frame_predict_adds_contacts_only_when_asked(pkg):
    n = 224
    cal = _cal(pkg)
    ref = pkg.synth.reference_frame(n)
    sensor = pkg.FtpSensor(ref, pkg.synth.roi_circle(n), pkg.FtpConfig.as_shipped(), cal[0], cal[1], cal[2], max_batch=1)
    frame = H.multi_contact_frame(pkg, n, 15)
    plain = sensor.predict(frame)
    assert "contacts" not in plain and "contact_count" not in plain
    res = sensor.predict(frame, contacts=2)
    assert set(res) == set(plain) | {"contacts", "contact_count"}
    assert res["contact_count"] >= 3 and len(res["contacts"]) == 2
    top = res["contacts"][0]
    assert top["argmax_index"] == res["argmax_depth_index"] and top["max_depth_mm"] == res["max_depth_mm"]
    assert top["argmax_xy"] == (top["argmax_index"] % n, top["argmax_index"] // n)
    x0, y0, x1, y1 = top["bbox"]
    assert x0 <= top["centroid_xy"][0] <= x1 and y0 <= top["centroid_xy"][1] <= y1
