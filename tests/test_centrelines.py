"""The centreline read-out (include_ext/vistaf_centreline.h): skeleton, axis path, length, width profile, end tangents and bend of every contact.

The reference is tests/centreline_helpers.py: Guo-Hall thinning by whole-plane boolean operations, the exact distance by a separable integer
minimum, the walk by a plain queue, the measures one IEEE operation at a time.  On the CPU: the properties of the thinning and of the path on
random masks, the distance against brute force, the numbers the definition gives on known shapes, the capacity and table rules, the header
against `_lib`'s tables, the refusals of the C ABI (they come before any HIP call) and the writers.  On the GPU every written field must have
the reference's bits (NaN where it has NaN), and stations, their D2, offsets and the skeleton plane must be equal exactly."""
import csv
import ctypes
import os
import re

import numpy as np
import pytest

import centreline_helpers as CL
import contacts_helpers as CH
from abi_helpers import _hold_against, _prototypes
from abi_helpers import _same_f64_bits as _same_bits
from centreline_helpers import F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
HEADER = os.path.join(ROOT, "include_ext", "vistaf_centreline.h")
E_INVALID = -1
NWRITTEN = 37
CL_X0, CL_X1 = 9, 11                  # VISTAF_CONTACT_BBOX_X0, _X1


# ------------------------------------------------------------------------------------------------------------------------------------ CPU
def _random_masks(n, seed, top=14):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        h, w = rng.integers(1, top), rng.integers(1, top)
        yield rng.random((h, w)) < rng.uniform(0.5, 1.0)


def test_thinning_keeps_pieces_and_holes_on_random_masks():
    n = 0
    for m in _random_masks(600, 0):
        if not m.any():
            continue
        s, passes = CL.thin(m)
        assert s.any() and not (s & ~m).any()
        assert CL.components(s, True) == CL.components(m, True) and CL.holes(s) == CL.holes(m)
        again, more = CL.thin(s)
        assert np.array_equal(again, s) and more == 0
        n += 1
    assert n > 590


def test_path_is_simple_and_ordered_on_random_masks():
    for m in _random_masks(300, 1):
        if not m.any():
            continue
        s, _ = CL.thin(m)
        path, seed = CL.walk(s, CL.d2_plane(m))
        assert len(set(path)) == len(path) and all(s[y, x] for x, y in path) and s[seed[1], seed[0]]
        assert all(max(abs(p[0] - q[0]), abs(p[1] - q[1])) == 1 for p, q in zip(path, path[1:]))
        assert (path[0][1], path[0][0]) <= (path[-1][1], path[-1][0])


def test_distance_equals_brute_force():
    for m in _random_masks(150, 2):
        assert np.array_equal(CL.d2_plane(m), CL.d2_brute(m))


def test_known_numbers():
    for n in (2, 3, 4, 5):
        assert CL.thin(np.ones((n, n), bool))[0].sum() == 1
    assert CL.thin(np.ones((2, 6), bool))[0].sum() == 5
    rec, path, dd, sk = CL.measure_mask(CL.bar(40, 80, 10, 15, 69, 21), 1.0)
    assert [rec[F[n]] for n in ("skeleton_pixels", "stations", "path_length_mm", "length_mm", "interior_stations")] == [54, 54, 53, 60, 38]
    assert [rec[F[n]] for n in ("width_mean_mm", "width_min_mm", "width_max_mm", "sagitta_mm", "tortuosity")] == [7, 7, 7, 0, 1]
    assert [rec[F[n]] for n in ("a_tx", "a_ty", "b_tx", "b_ty")] == [1, 0, -1, 0] and sk.sum() == 54 and len(path) == 54
    one = np.zeros((9, 9), bool)
    one[4, 4] = True
    rec = CL.measure_mask(one, 1.0)[0]
    assert int(rec[F["status"]]) & 7 == CL.POINT and rec[F["length_mm"]] == 1.0 and rec[F["interior_stations"]] == 0
    assert all(np.isnan(rec[F[n]]) for n in ("a_tx", "a_ty", "b_tx", "b_ty", "tortuosity", "width_mean_mm", "width_min_mm", "width_max_mm"))
    rec = CL.measure_mask(CL.disc(64, 64, 30, 30, 20), 1.0)[0]
    assert rec[F["stations"]] == 3 and abs(rec[F["elongation"]] - 1.0) <= 0.05
    rec = CL.measure_mask(CL.tee(40, 60, 5, 5, 41, 20, 5), 1.0)[0]
    assert int(rec[F["status"]]) & CL.BRANCHED and rec[F["stations"]] < rec[F["skeleton_pixels"]]


def test_reference_capacity_and_table_rules():
    names, c = CL.hand_made(24, 32)
    full = CL.reference(c["index"], c["tab"], c["count"], c["mpp"], c["depth"], 8, 512)
    out = full["centrelines"]
    b = names.index("borders_and_corner")
    n = out[b, :, F["stations"]].astype(int)
    assert list(full["offsets"][b]) == [0] + list(np.cumsum(n)) and (out[b, :, F["stations_written"]] == n).all()
    assert not (out[b, :, F["status"]].astype(int) & CL.TRUNCATED).any()
    cap = int(n[:2].sum() + n[2] // 2)                                              # cuts in the middle of row 2
    cut = CL.reference(c["index"], c["tab"], c["count"], c["mpp"], c["depth"], 8, cap)
    assert list(cut["offsets"][b]) == [0, n[0], n[0] + n[1]] + [n[0] + n[1]] * 6 and cut["stations"][b] == full["stations"][b][:n[0] + n[1]]
    assert list(cut["centrelines"][b, :, F["stations_written"]]) == [n[0], n[1], 0, 0, 0, 0, 0, 0]
    assert ((cut["centrelines"][b, 2:, F["status"]].astype(int) & CL.TRUNCATED) != 0).all()
    none = CL.reference(c["index"], c["tab"], c["count"], c["mpp"], None, 8, None)["centrelines"]
    used = ~np.isnan(none[..., 0])
    assert (none[..., F["stations_written"]][used] == 0).all() and np.isnan(none[..., F["depth_mean_mm"]]).all()
    # contacts that run off the skin say so at the end that does, and only there
    flags = [(int(out[b, k, F["a_at_border"]]), int(out[b, k, F["b_at_border"]])) for k in range(8)]
    assert flags[0] == (1, 0) and flags[1] == (0, 1) and flags[2] == (1, 0) and flags[3] == (0, 1) and flags[7] == (0, 0), flags
    assert all(max(f) == 1 for f in flags[4:7])
    t = names.index("ring_disc_empty_pieces")
    assert out[t, 2, F["pixels"]] == 0 and out[t, 2, F["status"]] == CL.NO_PIXELS and np.isnan(out[t, 2, F["length_mm"]]) and (out[t, 2, :7] == 0).all()
    two = CL.row_mask(c["index"][t], c["tab"][t, 3], 3)
    assert CL.components(two, True) == 2 and out[t, 3, F["end_pixels"]] == 4                # both pieces counted, one walked
    comp = CL.components(full["skeleton"][t] == 3, True)
    assert comp == 2 and out[t, 3, F["stations"]] < out[t, 3, F["skeleton_pixels"]]
    q = names.index("clipped_and_bad_boxes")
    assert out[q, 0, F["pixels"]] == 15 * 4 and out[q, 1, F["pixels"]] == 9 * 5                 # the box rules, in and out of the frame
    assert (out[q, 2:5, F["status"]] == CL.NO_PIXELS).all()
    assert np.isnan(out[names.index("count_zero")]).all() and not np.isnan(out[names.index("count_above_K"), :, 0]).any()
    assert (full["skeleton"][names.index("count_zero")] == -1).all()


def test_centreline_names_and_signatures_follow_the_header(pkg):
    hdr = open(HEADER).read()
    idx = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define VISTAF_CENTRELINE_(\w+)\s+(\d+)\b", hdr)}
    assert sorted(idx.values()) == list(range(NWRITTEN))
    for name, i in idx.items():
        assert pkg.CENTRELINE_NAMES[i] == name
    assert list(pkg.CENTRELINE_NAMES) == list(pkg._lib.CENTRELINE_NAMES) == list(pkg.writers.CENTRELINE_FIELDS) == list(CL.FIELDS)
    assert int(re.search(r"#define VISTAF_NCENTRELINE\s+(\d+)", hdr).group(1)) == pkg._lib.NCENTRELINE == CL.NCENTRELINE == 40
    status = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define VISTAF_CLST_(\w+)\s+(\d+)\b", hdr)}
    assert status == pkg.CENTRELINE_STATUS == {"ok": CL.OK, "no_pixels": CL.NO_PIXELS, "point": CL.POINT, "branched": CL.BRANCHED, "truncated": CL.TRUNCATED}
    for name in ("centreline", "CENTRELINE_NAMES", "contact_centrelines", "CentrelineWorkspace", "centrelines_table", "write_centrelines_csv",
                 "centreline_frame_record"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    for name in ("contact_centrelines", "CentrelineWorkspace", "workspace_bytes", "default_max_stations", "trim"):
        assert hasattr(pkg.centreline, name)
    lib = pkg._lib.load()
    table = pkg._lib.CENTRELINE_SIGNATURES
    _hold_against(_prototypes(hdr), table, lib)
    assert sorted(table) == ["vistaf_centreline_measure", "vistaf_centreline_workspace_bytes"]
    assert not set(table) & {n for g in pkg._lib.SIGNATURES.values() for n in g}
    hooks = open(os.path.join(os.path.dirname(pkg.__file__), "csrc", "test_hooks_centreline.h")).read()
    _hold_against(_prototypes(hooks), pkg._lib.CENTRELINE_TEST_SIGNATURES, lib)
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other.endswith(".h"):
            assert "vistaf_centreline" not in open(os.path.join(ROOT, "include", other)).read(), other


def test_tier_hook_is_monotone_and_refuses(pkg):
    lib = pkg._lib.load()
    tier = lib.vistaf_ftp_test_centreline_tier
    assert tier(1, 1) == 1 and tier(64, 64) == 1 and tier(224, 224) == 1 and tier(32767, 32767) == 0
    last = 1
    for n in range(1, 600):
        t = tier(n, n)
        assert t in (0, 1) and t <= last
        last = t
    assert last == 0
    for bad in ((0, 8), (8, 0), (32768, 8), (8, 32768)):
        assert tier(*bad) == E_INVALID


def test_centreline_c_abi_refuses_with_the_arguments_name(pkg):
    lib = pkg._lib.load()
    err = lib.vistaf_ftp_last_error
    n = ctypes.c_size_t(1)
    assert lib.vistaf_centreline_workspace_bytes(8, 8, 1, 8, None) == E_INVALID and b"bytes" in err()
    for args, word in (((0, 8, 1, 8), b"h "), ((32768, 8, 1, 8), b"h "), ((8, 0, 1, 8), b"w "), ((8, 32768, 1, 8), b"w "),
                       ((32767, 32767, 1, 8), b"h * w"), ((8, 8, 0, 8), b"batch"), ((8, 8, 1, 0), b"max_contacts"), ((8, 8, 1, 65), b"max_contacts")):
        n.value = 1
        assert lib.vistaf_centreline_workspace_bytes(*args, ctypes.byref(n)) == E_INVALID and n.value == 0 and word in err(), args
    assert lib.vistaf_centreline_workspace_bytes(8, 8, 1, 8, ctypes.byref(n)) == 0 and n.value > 0
    assert pkg.centreline.workspace_bytes(8, 8, 1, 8) == n.value
    small = pkg.centreline.workspace_bytes(224, 224, 2, 8)
    assert small < pkg.centreline.workspace_bytes(320, 320, 2, 8) // 2 and pkg.centreline.default_max_stations(24, 32) == 112
    with pytest.raises(ValueError, match="max_contacts"):
        pkg.centreline.workspace_bytes(8, 8, 1, 0)
    # measure: host memory stands in for the device's, every call is refused before any HIP call
    f64, i32, i8, f32 = (ctypes.c_double * 512)(), (ctypes.c_int32 * 64)(), (ctypes.c_int8 * 64)(), (ctypes.c_float * 64)()
    raw = (ctypes.c_uint8 * 2048)()
    ws = (ctypes.addressof(raw) + 255) & ~255
    p = ctypes.addressof
    good = dict(idx=p(i8), tab=p(f64), cnt=p(i32), mpp=p(f64), dep=p(f32), B=1, h=8, w=8, K=8, span=8, V=8, out=p(f64), st=p(i32), d2=p(i32), offs=p(i32),
                sk=p(i8), ws=ws, n=n.value)

    def call(**kw):
        a = dict(good, **kw)
        return lib.vistaf_centreline_measure(a["idx"], a["tab"], a["cnt"], a["mpp"], a["dep"], a["B"], a["h"], a["w"], a["K"], a["span"], a["V"], a["out"],
                                             a["st"], a["d2"], a["offs"], a["sk"], a["ws"], a["n"], None)
    for kw, words in ((dict(idx=None), [b"d_contact_index"]), (dict(tab=None), [b"d_contacts"]), (dict(cnt=None), [b"d_count"]),
                      (dict(mpp=None), [b"d_mm_per_px"]), (dict(out=None), [b"d_centrelines"]), (dict(ws=None), [b"d_workspace"]),
                      (dict(st=None), [b"d_stations", b"d_offsets"]), (dict(st=None, offs=None), [b"d_stations", b"d_station_d2"]),
                      (dict(offs=None), [b"d_offsets", b"d_stations"]), (dict(h=0), [b"h "]), (dict(w=32768), [b"w "]), (dict(B=0), [b"batch"]),
                      (dict(K=0), [b"max_contacts"]), (dict(K=65), [b"max_contacts"]), (dict(V=-1), [b"max_stations"]),
                      (dict(span=0), [b"tangent_span"]), (dict(span=1025), [b"tangent_span"]),
                      (dict(tab=p(f64) + 4), [b"d_contacts", b"aligned"]), (dict(cnt=p(i32) + 2), [b"d_count", b"aligned"]),
                      (dict(dep=p(f32) + 2), [b"d_depth_mm", b"aligned"]), (dict(d2=p(i32) + 1), [b"d_station_d2", b"aligned"]),
                      (dict(ws=ws + 128), [b"d_workspace", b"aligned"]), (dict(n=n.value - 1), [b"workspace_bytes"]), (dict(n=0), [b"workspace_bytes"])):
        assert call(**kw) == E_INVALID, kw
        assert all(word in err() for word in words), (kw, err())


def _hand_table():
    t = np.full((2, 3, 40), np.nan)
    t[0, 0, :37] = [420, 54, 3, 2, 0, 54, 54, 0, 13, 18, 66, 18, 5.3, 6.0, 5.3, 1.0, 0.0, 0, 38, 0.7, 0.7, 8, 0.7, 8, 0.7, 8.571428571428571, 1, 0, -1,
                    0, 0, 0, 0.31, 0.3, 0.32, 0.4, 17]
    t[0, 1, :7] = 0
    t[0, 1, 7] = 1
    t[1, 0, :32] = [1, 1, 0, 0, 0, 1, 0, 18, 4, 4, 4, 4, 0.0, 0.1, 0.0, np.nan, np.nan, 0, 0, np.nan, np.nan, np.nan, np.nan, np.nan, 0.1, 1.0, np.nan,
                    np.nan, np.nan, np.nan, 0, 0]
    return t, np.array([2, 1], np.int32)


def test_centreline_writers_round_trip(pkg, tmp_path):
    t, n = _hand_table()
    rows = pkg.centrelines_table(t, n)
    assert [(r["frame"], r["contact"]) for r in rows] == [(0, 0), (0, 1), (1, 0)]
    assert list(rows[0])[2:] == list(pkg.CENTRELINE_NAMES) and isinstance(rows[0]["pixels"], int) and isinstance(rows[0]["length_mm"], float)
    assert rows[1]["pixels"] == 0 and rows[1]["status"] == 1 and np.isnan(rows[1]["length_mm"]) and rows[1]["sagitta_station"] == -1
    assert rows[2]["status"] == 18 and rows[2]["depth_peak_station"] == -1 and np.isnan(rows[2]["a_tx"])
    with pytest.raises(ValueError):
        pkg.centrelines_table(t[..., :20], n)
    path = pkg.write_centrelines_csv(str(tmp_path), t[:1], n[:1])
    back = list(csv.DictReader(open(path)))
    assert len(back) == 2 and list(back[0]) == ["frame", "contact"] + list(pkg.CENTRELINE_NAMES)
    for r, q in zip(rows, back):
        for name in pkg.CENTRELINE_NAMES:
            v = float(q[name])
            assert v == r[name] or (np.isnan(v) and np.isnan(r[name]))
    st = np.array([[4, 4], [9, 9], [0, 0]], np.int32)
    d2 = np.array([1, 7, 0], np.int32)
    rec = pkg.centreline_frame_record(t[1, :1], st, d2, np.array([0, 0]), 1)
    assert rec["stations"] == [None] and rec["d2"] == [None] and rec["contact_count"] == 1                 # stations 1, written 0: left out
    t[1, 0, 6] = 1
    rec = pkg.centreline_frame_record(t[1, :1], st, d2, np.array([0, 1]), 1)
    assert rec["stations"] == [[[4, 4]]] and rec["d2"] == [[1]] and rec["centrelines"][0]["tortuosity"] is None and "frame" not in rec["centrelines"][0]
    rec = pkg.centreline_frame_record(t[0, 1:2], st, d2, np.array([0, 0]), 1)
    assert rec["centrelines"][0]["length_mm"] is None
    with pytest.raises(ValueError):
        pkg.centreline_frame_record(t[0, :2], st, d2, np.array([0, 0]), 2)


def test_contact_centrelines_needs_a_device_or_refuses_bad_arguments(pkg):
    import torch
    idx, tab = np.zeros((1, 8, 8), np.int8), np.zeros((1, 4, 16))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):
            pkg.contact_centrelines(idx, tab, [1], [0.1])
        return
    for bad in ((idx[0], tab, [1], [0.1]), (idx, tab[:, :, :8], [1], [0.1]), (idx, tab, [1, 2], [0.1]), (idx, tab, [1], [0.1, 0.2]),
                (idx, tab, [1], [0.1], np.zeros((1, 8, 9), np.float32))):
        with pytest.raises(ValueError):
            pkg.contact_centrelines(*bad)
    for kw in (dict(max_stations=-1), dict(tangent_span=0), dict(tangent_span=1025)):
        with pytest.raises(ValueError):
            pkg.contact_centrelines(idx, tab, [1], [0.1], **kw)


# ------------------------------------------------------------------------------------------------------------- GPU, through the C ABI
SENTINEL = -77


def _abi(pkg, c, V, span=8, depth=True, polylines=True, d2=True, skeleton=True, sel=None):
    """vistaf_centreline_measure on case c (frames `sel`): dict of arrays; every output is filled with a sentinel first; the polyline pointers
    are NULL with polylines=False, d_station_d2 alone with d2=False, d_skeleton with skeleton=False"""
    import torch
    sel = slice(None) if sel is None else sel
    dev = torch.device("cuda:0")
    idx, tab = torch.as_tensor(c["index"][sel]).to(dev).contiguous(), torch.as_tensor(c["tab"][sel]).to(dev).contiguous()
    cnt, mpp = torch.as_tensor(c["count"][sel]).to(dev).contiguous(), torch.as_tensor(c["mpp"][sel]).to(dev).contiguous()
    dep = torch.as_tensor(c["depth"][sel]).to(dev).contiguous() if depth else None
    B, h, w = idx.shape
    K = tab.shape[1]
    nbytes = pkg.centreline.workspace_bytes(h, w, B, K)
    ws = torch.empty((nbytes + 256,), dtype=torch.uint8, device=dev)
    out = torch.full((B, K, 40), 123.0, dtype=torch.float64, device=dev)
    st = torch.full((B, max(V, 1), 2), SENTINEL, dtype=torch.int32, device=dev)
    sd = torch.full((B, max(V, 1)), SENTINEL, dtype=torch.int32, device=dev)
    offs = torch.full((B, K + 1), SENTINEL, dtype=torch.int32, device=dev)
    sk = torch.full((B, h, w), SENTINEL, dtype=torch.int8, device=dev)
    pkg._handle.call(dev, "vistaf_centreline_measure", idx.data_ptr(), tab.data_ptr(), cnt.data_ptr(), mpp.data_ptr(), dep.data_ptr() if depth else None,
                     B, h, w, K, span, V, out.data_ptr(), st.data_ptr() if polylines else None, sd.data_ptr() if polylines and d2 else None,
                     offs.data_ptr() if polylines else None, sk.data_ptr() if skeleton else None, (ws.data_ptr() + 255) & ~255, nbytes,
                     pkg._handle.stream(dev))
    torch.cuda.synchronize()
    return {"centrelines": out.cpu().numpy(), "stations": st.cpu().numpy()[:, :V], "d2": sd.cpu().numpy()[:, :V], "offsets": offs.cpu().numpy(),
            "skeleton": sk.cpu().numpy()}


def _check(got, want, what, polylines=True, d2=True, skeleton=True):
    out, ref = got["centrelines"], want["centrelines"]
    assert out.shape == ref.shape, what
    for i, name in enumerate(CL.FIELDS):
        assert _same_bits(out[..., i], ref[..., i]), (what, name, out[..., i], ref[..., i])
    assert np.isnan(out[..., NWRITTEN:]).all(), (what, "reserved fields")
    if polylines:
        assert np.array_equal(got["offsets"], want["offsets"]), (what, got["offsets"], want["offsets"])
        for b, sb in enumerate(want["stations"]):
            n = len(sb)
            assert np.array_equal(got["stations"][b, :n], np.array(sb, np.int32).reshape(-1, 2)), (what, b)
            assert (got["stations"][b, n:] == SENTINEL).all(), (what, b, "the tail was written")
            if d2:
                assert np.array_equal(got["d2"][b, :n], np.array(want["d2"][b], np.int32)) and (got["d2"][b, n:] == SENTINEL).all(), (what, b)
    else:
        assert (got["stations"] == SENTINEL).all() and (got["offsets"] == SENTINEL).all()
    if not (polylines and d2):
        assert (got["d2"] == SENTINEL).all()
    assert np.array_equal(got["skeleton"], want["skeleton"]) if skeleton else (got["skeleton"] == SENTINEL).all(), what


_REF = {}


def _hand_case(h, w):
    if (h, w) not in _REF:
        names, c = CL.hand_made(h, w)
        _REF[(h, w)] = (names, c, CL.reference(c["index"], c["tab"], c["count"], c["mpp"], c["depth"], 8, 1024))
    return _REF[(h, w)]


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", [(24, 32), (37, 53)])
def test_hand_made_cases_equal_the_reference(pkg, h, w):
    names, c, want = _hand_case(h, w)
    ref = want["centrelines"]
    bars = names.index("bars")
    assert (ref[bars, :4, F["branch_pixels"]] == 0).all() and ref[bars, 0, F["thinning_passes"]] == 0 and ref[bars, 3, F["thinning_passes"]] >= 3
    other = names.index("diagonal_tee_pixel")
    assert int(ref[other, 1, F["status"]]) & CL.BRANCHED and int(ref[other, 2, F["status"]]) == CL.POINT and ref[other, 0, F["a_ty"]] > 0
    _check(_abi(pkg, c, 1024), want, f"hand-made {h}x{w}")


def _batch_case():
    if "batch" not in _REF:
        h, w = 64, 96
        a = CL.Scene(h, w).paint(0, CL.arc(h, w, 48, 70, 50, 5, -2.6, -0.6))
        s = CL.Scene(h, w).paint(0, CL.sine_cable(h, w, 14, 60, 4))
        f = CL.Scene(h, w).paint(0, CL.bar(h, w, 4, 4, 40, 8)).paint(1, CL.disc(h, w, 70, 20, 11)).paint(2, CL.tee(h, w, 10, 30, 31, 18, 3))
        f.paint(3, CL.diagonal_bar(h, w, 56, 36, 24, 4))
        c = CL.pack([a, s, f], [0.05, 0.0731, 0.1])
        yy, xx = np.mgrid[0:h, 0:w]
        c["depth"] = np.stack([(0.2 + 0.004 * ((5 * xx + 3 * yy + 11 * b) % 29) + 0.002 * yy).astype(np.float32) for b in range(3)])
        _REF["batch"] = c
    return _REF["batch"]


def _batch_ref(span, depth, V):
    key = ("batch", span, depth, V)
    if key not in _REF:
        c = _batch_case()
        _REF[key] = CL.reference(c["index"], c["tab"], c["count"], c["mpp"], c["depth"] if depth else None, span, V)
    return _REF[key]


@pytest.mark.gpu
@pytest.mark.parametrize("span", [1, 8, 1024])
def test_batch_of_curves_with_spans_depth_and_capacities(pkg, span):
    c = _batch_case()
    ample = _batch_ref(span, True, 512)
    ref = ample["centrelines"]
    assert ref[1, 0, F["a_at_border"]] == 1 and ref[1, 0, F["b_at_border"]] == 1 and ref[1, 0, F["tortuosity"]] > 1.1       # the cable crosses the frame
    assert abs(ref[0, 0, F["sagitta_mm"]]) > 10 * 0.05 and ref[0, 0, F["stations"]] > 60
    n = ref[2, :4, F["stations"]].astype(int)
    cap = int(n[:2].sum() + n[2] // 2)                                               # cuts in the middle of the third frame's rows
    _check(_abi(pkg, c, 512, span), ample, f"span {span}")
    _check(_abi(pkg, c, cap, span), _batch_ref(span, True, cap), f"span {span} capacity {cap}")
    zero = _abi(pkg, c, 0, span, depth=False)
    _check(zero, _batch_ref(span, False, 0), f"span {span} capacity 0 no depth")
    assert np.isnan(zero["centrelines"][..., F["depth_mean_mm"]:NWRITTEN]).all()
    null = _abi(pkg, c, 512, span, polylines=False, skeleton=False)
    _check(null, _batch_ref(span, True, None), f"span {span} NULL polylines", polylines=False, skeleton=False)
    nod2 = _abi(pkg, c, 512, span, d2=False)
    _check(nod2, ample, f"span {span} NULL d2", d2=False)


@pytest.mark.gpu
def test_batch_positions_and_second_call_give_the_same_bits(pkg):
    import torch
    c = _batch_case()
    keys = ("centrelines", "stations", "d2", "offsets", "skeleton")
    whole, again = _abi(pkg, c, 512), _abi(pkg, c, 512)
    for k in keys:
        assert np.array_equal(whole[k].view(np.uint8), again[k].view(np.uint8)), k
    for i in range(3):
        one = _abi(pkg, c, 512, sel=slice(i, i + 1))
        for k in keys:
            assert np.array_equal(one[k].view(np.uint8), whole[k][i:i + 1].view(np.uint8)), (i, k)
    perm = [2, 0, 1]
    moved = _abi(pkg, {k: (v[perm] if isinstance(v, np.ndarray) else v) for k, v in c.items()}, 512)
    for k in keys:
        assert np.array_equal(moved[k].view(np.uint8), whole[k][perm].view(np.uint8)), k
    # the Python entry point: the same bits, the dict's keys, trim
    r = pkg.contact_centrelines(c["index"], c["tab"], c["count"], c["mpp"], c["depth"], max_stations=512)
    torch.cuda.synchronize()
    assert set(r) == {"centrelines", "stations", "station_d2", "offsets", "skeleton"} and _same_bits(r["centrelines"].cpu().numpy(), whole["centrelines"])
    assert np.array_equal(r["offsets"].cpu().numpy(), whole["offsets"]) and np.array_equal(r["skeleton"].cpu().numpy(), whole["skeleton"])
    t = pkg.centreline.trim(r)
    want = _batch_ref(8, True, 512)
    assert not t["overflow"] and [len(p) for p in t["stations"]] == [1, 1, 4]
    assert np.array_equal(t["stations"][2][1], np.array(want["stations"][2], np.int32)[want["offsets"][2, 1]:want["offsets"][2, 2]])
    assert np.array_equal(np.concatenate(t["d2"][2]), np.array(want["d2"][2], np.int32))
    small = pkg.contact_centrelines(c["index"], c["tab"], c["count"], c["mpp"], max_stations=0, skeleton=False)
    assert set(small) == {"centrelines"} and pkg.centreline.trim(small)["overflow"]
    assert tuple(pkg.contact_centrelines(c["index"], c["tab"], c["count"], c["mpp"])["stations"].shape) == (3, 2 * (64 + 96), 2)


@pytest.mark.gpu
def test_both_storage_tiers_equal_the_reference(pkg):
    tier = pkg._lib.load().vistaf_ftp_test_centreline_tier
    n = next(v for v in range(65, 2000) if tier(v, v) == 0)                        # the smallest square box that leaves LDS
    assert tier(64, 64) == 1 and tier(n - 1, n - 1) == 1 and tier(n, n) == 0
    h = w = n + 6
    big = CL.bar(h, w, 3, 2, 3 + n - 1, 2 + n - 1) & ~CL.bar(h, w, 3 + n // 2 - 20, 2, 3 + n // 2 + 19, 2 + n // 3)      # a full square with a 40-pixel notch
    small = CL.bar(h, w, 100, 90, 163, 153) & ~CL.bar(h, w, 120, 90, 139, 120)                                        # 64 x 64 with a notch
    c = CL.pack([CL.Scene(h, w).paint(0, big), CL.Scene(h, w).paint(0, small)], 0.05)
    assert [int(c["tab"][b, 0, CL_X1] - c["tab"][b, 0, CL_X0] + 1) for b in range(2)] == [n, 64]
    yy, xx = np.mgrid[0:h, 0:w]
    c["depth"] = np.stack([(0.1 + 0.001 * ((xx + 2 * yy + b) % 31)).astype(np.float32) for b in range(2)])
    want = CL.reference(c["index"], c["tab"], c["count"], c["mpp"], c["depth"], 8, 2 * (h + w))
    ref = want["centrelines"]
    assert ref[0, 0, F["thinning_passes"]] > 40 and ref[0, 0, F["stations"]] > n // 2 and ref[1, 0, F["stations"]] > 20
    _check(_abi(pkg, c, 2 * (h + w)), want, f"tiers, box {n}")


# ---------------------------------------------------------------------------------------------------------------- GPU, through the session
def _session(pkg, n, max_batch):
    model, neg = pkg.load_calibration(os.path.join(G, "calibration_phase_to_height.json"))
    fm = pkg.load_force_calibration(os.path.join(G, "calibration_height_to_force.json"))["best_model"]
    return pkg.FtpSensor(pkg.synth.reference_frame(n), pkg.synth.roi_circle(n), pkg.FtpConfig.scaled(n), model, neg, fm, max_batch=max_batch)


@pytest.mark.gpu
def test_session_centrelines_equal_the_reference_and_leave_the_predict_alone(pkg):
    import torch
    n, nb, K = 64, 4, 8
    s = _session(pkg, n, nb)
    with pytest.raises(RuntimeError):
        s.centrelines()                                      # no predict yet
    o = s.predict_batch(CH.multi_contact_batch(pkg, n, 0, nb))
    before = {k: v.clone() for k, v in o.items()}
    plain = {k: v.clone() for k, v in s.contacts(K, index_plane=True).items()}
    r = s.centrelines(K)
    first = s._centrelines
    again = s.centrelines(K)
    assert s._centrelines is first and s.centrelines(4)["centrelines"].shape == (nb, 4, 40) and s._centrelines is not first   # kept; remade for another K
    with pytest.raises(TypeError):
        s.centrelines(K, smoothing=3)
    torch.cuda.synchronize()
    assert set(r) == {"contacts", "count", "contact_index", "centrelines", "stations", "station_d2", "offsets", "skeleton"}
    assert tuple(r["stations"].shape) == (nb, 2 * (n + n), 2) and tuple(r["offsets"].shape) == (nb, K + 1)
    for k, v in before.items():
        assert torch.equal(o[k].view(torch.uint8), v.view(torch.uint8)), k
    for k, v in plain.items():
        assert torch.equal(r[k].view(torch.uint8), v.view(torch.uint8)), k
    assert _same_bits(r["centrelines"].cpu().numpy(), again["centrelines"].cpu().numpy())
    idx, tab, cnt = r["contact_index"].cpu().numpy(), r["contacts"].cpu().numpy(), r["count"].cpu().numpy()
    mpp, depth = o["scalars"][:, 6].cpu().numpy(), o["height_map_mm"].cpu().numpy()
    # the table agrees with contact_centrelines called by hand on the session's own planes, and with the reference
    by_hand = pkg.contact_centrelines(r["contact_index"], r["contacts"], r["count"], o["scalars"][:, 6].contiguous(), o["height_map_mm"])
    for k in ("centrelines", "offsets", "skeleton"):
        assert np.array_equal(by_hand[k].cpu().numpy().view(np.uint8), r[k].cpu().numpy().view(np.uint8)), k
    got = {"centrelines": r["centrelines"].cpu().numpy(), "offsets": r["offsets"].cpu().numpy(), "skeleton": r["skeleton"].cpu().numpy()}
    tail = np.arange(2 * (n + n))[None, :] >= got["offsets"][:, -1][:, None]
    got["stations"] = np.where(tail[..., None], SENTINEL, r["stations"].cpu().numpy())
    got["d2"] = np.where(tail, SENTINEL, r["station_d2"].cpu().numpy())
    s.close()
    assert s._centrelines is None
    _check(got, CL.reference(idx, tab, cnt, mpp, depth, 8, 2 * (n + n)), "session")
    out = got["centrelines"]
    used = ~np.isnan(out[..., 0])
    print("session counts", cnt, "stations", out[..., F["stations"]][used], "passes", out[..., F["thinning_passes"]][used])
    assert used.sum() == np.minimum(cnt, K).sum() >= 1
    assert np.array_equal(out[..., F["pixels"]][used], tab[..., 0][used])                    # VISTAF_CONTACT_PIXELS: the component itself
    assert (out[..., F["stations_written"]][used] == out[..., F["stations"]][used]).all() and not np.isnan(out[..., F["depth_mean_mm"]][used]).any()


@pytest.mark.gpu
def test_predict_centrelines_flag(pkg):
    n = 64
    s = _session(pkg, n, 1)
    frame = CH.multi_contact_frame(pkg, n, 2)
    plain, with_contacts = s.predict(frame), s.predict(frame, contacts=2)
    res = s.predict(frame, contacts=2, centrelines=True)
    assert set(res) == set(with_contacts) | {"centrelines", "centreline_stations", "centreline_d2"} and set(with_contacts) == set(plain) | {"contacts", "contact_count"}
    assert len(res["centrelines"]) == len(res["contacts"]) == len(res["centreline_stations"]) == len(res["centreline_d2"]) >= 1
    for cl, ct, line, d2 in zip(res["centrelines"], res["contacts"], res["centreline_stations"], res["centreline_d2"]):
        assert list(cl)[0] == "contact" and list(cl)[1:] == list(pkg.CENTRELINE_NAMES)
        assert cl["pixels"] == ct["pixels"] and len(line) == len(d2) == cl["stations"] == cl["stations_written"]
        assert line[0] == [cl["a_x"], cl["a_y"]] and line[-1] == [cl["b_x"], cl["b_y"]]
    wide = s.predict(frame, contacts=2, centrelines=dict(tangent_span=2, max_stations=0))
    assert wide["centreline_stations"] == [None] * len(wide["centrelines"]) and all(r["status"] & 16 for r in wide["centrelines"])
    assert np.array_equal(res["height_map_mm_crop"], plain["height_map_mm_crop"], equal_nan=True) and "centrelines" not in with_contacts
    with pytest.raises(ValueError):
        s.predict(frame, centrelines=True)
    s.close()
