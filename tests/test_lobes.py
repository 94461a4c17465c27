"""The lobe read-out (include_ext/vistaf_lobes.h): the depth maxima inside a contact, their prominence, the lobes and the split table.

The reference is tests/lobes_helpers.py: the ascent pixel by pixel, Kruskal over all passes with a plain union-find, the sums in row-major
order.  On the CPU: the properties of the lobes on random connected masks (8-connected, every pixel labelled, the chain of into() ends), the
known numbers of the bump fields, plateaus and the 2-pixel grid, the split table's rules, the header against `_lib`'s tables, the refusals of
the C ABI (they come before any HIP call) and the writers.  On the GPU every integer-valued field, both planes, parents, counts, peak and
saddle pixels and the fields that are single IEEE operations on samples must equal the reference exactly; the summed fields (float64 sums of
n positive terms in an order the definition leaves open) within 4 * n * 2^-52 relative, n the contact's pixel count, the split table's
volume with one float32 unit in the last place on top.  The largest deviation seen is printed."""
import csv
import ctypes
import os
import re

import numpy as np
import pytest

import contacts_helpers as CH
import lobes_helpers as LH
from abi_helpers import _hold_against, _prototypes
from abi_helpers import _same_f64_bits as _same_bits
from lobes_helpers import LF, RF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
HEADER = os.path.join(ROOT, "include_ext", "vistaf_lobes.h")
E_INVALID = -1
C_X0, C_X1 = 9, 11                  # VISTAF_CONTACT_BBOX_X0, _X1


# ------------------------------------------------------------------------------------------------------------------------------------ CPU
def _connected_masks(n, seed, top=14):
    """random 8-connected masks up to 13 x 13: the largest piece of a random plane"""
    rng = np.random.default_rng(seed)
    made = 0
    while made < n:
        h, w = rng.integers(1, top), rng.integers(1, top)
        m = rng.random((h, w)) < rng.uniform(0.45, 1.0)
        if not m.any():
            continue
        lab = -np.ones((h, w), int)
        pieces = []
        for y, x in zip(*np.nonzero(m)):
            if lab[y, x] >= 0:
                continue
            stack, piece = [(y, x)], []
            lab[y, x] = len(pieces)
            while stack:
                a, b = stack.pop()
                piece.append((a, b))
                for dx, dy in LH.NB8:
                    c, d = a + dy, b + dx
                    if 0 <= c < h and 0 <= d < w and m[c, d] and lab[c, d] < 0:
                        lab[c, d] = len(pieces)
                        stack.append((c, d))
            pieces.append(piece)
        best = max(pieces, key=len)
        out = np.zeros((h, w), bool)
        for p in best:
            out[p] = True
        made += 1
        yield out, rng


def test_lobes_are_connected_cover_the_mask_and_the_chain_ends_on_random_masks():
    n = 0
    for m, rng in _connected_masks(200, 0):
        for levels in (None, 4):
            d = rng.random(m.shape).astype(np.float32) if levels is None else (rng.integers(0, levels, m.shape) / np.float32(levels)).astype(np.float32)
            tau = float(rng.choice([0.0, 0.1, 0.3]))
            r = LH.lobes_of_mask(m, d, tau, 0.0)
            assert r["chain_ended"]
            assert ((r["lobe"] >= 0) == m).all()                                          # every pixel got a lobe
            for j, pk in enumerate(r["peaks"]):
                mine = r["lobe"] == j
                assert LH.components(mine, True) == 1, (m, d, j)
                ys, xs = np.nonzero(mine)
                assert max(zip(ys, xs), key=lambda p: (float(d[p]), -(p[0] * m.shape[1] + p[1]))) == pk      # a lobe's greatest pixel is its peak
            if levels is None and len(np.unique(d[m])) == m.sum():
                assert len(LH.lobes_of_mask(m, d, 0.0, 0.0)["peaks"]) == len(r["maxima"])      # tie-free depths: every maximum stands out at tau = 0
            one = LH.lobes_of_mask(m, d, 1.0e9, 0.0)
            assert len(one["peaks"]) == 1 and (one["lobe"][m] == 0).all()
            n += 1
    assert n == 400


def test_known_numbers_on_the_bump_fields():
    d, m = LH.two_bumps()
    r = LH.lobes_of_mask(m, d, 0.2, 0.0)
    assert r["maxima"] == [(12, 12), (11, 27)]
    assert [round(r["prominence"][p], 4) for p in r["maxima"]] == [1.0004, 0.4493]
    assert [int((r["lobe"] == j).sum()) for j in range(2)] == [185, 153] and len(r["peaks"]) == 2
    r = LH.lobes_of_mask(m, d, 0.5, 0.0)
    assert len(r["peaks"]) == 1 and int((r["lobe"] == 0).sum()) == 338 == int(m.sum())
    assert len(LH.lobes_of_mask(m, d, 0.0, 0.45)["peaks"]) == 1 and len(LH.lobes_of_mask(m, d, 0.0, 0.44)["peaks"]) == 2      # the fraction works alike
    d, m = LH.three_bumps()
    r = LH.lobes_of_mask(m, d, 0.2, 0.0)
    assert [round(r["prominence"][p], 4) for p in r["maxima"]] == [1.0006, 0.5037, 0.3692]
    assert [int((r["lobe"] == j).sum()) for j in range(3)] == [149, 136, 111]
    r = LH.lobes_of_mask(m, d, 0.45, 0.0)
    assert [int((r["lobe"] == j).sum()) for j in range(2)] == [149, 247] and len(r["peaks"]) == 2      # the third joins the middle one, not the deepest
    row, recs, plane, extra = LH.measure_mask(m, d, 0.1, 3.0, 2, 0.2, 0.0, 0.0)
    assert row[RF["peaks"]] == 3 and row[RF["peaks_written"]] == 2 and int(row[RF["status"]]) == LH.TRUNCATED and (plane == -2).sum() == 111
    assert row[RF["separation_mm"]] == 12 * 0.1 and recs[1, LF["neighbour"]] == 0 and recs[0, LF["neighbour"]] == -1 and np.isnan(recs[0, LF["saddle_x"]])
    assert row[RF["threshold_mm"]] == 0.2 and np.isnan(row[RF["next_prominence_mm"]]) and row[RF["deepest_saddle_mm"]] == recs[1, LF["saddle_depth_mm"]]
    row = LH.measure_mask(m, d, 0.1, 3.0, 4, 0.45, 0.0, 0.0)[0]
    assert round(row[RF["next_prominence_mm"]], 4) == 0.3692 and row[RF["peaks"]] == 2


def test_plateaus_and_many_maxima():
    flat = np.ones((24, 40), np.float32)
    for m in (LH.disc(24, 40, 12, 12, 6), LH.ring(24, 40, 12, 12, 6, 2)):
        r = LH.lobes_of_mask(m, flat, 0.0, 0.0)
        assert len(r["maxima"]) == 2 and len(r["peaks"]) == 1 and (r["lobe"][m] == 0).all()
    r = LH.lobes_of_mask(np.ones((24, 40), bool), LH.grid_depth(24, 40), 0.0, 0.0)
    assert len(r["maxima"]) == 240 and r["chain_ended"]


def test_split_table_rules_on_the_reference():
    names, c = LH.hand_made(24, 32)
    K = c["tab"].shape[1]
    ref = LH.reference(c["index"], c["tab"], c["count"], c["mpp"], c["depth"], 4, 0.05, 0.0, 0.01)
    rows, lobes, split, parent = ref["rows"], ref["lobes"], ref["split_contacts"], ref["split_parent"]
    for b, name in enumerate(names):
        kk = LH.clamp_count(c["count"][b], K)
        written = [int(rows[b, k, RF["peaks_written"]]) for k in range(kk)]
        assert ref["split_count"][b] == sum(written), name
        used = min(sum(written), K)
        assert np.isnan(split[b, used:]).all() and (parent[b, used:] == -1).all() and np.isnan(split[b, :used, 13:]).all()
        keys = [(-split[b, r, 4], split[b, r, 5]) for r in range(used)]
        assert keys == sorted(keys), name                                               # depth descending, ties by arg-max index ascending
        assert sorted(map(tuple, parent[b, :used])) == sorted(set(map(tuple, parent[b, :used])))
        for r in range(used):
            k, j = parent[b, r]
            assert split[b, r, 0] == lobes[b, k, j, LF["pixels"]] == (ref["split_index"][b] == r).sum()
            assert split[b, r, 4] == lobes[b, k, j, LF["depth_mm"]] and split[b, r, 5] == lobes[b, k, j, LF["y"]] * 32 + lobes[b, k, j, LF["x"]]
        for k in range(kk):                                                             # the shares of a contact add up to its force
            if rows[b, k, RF["peaks"]] == rows[b, k, RF["peaks_written"]] > 0 and not np.isnan(lobes[b, k, 0, LF["force_share_N"]]):
                assert abs(lobes[b, k, :written[k], LF["force_share_N"]].sum() - c["tab"][b, k, LH.C_FORCE]) <= 1e-12 * c["tab"][b, k, LH.C_FORCE]
    assert ref["split_count"][names.index("count_zero")] == 0 and (ref["split_index"][names.index("count_zero")] == -1).all()
    assert np.isnan(rows[names.index("count_zero")]).all() and np.isnan(lobes[names.index("count_zero")]).all()
    g = names.index("grid")
    assert rows[g, 0, RF["raw_maxima"]] == 12 * 16 and rows[g, 0, RF["peaks"]] == 192 and int(rows[g, 0, RF["status"]]) == LH.TRUNCATED
    assert ref["split_count"][g] == 4 and (ref["lobe_index"][g] == -2).sum() > 0 and ((ref["split_index"][g] >= 0) == (ref["lobe_index"][g] >= 0)).all()
    two = LH.reference(c["index"], c["tab"], c["count"], c["mpp"], c["depth"], 64, 0.0, 0.0, 0.01)      # more lobes than K rows: truncated at K
    assert two["split_count"][g] == 64 and two["rows"][g, 0, RF["peaks"]] == 192 and not np.isnan(two["split_contacts"][g, :, 0]).any() and two["split_index"][g].max() == K - 1
    assert ((two["split_index"][g] == -1) & (two["lobe_index"][g] >= 0)).any()
    e = names.index("clipped_pixel_empty")
    assert rows[e, 2, RF["pixels"]] == 1 and rows[e, 2, RF["peaks"]] == 1 and lobes[e, 2, 0, LF["pixels"]] == 1
    assert rows[e, 3, RF["status"]] == LH.NO_PIXELS and (rows[e, 3, :4] == 0).all() and np.isnan(lobes[e, 3]).all()
    assert rows[e, 4, RF["pixels"]] == 7 * 6                                                 # the box cuts its label
    assert rows[e, 5, RF["pixels"]] == 8 * 5 and rows[e, 0, RF["pixels"]] == 10 * 9            # clipped by the frame: the box leaves it, the contact lies in the corner
    q = names.index("nonfinite_subeps_badbox")
    assert (rows[q, 3:5, RF["status"]] == LH.NO_PIXELS).all() and lobes[q, 2, 0, LF["contact_pixels"]] == 0 and np.isnan(lobes[q, 2, 0, LF["centroid_x"]])
    p = names.index("plateau_and_ring")
    assert rows[p, 0, RF["raw_maxima"]] == 2 and rows[p, 0, RF["peaks"]] == 1 and rows[p, 0, RF["next_prominence_mm"]] == 0.0


def test_lobe_names_and_signatures_follow_the_header(pkg):
    hdr = open(HEADER).read()
    idx = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define VISTAF_LOBE_(\w+)\s+(\d+)\b", hdr)}
    assert sorted(idx.values()) == list(range(16))
    for name, i in idx.items():
        assert pkg.LOBE_NAMES[i].lower() == name
    ridx = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define VISTAF_LOBEROW_(\w+)\s+(\d+)\b", hdr)}
    assert sorted(ridx.values()) == list(range(9))
    for name, i in ridx.items():
        assert pkg.LOBE_ROW_NAMES[i] == name
    assert list(pkg.LOBE_NAMES) == list(pkg._lib.LOBE_NAMES) == list(pkg.writers.LOBE_FIELDS) == list(LH.LOBE_FIELDS)
    assert list(pkg.LOBE_ROW_NAMES) == list(pkg._lib.LOBE_ROW_NAMES) == list(pkg.writers.LOBE_ROW_FIELDS) == list(LH.ROW_FIELDS)
    assert int(re.search(r"#define VISTAF_NLOBE\s+(\d+)", hdr).group(1)) == pkg._lib.NLOBE == LH.NLOBE == 16
    assert int(re.search(r"#define VISTAF_NLOBEROW\s+(\d+)", hdr).group(1)) == pkg._lib.NLOBEROW == LH.NLOBEROW == 12
    assert int(re.search(r"#define VISTAF_LOBES_MAX\s+(\d+)", hdr).group(1)) == pkg._lib.LOBES_MAX == 64
    status = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define VISTAF_LOBEST_(\w+)\s+(\d+)\b", hdr)}
    assert status == pkg.LOBE_STATUS == {"ok": LH.OK, "no_pixels": LH.NO_PIXELS, "truncated": LH.TRUNCATED}
    assert "DIFFERS FROM THE CONTACTS TABLE" in hdr and "0.02" in hdr and "0.10" in hdr
    assert (pkg.lobes.DEFAULT_MIN_PROMINENCE_MM, pkg.lobes.DEFAULT_MIN_PROMINENCE_FRAC) == (0.02, 0.10)
    for name in ("lobes", "LOBE_NAMES", "LOBE_ROW_NAMES", "LOBE_STATUS", "contact_lobes", "LobesWorkspace", "lobes_table", "write_lobes_csv", "lobe_frame_record"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    for name in ("contact_lobes", "LobesWorkspace", "workspace_bytes", "trim"):
        assert hasattr(pkg.lobes, name)
    assert hasattr(pkg.FtpSensor, "lobes")
    lib = pkg._lib.load()
    table = pkg._lib.LOBES_SIGNATURES
    _hold_against(_prototypes(hdr), table, lib)
    assert sorted(table) == ["vistaf_lobes_measure", "vistaf_lobes_workspace_bytes"]
    assert not set(table) & {n for g in pkg._lib.SIGNATURES.values() for n in g}
    hooks = open(os.path.join(os.path.dirname(pkg.__file__), "csrc", "test_hooks_lobes.h")).read()
    _hold_against(_prototypes(hooks), pkg._lib.LOBES_TEST_SIGNATURES, lib)
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other.endswith(".h"):
            assert "vistaf_lobes" not in open(os.path.join(ROOT, "include", other)).read(), other


def test_lobes_tier_hook_is_monotone_and_refuses(pkg):
    tier = pkg._lib.load().vistaf_ftp_test_lobes_tier
    assert tier(1, 1) == 1 and tier(32, 32) == 1 and tier(48, 48) == 1 and tier(224, 224) == 0 and tier(32767, 32767) == 0
    last = 1
    for n in range(1, 200):
        t = tier(n, n)
        assert t in (0, 1) and t <= last
        last = t
    assert last == 0
    for bad in ((0, 8), (8, 0), (32768, 8), (8, 32768)):
        assert tier(*bad) == E_INVALID


def test_lobes_c_abi_refuses_with_the_arguments_name(pkg):
    lib = pkg._lib.load()
    err = lib.vistaf_ftp_last_error
    n = ctypes.c_size_t(1)
    assert lib.vistaf_lobes_workspace_bytes(8, 8, 1, 8, None) == E_INVALID and b"bytes" in err()
    for args, word in (((0, 8, 1, 8), b"h "), ((32768, 8, 1, 8), b"h "), ((8, 0, 1, 8), b"w "), ((8, 32768, 1, 8), b"w "),
                       ((32767, 32767, 1, 8), b"h * w"), ((8, 8, 0, 8), b"batch"), ((8, 8, 1, 0), b"max_contacts"), ((8, 8, 1, 65), b"max_contacts")):
        n.value = 1
        assert lib.vistaf_lobes_workspace_bytes(*args, ctypes.byref(n)) == E_INVALID and n.value == 0 and word in err(), args
    assert lib.vistaf_lobes_workspace_bytes(8, 8, 1, 8, ctypes.byref(n)) == 0 and n.value > 0
    assert pkg.lobes.workspace_bytes(8, 8, 1, 8) == n.value
    assert pkg.lobes.workspace_bytes(48, 48, 2, 8) < pkg.lobes.workspace_bytes(64, 64, 2, 8) // 2          # no row tables while every box fits LDS
    with pytest.raises(ValueError, match="max_contacts"):
        pkg.lobes.workspace_bytes(8, 8, 1, 0)
    # measure: host memory stands in for the device's, every call is refused before any HIP call
    f64, i32, i8, f32 = (ctypes.c_double * 1024)(), (ctypes.c_int32 * 64)(), (ctypes.c_int8 * 64)(), (ctypes.c_float * 64)()
    raw = (ctypes.c_uint8 * (n.value + 512))()
    ws = (ctypes.addressof(raw) + 255) & ~255
    p = ctypes.addressof
    good = dict(idx=p(i8), tab=p(f64), cnt=p(i32), mpp=p(f64), dep=p(f32), B=1, h=8, w=8, K=8, L=4, pmm=0.02, pfrac=0.1, eps=0.01, lobes=p(f64), rows=p(f64),
                lidx=p(i8), split=p(f64), scount=p(i32), sidx=p(i8), parent=p(i32), ws=ws, n=n.value)

    def call(**kw):
        a = dict(good, **kw)
        return lib.vistaf_lobes_measure(a["idx"], a["tab"], a["cnt"], a["mpp"], a["dep"], a["B"], a["h"], a["w"], a["K"], a["L"], a["pmm"], a["pfrac"], a["eps"],
                                        a["lobes"], a["rows"], a["lidx"], a["split"], a["scount"], a["sidx"], a["parent"], a["ws"], a["n"], None)
    nan, inf = float("nan"), float("inf")
    for kw, words in ((dict(idx=None), [b"d_contact_index"]), (dict(tab=None), [b"d_contacts"]), (dict(cnt=None), [b"d_count"]),
                      (dict(mpp=None), [b"d_mm_per_px"]), (dict(dep=None), [b"d_depth_mm"]), (dict(lobes=None), [b"d_lobes"]), (dict(rows=None), [b"d_rows"]),
                      (dict(ws=None), [b"d_workspace"]), (dict(split=None), [b"d_split_contacts", b"all"]), (dict(scount=None), [b"d_split_count"]),
                      (dict(sidx=None), [b"d_split_index"]), (dict(parent=None), [b"d_split_parent"]),
                      (dict(split=None, scount=None, sidx=None), [b"d_split_parent"]), (dict(h=0), [b"h "]), (dict(w=32768), [b"w "]), (dict(B=0), [b"batch"]),
                      (dict(K=0), [b"max_contacts"]), (dict(K=65), [b"max_contacts"]), (dict(L=0), [b"max_lobes"]), (dict(L=65), [b"max_lobes"]),
                      (dict(pmm=-0.1), [b"min_prominence_mm"]), (dict(pmm=nan), [b"min_prominence_mm"]), (dict(pmm=inf), [b"min_prominence_mm"]),
                      (dict(pfrac=-0.1), [b"min_prominence_frac"]), (dict(pfrac=nan), [b"min_prominence_frac"]), (dict(eps=-1e-9), [b"depth_eps_mm"]),
                      (dict(eps=inf), [b"depth_eps_mm"]),
                      (dict(tab=p(f64) + 4), [b"d_contacts", b"aligned"]), (dict(cnt=p(i32) + 2), [b"d_count", b"aligned"]),
                      (dict(dep=p(f32) + 2), [b"d_depth_mm", b"aligned"]), (dict(parent=p(i32) + 1), [b"d_split_parent", b"aligned"]),
                      (dict(ws=ws + 128), [b"d_workspace", b"aligned"]), (dict(n=n.value - 1), [b"workspace_bytes"]), (dict(n=0), [b"workspace_bytes"])):
        assert call(**kw) == E_INVALID, kw
        assert all(word in err() for word in words), (kw, err())


def test_lobe_writers_round_trip(pkg, tmp_path):
    d, m = LH.three_bumps()
    sc = LH.Scene(24, 40).paint(0, m)
    one = np.zeros((24, 40), bool)
    sc.paint(1, one, box=[1, 1, 3, 3])
    c = LH.pack([sc], 0.1)
    c["tab"][0, :2, LH.C_FORCE] = [3.0, 1.0]
    ref = LH.reference(c["index"], c["tab"], c["count"], c["mpp"], d[None], 2, 0.2, 0.0, 0.0)
    rows = pkg.lobes_table(ref["lobes"], ref["rows"], c["count"])
    assert [(r["frame"], r["contact"], r["lobe"]) for r in rows] == [(0, 0, 0), (0, 0, 1)]
    assert list(rows[0])[3:] == list(pkg.LOBE_NAMES) and isinstance(rows[0]["pixels"], int) and isinstance(rows[0]["depth_mm"], float)
    assert rows[0]["neighbour"] == -1 and rows[0]["saddle_x"] == -1 and np.isnan(rows[0]["saddle_depth_mm"]) and rows[1]["neighbour"] == 0
    assert (rows[0]["x"], rows[0]["y"], rows[0]["pixels"], rows[1]["pixels"]) == (8, 12, 149, 136)
    with pytest.raises(ValueError):
        pkg.lobes_table(ref["lobes"][..., :8], ref["rows"], c["count"])
    path = pkg.write_lobes_csv(str(tmp_path), ref["lobes"], ref["rows"], c["count"])
    back = list(csv.DictReader(open(path)))
    assert len(back) == 2 and list(back[0]) == ["frame", "contact", "lobe"] + list(pkg.LOBE_NAMES)
    for r, q in zip(rows, back):
        for name in pkg.LOBE_NAMES:
            v = float(q[name])
            assert v == r[name] or (np.isnan(v) and np.isnan(r[name]))
    rec = pkg.lobe_frame_record(ref["lobes"][0], ref["rows"][0], 2, ref["split_contacts"][0], ref["split_count"][0], ref["split_parent"][0])
    assert rec["contact_count"] == 2 and [len(v) for v in rec["lobes"]] == [2, 0] and rec["lobes"][0][0]["saddle_depth_mm"] is None
    assert rec["lobe_rows"][0]["peaks"] == 3 and rec["lobe_rows"][0]["status"] == 16 and rec["lobe_rows"][1]["status"] == 1 and rec["lobe_rows"][1]["threshold_mm"] is None
    assert rec["split_count"] == 2 and [r["parent"] for r in rec["split_contacts"]] == [[0, 0], [0, 1]] and "frame" not in rec["split_contacts"][0]
    assert rec["split_contacts"][0]["pixels"] == 149 and 2.0 < rec["split_contacts"][0]["force_N"] + rec["split_contacts"][1]["force_N"] < 3.0      # the third lobe's share was not written
    assert "split_contacts" not in pkg.lobe_frame_record(ref["lobes"][0], ref["rows"][0], 2)
    with pytest.raises(ValueError):
        pkg.lobe_frame_record(ref["lobes"], ref["rows"], 2)


def test_contact_lobes_needs_a_device_or_refuses_bad_arguments(pkg):
    import torch
    idx, tab, dep = np.zeros((1, 8, 8), np.int8), np.zeros((1, 4, 16)), np.zeros((1, 8, 8), np.float32)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):
            pkg.contact_lobes(idx, tab, [1], [0.1], dep)
        return
    for bad in ((idx[0], tab, [1], [0.1], dep), (idx, tab[:, :, :8], [1], [0.1], dep), (idx, tab, [1, 2], [0.1], dep), (idx, tab, [1], [0.1, 0.2], dep),
                (idx, tab, [1], [0.1], np.zeros((1, 8, 9), np.float32)), (idx, tab, [1], [0.1], None)):
        with pytest.raises(ValueError):
            pkg.contact_lobes(*bad)
    for kw in (dict(max_lobes=0), dict(max_lobes=65), dict(min_prominence_mm=-1.0), dict(min_prominence_frac=float("nan")), dict(depth_eps_mm=-1.0)):
        with pytest.raises(ValueError):
            pkg.contact_lobes(idx, tab, [1], [0.1], dep, **kw)


# ------------------------------------------------------------------------------------------------------------- GPU, through the C ABI
SENTINEL = -77
WORST = {"lobes": 0.0, "split": 0.0}


def _abi(pkg, c, L, tau_mm, tau_frac, eps, lobe_index=True, split=True, sel=None):
    """vistaf_lobes_measure on case c (frames `sel`): dict of arrays; every output is filled with a sentinel first; d_lobe_index is NULL with
    lobe_index=False, the split set with split=False"""
    import torch
    sel = slice(None) if sel is None else sel
    dev = torch.device("cuda:0")
    idx, tab = torch.as_tensor(c["index"][sel]).to(dev).contiguous(), torch.as_tensor(c["tab"][sel]).to(dev).contiguous()
    cnt, mpp = torch.as_tensor(c["count"][sel]).to(dev).contiguous(), torch.as_tensor(c["mpp"][sel]).to(dev).contiguous()
    dep = torch.as_tensor(c["depth"][sel]).to(dev).contiguous()
    B, h, w = idx.shape
    K = tab.shape[1]
    nbytes = pkg.lobes.workspace_bytes(h, w, B, K)
    ws = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device=dev)
    lobes = torch.full((B, K, L, 16), 123.0, dtype=torch.float64, device=dev)
    rows = torch.full((B, K, 12), 123.0, dtype=torch.float64, device=dev)
    lidx = torch.full((B, h, w), SENTINEL, dtype=torch.int8, device=dev)
    sp = torch.full((B, K, 16), 123.0, dtype=torch.float64, device=dev)
    scnt = torch.full((B,), SENTINEL, dtype=torch.int32, device=dev)
    sidx = torch.full((B, h, w), SENTINEL, dtype=torch.int8, device=dev)
    par = torch.full((B, K, 2), SENTINEL, dtype=torch.int32, device=dev)
    pkg._handle.call(dev, "vistaf_lobes_measure", idx.data_ptr(), tab.data_ptr(), cnt.data_ptr(), mpp.data_ptr(), dep.data_ptr(), B, h, w, K, L,
                     float(tau_mm), float(tau_frac), float(eps), lobes.data_ptr(), rows.data_ptr(), lidx.data_ptr() if lobe_index else None,
                     sp.data_ptr() if split else None, scnt.data_ptr() if split else None, sidx.data_ptr() if split else None,
                     par.data_ptr() if split else None, (ws.data_ptr() + 255) & ~255, nbytes, pkg._handle.stream(dev))
    torch.cuda.synchronize()
    return {"lobes": lobes.cpu().numpy(), "rows": rows.cpu().numpy(), "lobe_index": lidx.cpu().numpy(), "split_contacts": sp.cpu().numpy(),
            "split_count": scnt.cpu().numpy(), "split_index": sidx.cpu().numpy(), "split_parent": par.cpu().numpy()}


def _within(got, ref, rel, what, bucket):
    """NaN in the same places and |got - ref| <= rel * |ref| elsewhere (rel broadcasts); records the largest deviation in units of 2^-52"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    rel = np.broadcast_to(np.asarray(rel, np.float64), ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, got, ref)
    ok = ~np.isnan(ref)
    dev = np.abs(got[ok] - ref[ok])
    scale = np.abs(ref[ok])
    with np.errstate(divide="ignore", invalid="ignore"):
        units = np.where(dev == 0, 0.0, dev / scale) / 2.0 ** -52
    if units.size:
        WORST[bucket] = max(WORST[bucket], float(units.max()))
    assert (dev <= rel[ok] * scale).all(), (what, got[ok][dev > rel[ok] * scale], ref[ok][dev > rel[ok] * scale])


def _check(got, want, what, lobe_index=True, split=True):
    """exact fields bit for bit; the summed fields within 4 * n * 2^-52 relative, n the pixel count of the contact"""
    rows, ref_rows = got["rows"], want["rows"]
    for i, name in enumerate(LH.ROW_FIELDS):
        assert _same_bits(rows[..., i], ref_rows[..., i]), (what, name, rows[..., i], ref_rows[..., i])
    assert np.isnan(rows[..., len(LH.ROW_FIELDS):]).all(), (what, "reserved fields")
    n = np.nan_to_num(ref_rows[..., RF["pixels"]])[..., None]                          # [B,K,1]
    for i, name in enumerate(LH.LOBE_FIELDS):
        if name in LH.LOBE_SUMMED:
            _within(got["lobes"][..., i], want["lobes"][..., i], 4.0 * n * 2.0 ** -52, (what, name), "lobes")
        else:
            assert _same_bits(got["lobes"][..., i], want["lobes"][..., i]), (what, name, got["lobes"][..., i], want["lobes"][..., i])
    assert np.array_equal(got["lobe_index"], want["lobe_index"]) if lobe_index else (got["lobe_index"] == SENTINEL).all(), what
    if not split:
        assert (got["split_contacts"] == 123.0).all() and (got["split_count"] == SENTINEL).all() and (got["split_index"] == SENTINEL).all()
        assert (got["split_parent"] == SENTINEL).all()
        return
    assert np.array_equal(got["split_count"], want["split_count"]) and np.array_equal(got["split_parent"], want["split_parent"]), what
    assert np.array_equal(got["split_index"], want["split_index"]), what
    pn = want["pixels"]
    for i in range(16):
        if i in LH.SPLIT_SUMMED:
            rel = 4.0 * pn * 2.0 ** -52 + (2.0 ** -23 if i == 3 else 0.0)
            _within(got["split_contacts"][..., i], want["split_contacts"][..., i], rel, (what, "split", i), "split")
        else:
            assert _same_bits(got["split_contacts"][..., i], want["split_contacts"][..., i]), (what, "split", i)


_REF = {}
HAND = dict(L=4, tau_mm=0.05, tau_frac=0.0, eps=0.01)


def _hand_case(h, w):
    if (h, w) not in _REF:
        names, c = LH.hand_made(h, w)
        _REF[(h, w)] = (names, c, LH.reference(c["index"], c["tab"], c["count"], c["mpp"], c["depth"], HAND["L"], HAND["tau_mm"], HAND["tau_frac"], HAND["eps"]))
    return _REF[(h, w)]


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", [(24, 32), (37, 53)])
def test_hand_made_cases_equal_the_reference(pkg, h, w):
    names, c, want = _hand_case(h, w)
    rows = want["rows"]
    assert rows[names.index("two_bumps"), 0, RF["peaks"]] == 2 and rows[names.index("three_bumps"), 0, RF["peaks"]] == 3
    assert rows[names.index("grid"), 0, RF["raw_maxima"]] == ((h + 1) // 2) * ((w + 1) // 2)
    assert rows[names.index("count_above_K"), :2, RF["peaks"]].min() >= 2
    _check(_abi(pkg, c, **HAND), want, f"hand-made {h}x{w}")
    print("largest deviation of a summed field, units of 2^-52:", WORST)


def _batch_case():
    if "batch" not in _REF:
        h, w = 64, 96
        scenes, depths = [], []
        for b in range(3):
            d = (LH.bumps(h, w, [(1.0, 14 + b, 16), (0.8, 30 + b, 18), (0.55, 46, 14 + b), (0.9, 70, 40), (0.6, 82 - b, 46), (0.7, 20, 48)], 40.0 + 6 * b)
                 + 0.01 * LH.periodic_depth(h, w, b))
            sc = LH.Scene(h, w)
            sc.paint(0, LH.rect(h, w, 2, 2, 60, 30) & (d > 0.3)).paint(1, LH.rect(h, w, 55, 25, 95, 63) & ~LH.rect(h, w, 2, 2, 60, 30) & (d > 0.3))
            sc.paint(2, LH.disc(h, w, 20, 48, 9))
            scenes.append(sc)
            depths.append(d.astype(np.float32))
        c = LH.pack(scenes, [0.05, 0.0731, 0.1])
        c["depth"] = np.stack(depths)
        c["tab"][..., LH.C_FORCE] = np.where(np.isnan(c["tab"][..., 0]), np.nan, 1.0 + 0.37 * np.arange(8)[None, :] + 0.11 * np.arange(3)[:, None])
        _REF["batch"] = c
    return _REF["batch"]


def _batch_ref(L):
    if ("batch", L) not in _REF:
        c = _batch_case()
        _REF[("batch", L)] = LH.reference(c["index"], c["tab"], c["count"], c["mpp"], c["depth"], L, 0.05, 0.1, 0.01)
    return _REF[("batch", L)]


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 2, 4])
def test_batch_with_truncation_and_null_outputs(pkg, L):
    c, want = _batch_case(), _batch_ref(L)
    rows = want["rows"]
    assert rows[0, 0, RF["peaks"]] == 3 and rows[0, 1, RF["peaks"]] == 2 and rows[0, 2, RF["peaks"]] == 1
    if L < 3:
        assert int(rows[0, 0, RF["status"]]) & LH.TRUNCATED and (want["lobe_index"] == -2).any()
    else:
        assert not (rows[..., RF["status"]][~np.isnan(rows[..., 0])].astype(int) & LH.TRUNCATED).any() and not (want["lobe_index"] == -2).any()
    _check(_abi(pkg, c, L, 0.05, 0.1, 0.01), want, f"batch L={L}")
    _check(_abi(pkg, c, L, 0.05, 0.1, 0.01, lobe_index=False), want, f"batch L={L} NULL lobe_index", lobe_index=False)
    _check(_abi(pkg, c, L, 0.05, 0.1, 0.01, split=False), want, f"batch L={L} NULL split", split=False)
    print("largest deviation of a summed field, units of 2^-52:", WORST)


@pytest.mark.gpu
def test_batch_positions_and_second_call_give_the_same_bits(pkg):
    import torch
    c = _batch_case()
    keys = ("lobes", "rows", "lobe_index", "split_contacts", "split_count", "split_index", "split_parent")
    args = (4, 0.05, 0.1, 0.01)
    whole, again = _abi(pkg, c, *args), _abi(pkg, c, *args)
    for k in keys:
        assert np.array_equal(whole[k].view(np.uint8), again[k].view(np.uint8)), k
    for i in range(3):
        one = _abi(pkg, c, *args, sel=slice(i, i + 1))
        for k in keys:
            assert np.array_equal(one[k].view(np.uint8), whole[k][i:i + 1].view(np.uint8)), (i, k)
    perm = [2, 0, 1]
    moved = _abi(pkg, {k: (v[perm] if isinstance(v, np.ndarray) else v) for k, v in c.items()}, *args)
    for k in keys:
        assert np.array_equal(moved[k].view(np.uint8), whole[k][perm].view(np.uint8)), k
    # the Python entry point: the same bits, the dict's keys, trim
    r = pkg.contact_lobes(c["index"], c["tab"], c["count"], c["mpp"], c["depth"], 4, 0.05, 0.1, 0.01)
    torch.cuda.synchronize()
    assert set(r) == {"lobes", "lobe_rows", "lobe_index", "split_contacts", "split_count", "split_index", "split_parent"}
    for k in keys:
        assert np.array_equal(r["lobe_rows" if k == "rows" else k].cpu().numpy().view(np.uint8), whole[k].view(np.uint8)), k
    t = pkg.lobes.trim(r)
    assert not t["overflow"] and [len(v) for v in t["lobes"][0]] == [3, 2, 1] and t["lobes"][0][0].shape == (3, 16)
    small = pkg.contact_lobes(c["index"], c["tab"], c["count"], c["mpp"], c["depth"], 1, 0.05, 0.1, 0.01, split=False, lobe_index=False)
    assert set(small) == {"lobes", "lobe_rows"} and pkg.lobes.trim(small)["overflow"]


@pytest.mark.gpu
def test_both_storage_tiers_equal_the_reference(pkg):
    tier = pkg._lib.load().vistaf_ftp_test_lobes_tier
    n = next(v for v in range(9, 2000) if tier(v, v) == 0)                        # the smallest square box that leaves LDS
    assert tier(n - 1, n - 1) == 1 and tier(n, n) == 0
    h = w = n + 6
    big = LH.rect(h, w, 3, 2, 3 + n - 1, 2 + n - 1) & ~LH.rect(h, w, 3 + n // 2 - 8, 2, 3 + n // 2 + 7, 2 + n // 3)      # a full square with a notch
    small = LH.rect(h, w, 3, 4, 3 + n - 2, 4 + n - 2) & ~LH.rect(h, w, 20, 4, 27, 20)                                # one pixel smaller: the LDS tier
    c = LH.pack([LH.Scene(h, w).paint(0, big), LH.Scene(h, w).paint(0, small)], 0.05)
    assert [int(c["tab"][b, 0, C_X1] - c["tab"][b, 0, C_X0] + 1) for b in range(2)] == [n, n - 1]
    c["depth"] = np.stack([LH.periodic_depth(h, w, b) for b in range(2)])
    c["tab"][:, 0, LH.C_FORCE] = [2.5, 1.5]
    want = LH.reference(c["index"], c["tab"], c["count"], c["mpp"], c["depth"], 64, 0.015, 0.0, 0.0)
    rows = want["rows"]
    assert (rows[:, 0, RF["raw_maxima"]] > 60).all() and (rows[:, 0, RF["peaks"]] > 8).all() and (rows[:, 0, RF["raw_maxima"]] > rows[:, 0, RF["peaks"]]).all()
    _check(_abi(pkg, c, 64, 0.015, 0.0, 0.0), want, f"tiers, box {n}")
    print("largest deviation of a summed field, units of 2^-52:", WORST)


# ---------------------------------------------------------------------------------------------------------------- GPU, through the session
def _session(pkg, n, max_batch):
    model, neg = pkg.load_calibration(os.path.join(G, "calibration_phase_to_height.json"))
    fm = pkg.load_force_calibration(os.path.join(G, "calibration_height_to_force.json"))["best_model"]
    return pkg.FtpSensor(pkg.synth.reference_frame(n), pkg.synth.roi_circle(n), pkg.FtpConfig.scaled(n), model, neg, fm, max_batch=max_batch)


@pytest.mark.gpu
def test_session_lobes_equal_the_reference_and_feed_the_other_readouts(pkg):
    import torch
    n, nb, K, L = 64, 4, 8, 4
    s = _session(pkg, n, nb)
    with pytest.raises(RuntimeError):
        s.lobes()                                            # no predict yet
    o = s.predict_batch(CH.multi_contact_batch(pkg, n, 0, nb))
    before = {k: v.clone() for k, v in o.items()}
    plain = {k: v.clone() for k, v in s.contacts(K, index_plane=True).items()}
    r = s.lobes(K, L, min_prominence_mm=0.0, min_prominence_frac=0.02)
    first = s._lobes
    again = s.lobes(K, L, min_prominence_mm=0.0, min_prominence_frac=0.02)
    assert s._lobes is first and s.lobes(4)["lobes"].shape == (nb, 4, 4, 16) and s._lobes is not first      # kept; remade for another K
    assert set(s.lobes(K, split=False)) == {"contacts", "count", "contact_index", "lobes", "lobe_rows", "lobe_index"}
    torch.cuda.synchronize()
    assert set(r) == {"contacts", "count", "contact_index", "lobes", "lobe_rows", "lobe_index", "split_contacts", "split_count", "split_index", "split_parent"}
    for k, v in before.items():
        assert torch.equal(o[k].view(torch.uint8), v.view(torch.uint8)), k
    for k, v in plain.items():
        assert torch.equal(r[k].view(torch.uint8), v.view(torch.uint8)), k
    keys = ("lobes", "lobe_rows", "lobe_index", "split_contacts", "split_count", "split_index", "split_parent")
    for k in keys:
        assert np.array_equal(r[k].cpu().numpy().view(np.uint8), again[k].cpu().numpy().view(np.uint8)), k
    eps = s.config.depth_eps_mm
    by_hand = pkg.contact_lobes(r["contact_index"], r["contacts"], r["count"], o["scalars"][:, 6].contiguous(), o["height_map_mm"], L, 0.0, 0.02, eps)
    for k in keys:
        assert np.array_equal(by_hand[k].cpu().numpy().view(np.uint8), r[k].cpu().numpy().view(np.uint8)), k
    idx, tab, cnt = r["contact_index"].cpu().numpy(), r["contacts"].cpu().numpy(), r["count"].cpu().numpy()
    mpp, depth = o["scalars"][:, 6].cpu().numpy(), o["height_map_mm"].cpu().numpy()
    got = {("rows" if k == "lobe_rows" else k): r[k].cpu().numpy() for k in keys}
    # the split triple is a contacts table: the tracker and the centreline read-out take it unchanged and give one row per written lobe
    written = np.minimum(got["split_count"], K)
    tracker = pkg.ContactTracker(n, n, nb, K)
    tr = tracker.update(r["split_index"], r["split_contacts"], r["split_count"])["tracks"].cpu().numpy()
    tracker.close()
    cl = pkg.contact_centrelines(r["split_index"], r["split_contacts"], r["split_count"], o["scalars"][:, 6].contiguous(), o["height_map_mm"])
    cl = cl["centrelines"].cpu().numpy()
    s.close()
    assert s._lobes is None
    for b in range(nb):
        assert (~np.isnan(tr[b, :, 0])).sum() == written[b] == (~np.isnan(cl[b, :, 0])).sum(), b
        assert np.array_equal(cl[b, :written[b], 0], got["split_contacts"][b, :written[b], 0])              # PIXELS of the lobe, counted again by the centreline kernel
    _check(got, LH.reference(idx, tab, cnt, mpp, depth, L, 0.0, 0.02, eps), "session")
    rows = got["rows"]
    used = ~np.isnan(rows[..., 0])
    print("session counts", cnt, "raw maxima", rows[..., RF["raw_maxima"]][used], "peaks", rows[..., RF["peaks"]][used], "split", got["split_count"])
    print("largest deviation of a summed field, units of 2^-52:", WORST)
    assert used.sum() == np.minimum(cnt, K).sum() >= 1 and (got["split_count"] >= np.minimum(cnt, K)).all()
    assert np.array_equal(rows[..., RF["pixels"]][used], tab[..., 0][used])                    # VISTAF_CONTACT_PIXELS: the component itself


@pytest.mark.gpu
def test_predict_lobes_flag(pkg):
    n = 64
    s = _session(pkg, n, 1)
    frame = CH.multi_contact_frame(pkg, n, 2)
    plain, with_contacts = s.predict(frame), s.predict(frame, contacts=2)
    res = s.predict(frame, contacts=2, lobes=True)
    assert set(res) == set(with_contacts) | {"lobes", "lobe_rows", "split_contacts"} and set(with_contacts) == set(plain) | {"contacts", "contact_count"}
    assert len(res["lobes"]) == len(res["contacts"]) == len(res["lobe_rows"]) >= 1
    for lobes, row, ct in zip(res["lobes"], res["lobe_rows"], res["contacts"]):
        assert list(row) == list(pkg.LOBE_ROW_NAMES) and row["pixels"] == ct["pixels"] and len(lobes) == row["peaks_written"] >= 1
        assert list(lobes[0]) == ["lobe"] + list(pkg.LOBE_NAMES) and lobes[0]["depth_mm"] == ct["max_depth_mm"]
        assert sum(v["pixels"] for v in lobes) == ct["pixels"] or row["status"] & 16
    assert len(res["split_contacts"]) == min(2, sum(r["peaks_written"] for r in res["lobe_rows"]))
    assert all(r["parent"][0] in (0, 1) for r in res["split_contacts"])
    fine = s.predict(frame, contacts=2, lobes=dict(max_lobes=1, min_prominence_mm=0.0, min_prominence_frac=0.0))
    assert all(len(v) == 1 for v in fine["lobes"]) and all(r["peaks"] >= 1 for r in fine["lobe_rows"])
    assert np.array_equal(res["height_map_mm_crop"], plain["height_map_mm_crop"], equal_nan=True) and "lobes" not in with_contacts
    with pytest.raises(ValueError):
        s.predict(frame, lobes=True)
    s.close()
