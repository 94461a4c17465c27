"""Contact tracker (include/vistaf_track.h, ContactTracker, FtpSensor.track): persistent ids, motion, split and merge across frames.

The definition is restated in NumPy in tests/tracks_helpers.py (`numpy_tracks`).  The direct GPU tests hand the tracker hand-made int8 planes
and tables (no FTP session) and ask for equality of every field with that restatement: the same bits wherever a value is not NaN, NaN in
the same places.  The base shape is 37 x 53: P = 1961 is odd, so every frame's plane starts at another misalignment.  The session tests run
the tracker behind `FtpSensor.track` on a scene of two moving bumps.
"""
import csv
import ctypes
import os
import re

import numpy as np
import pytest

import contacts_helpers as CH
import tracks_helpers as TH
from tracks_helpers import T, BORN, SPLIT, MERGED, GATED, NO_ROW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
H, W = 37, 53


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_track_names_and_events_follow_the_header(pkg):
    hdr = open(os.path.join(ROOT, "include", "vistaf_track.h")).read()
    idx = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define VISTAF_TRACK_(\w+)\s+(\d+)\b", hdr)}
    expect = {"ID": "track_id", "AGE_FRAMES": "age_frames", "PARENT_ROW": "parent_row", "EVENTS": "events", "OVERLAP_PX": "overlap_px",
              "DX": "dx", "DY": "dy", "DFORCE_N": "dforce_N", "DVOLUME_CM3": "dvolume_cm3", "ORIGIN_TRACK_ID": "origin_track_id"}
    assert sorted(idx) == sorted(expect)
    assert sorted(idx.values()) == list(range(10))
    for cname, i in idx.items():
        assert pkg.TRACK_NAMES[i] == expect[cname]
    assert list(pkg.TRACK_NAMES) == list(pkg._lib.TRACK_NAMES) == list(pkg.writers.TRACK_FIELDS) == list(TH.FIELDS)
    ev = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define VISTAF_TRACKEV_(\w+)\s+(\d+)\b", hdr)}
    assert ev == pkg.TRACK_EVENTS == pkg._lib.TRACK_EVENTS == {"born": BORN, "split": SPLIT, "merged": MERGED, "gated": GATED}
    assert int(re.search(r"#define VISTAF_NTRACK\s+(\d+)", hdr).group(1)) == pkg._lib.NTRACK == TH.NTRACK == 16
    assert "VISTAF_FRAME_OK" in hdr and "ends every track" in hdr                   # the rule for empty / failed frames is stated


def test_library_exports_every_declared_track_symbol(pkg):
    hdr = open(os.path.join(ROOT, "include", "vistaf_track.h")).read()
    declared = sorted(set(re.findall(r"\b(vistaf_track_\w+)\s*\(", hdr)))
    assert declared == sorted(["vistaf_track_create", "vistaf_track_update", "vistaf_track_reset", "vistaf_track_destroy"])
    lib = pkg._lib.load()
    for name in declared:
        assert hasattr(lib, name), name
    assert sorted(pkg._lib.TRACK_EXPORTS) == declared
    ftp_h = open(os.path.join(ROOT, "include", "vistaf_ftp.h")).read()
    assert "vistaf_track" not in ftp_h                                               # its own header; vistaf_ftp.h is unchanged


def test_track_c_abi_refuses_null_and_bad_arguments(pkg):
    lib = pkg._lib.load()
    E_INVALID = -1
    buf = (ctypes.c_double * 16)()
    i8 = (ctypes.c_int8 * 16)()
    cnt = (ctypes.c_int32 * 1)()
    assert lib.vistaf_track_update(None, i8, buf, cnt, 1, buf, cnt, None) == E_INVALID
    assert b"null" in lib.vistaf_ftp_last_error()
    assert lib.vistaf_track_update(None, None, None, None, 1, None, None, None) == E_INVALID
    assert lib.vistaf_track_reset(None) == E_INVALID
    lib.vistaf_track_destroy(None)
    assert lib.vistaf_track_create(8, 8, 1, 8, 0.0, None) == E_INVALID
    h = ctypes.c_void_p()
    for args in ((0, 8, 1, 8, 0.0), (8, 0, 1, 8, 0.0), (8, 8, 0, 8, 0.0), (8, 8, 1, 0, 0.0), (8, 8, 1, 65, 0.0), (8, 8, 1, 8, -1.0),
                 (8, 8, 1, 8, float("nan")), (8, 8, 1, 8, float("inf"))):
        assert lib.vistaf_track_create(*args, ctypes.byref(h)) == E_INVALID, args
        assert not h.value


def _hand_made():
    c = np.full((3, 2, 16), np.nan)
    c[0, :, 0] = c[2, :, 0] = 5                      # tracks_table reads only the shape of the contacts table
    t = np.full((3, 2, 16), np.nan)
    t[0, 0, :10] = [0, 0, -1, BORN, 0, np.nan, np.nan, np.nan, np.nan, -1]
    t[0, 1, :10] = [1, 0, -1, BORN | SPLIT, 0, np.nan, np.nan, np.nan, np.nan, 0]
    t[2, 0, :10] = [1, 1, 1, MERGED, 37, -2.5, 0.25, 0.125, -1e-4, -1]
    t[2, 1, :10] = [2 ** 40, 7, 0, GATED, 0, 3.0, np.nan, 0.0, 0.0, -1]
    return t, c, np.array([2, 0, 5], np.int32)


def test_tracks_table_and_csv_round_trip(pkg, tmp_path):
    t, c, n = _hand_made()
    rows = pkg.tracks_table(t, c, n)
    assert [(r["frame"], r["contact"]) for r in rows] == [(0, 0), (0, 1), (2, 0), (2, 1)]
    assert list(rows[0])[2:] == list(pkg.TRACK_NAMES)
    assert rows[1]["events"] == BORN | SPLIT and rows[1]["origin_track_id"] == 0 and np.isnan(rows[0]["dx"])
    assert rows[2]["overlap_px"] == 37 and isinstance(rows[2]["overlap_px"], int) and rows[2]["dx"] == -2.5 and rows[2]["dvolume_cm3"] == -1e-4
    assert rows[3]["track_id"] == 2 ** 40 and isinstance(rows[3]["track_id"], int) and np.isnan(rows[3]["dy"])
    one = pkg.tracks_table(t[2], c[2], n[2])
    assert len(one) == 2 and one[0]["parent_row"] == 1
    with pytest.raises(ValueError):
        pkg.tracks_table(t[:, :, :5], c, n)
    with pytest.raises(ValueError):
        pkg.tracks_table(t, c[:, :1], n)
    path = pkg.write_tracks_csv(str(tmp_path), t, c, n)
    with open(path, newline="") as f:
        back = list(csv.DictReader(f))
    assert len(back) == 4 and list(back[0]) == ["frame", "contact"] + list(pkg.TRACK_NAMES)
    for r, s in zip(rows, back):
        for k, v in r.items():
            got = float(s[k])
            assert (np.isnan(v) and np.isnan(got)) or got == v, k


# ---------------------------------------------------------------------------------------------------------------- GPU, direct
def _run(pkg, planes, tab, counts, K, gate=0.0, splits=None, tracker=None):
    """the frames through a ContactTracker, in one update or in updates of the given sizes; host arrays back"""
    import torch
    h, w = planes.shape[1:]
    tr = tracker or pkg.ContactTracker(h, w, max(splits) if splits else len(planes), K, gate)
    tracks, fate = [], []
    b0 = 0
    for nb in splits or [len(planes)]:
        o = tr.update(planes[b0:b0 + nb], tab[b0:b0 + nb], counts[b0:b0 + nb])
        tracks.append(o["tracks"])
        fate.append(o["fate"])
        b0 += nb
    assert b0 == len(planes)
    torch.cuda.synchronize()
    if tracker is None:
        tr.close()
    return torch.cat(tracks).cpu().numpy(), torch.cat(fate).cpu().numpy()


def _check(pkg, sc, K, gate=0.0, splits=None):
    """run a scene, compare every field with numpy_tracks; returns the tracker's tables"""
    planes, tab, counts = sc
    got_t, got_f = _run(pkg, planes, tab, counts, K, gate, splits)
    want_t, want_f, _ = TH.numpy_tracks(planes, tab, counts, K, gate)
    assert got_t.shape == (len(planes), K, 16) and got_f.shape == (len(planes), K) and got_f.dtype == np.int32
    for t in range(len(planes)):
        assert TH.same_bits(got_t[t], want_t[t]), (t, got_t[t, :, :10], want_t[t, :, :10])
        assert np.array_equal(got_f[t], want_f[t]), (t, got_f[t], want_f[t])
    return got_t, got_f


@pytest.mark.gpu
def test_steady_drift_keeps_ids_while_rows_swap(pkg):
    K = 4
    frames = []
    for t in range(5):
        a, b = (5 + 2 * t, 5, 12 + 2 * t, 12), (30 - t, 20 + t, 38 - t, 28 + t)
        frames.append([a, b] if t != 2 and t != 3 else [b, a])                       # the table's order flips for two frames
    tr, fate = _check(pkg, TH.scene(H, W, frames, K), K)
    a_row = [0, 0, 1, 1, 0]
    for t in range(5):
        ra, rb = tr[t, a_row[t]], tr[t, 1 - a_row[t]]
        assert (ra[T["track_id"]], rb[T["track_id"]]) == (0, 1) and ra[T["age_frames"]] == rb[T["age_frames"]] == t
        assert np.isnan(tr[t, 2:]).all() and np.isnan(tr[t, :2, 10:]).all()
        if t:
            assert ra[T["events"]] == rb[T["events"]] == 0 and ra[T["parent_row"]] == a_row[t - 1]
            assert (ra[T["dx"]], ra[T["dy"]], ra[T["overlap_px"]]) == (2.0, 0.0, 6 * 8) and (rb[T["dx"]], rb[T["dy"]]) == (-1.0, 1.0)
            assert fate[t, a_row[t - 1]] == a_row[t] and (fate[t, 2:] == NO_ROW).all()
    assert (tr[0, :2, T["events"]] == BORN).all() and (fate[0] == NO_ROW).all()


@pytest.mark.gpu
def test_split_and_merge_events_origin_and_fate(pkg):
    K = 4
    whole, small, large = (10, 10, 30, 20), (10, 10, 18, 20), (21, 10, 30, 20)
    tr, fate = _check(pkg, TH.scene(H, W, [[whole], [small, large], [whole]], K), K)
    # frame 1: the larger part keeps the track, the smaller one broke off it
    assert tr[1, 1, T["parent_row"]] == 0 and tr[1, 1, T["track_id"]] == 0 and tr[1, 1, T["events"]] == 0 and tr[1, 1, T["overlap_px"]] == 110
    assert tr[1, 0, T["events"]] == BORN | SPLIT and tr[1, 0, T["origin_track_id"]] == 0 and tr[1, 0, T["track_id"]] == 1
    assert tr[1, 1, T["origin_track_id"]] == -1 and fate[1, 0] == 1
    # frame 2: both flow into one contact; the larger part's track goes on, the smaller one is absorbed
    assert tr[2, 0, T["parent_row"]] == 1 and tr[2, 0, T["track_id"]] == 0 and tr[2, 0, T["age_frames"]] == 2 and tr[2, 0, T["events"]] == MERGED
    assert fate[2, 1] == 0 and fate[2, 0] == -(2 + 0) and (fate[2, 2:] == NO_ROW).all()


@pytest.mark.gpu
def test_exact_overlap_tie_goes_to_the_lowest_row(pkg):
    K = 4
    whole, left, right = (10, 10, 29, 20), (10, 10, 19, 20), (20, 10, 29, 20)
    for halves in ([left, right], [right, left]):
        tr, fate = _check(pkg, TH.scene(H, W, [[whole], halves, [whole]], K), K)
        assert tr[1, 0, T["parent_row"]] == 0 and tr[1, 1, T["events"]] == BORN | SPLIT          # best_next[0]: O[0][0] == O[0][1]
        assert tr[2, 0, T["parent_row"]] == 0 and tr[2, 0, T["events"]] == MERGED and fate[2, 1] == -2       # best_prev[0]: O[0][0] == O[1][0]


@pytest.mark.gpu
@pytest.mark.parametrize("gate,linked", [(8.0, True), (7.0, True), (6.0, False), (0.0, False)])
def test_gate_links_a_jump_without_overlap(pkg, gate, linked):
    K = 4
    tr, fate = _check(pkg, TH.scene(H, W, [[(5, 5, 7, 7)], [(12, 5, 14, 7)]], K), K, gate)          # centroids 7 px apart, no common pixel
    if linked:
        assert tr[1, 0, T["events"]] == GATED and tr[1, 0, T["track_id"]] == 0 and tr[1, 0, T["overlap_px"]] == 0 and tr[1, 0, T["dx"]] == 7.0
        assert fate[1, 0] == 0
    else:
        assert tr[1, 0, T["events"]] == BORN and tr[1, 0, T["track_id"]] == 1 and fate[1, 0] == -1


@pytest.mark.gpu
def test_gate_equal_distances_greedy_conflict_and_nan_centroids(pkg):
    K = 4
    # two candidates at the same d2 = 25 from one row: (d2, i, j) picks the lower j
    tr, fate = _check(pkg, TH.scene(H, W, [[(9, 9, 11, 11)], [(14, 9, 16, 11), (9, 14, 11, 16)]], K), K, 6.0)
    assert tr[1, 0, T["events"]] == GATED and tr[1, 1, T["events"]] == BORN and fate[1, 0] == 0
    # ... and two rows at the same d2 from one candidate: the lower i
    tr, fate = _check(pkg, TH.scene(H, W, [[(14, 9, 16, 11), (9, 14, 11, 16)], [(9, 9, 11, 11)]], K), K, 6.0)
    assert tr[1, 0, T["parent_row"]] == 0 and list(fate[1, :2]) == [0, -1]
    # greedy: (i0, j0) at 4 px is linked first and takes i0, the nearest row of j1 (6 px); j1 then gets i1 at 16 px
    sc = TH.scene(H, W, [[(9, 9, 11, 11), (19, 9, 21, 11)], [(13, 9, 15, 11), (3, 9, 5, 11)]], K)
    tr, fate = _check(pkg, sc, K, 17.0)
    assert list(tr[1, :2, T["parent_row"]]) == [0, 1] and list(tr[1, :2, T["dx"]]) == [4.0, -16.0] and list(fate[1, :2]) == [0, 1]
    tr, fate = _check(pkg, sc, K, 7.0)                                               # with a 7 px gate j1 is left over
    assert list(tr[1, :2, T["parent_row"]]) == [0, -1] and list(fate[1, :2]) == [0, -1]
    # a row without a finite centroid takes no part in the gate stage
    sc = TH.scene(H, W, [[(5, 5, 7, 7)], [(12, 5, 14, 7)]], K, centroids=[[None], None])
    tr, fate = _check(pkg, sc, K, 8.0)
    assert tr[1, 0, T["events"]] == BORN


@pytest.mark.gpu
def test_truncated_tables_and_an_empty_frame(pkg):
    K = 2
    four = [(2, 2, 8, 8), (12, 2, 18, 8), (22, 2, 28, 8), (32, 2, 38, 8)]
    moved = [(x0 + 1, y0 + 1, x1 + 1, y1 + 1) for (x0, y0, x1, y1) in four]
    sc = TH.scene(H, W, [four, moved, [], moved, four], K)
    assert list(sc[2]) == [4, 4, 0, 4, 4] and sc[0].max() == 1                        # count > K; the contacts beyond K are -1 in the plane
    tr, fate = _check(pkg, sc, K)
    assert list(tr[1, :, T["track_id"]]) == [0, 1] and list(tr[1, :, T["age_frames"]]) == [1, 1]
    assert np.isnan(tr[2]).all() and list(fate[2]) == [-1, -1]                       # the empty frame ends both tracks
    assert (fate[3] == NO_ROW).all() and list(tr[3, :, T["track_id"]]) == [2, 3] and (tr[3, :, T["events"]] == BORN).all()
    assert list(tr[4, :, T["track_id"]]) == [2, 3]


@pytest.mark.gpu
def test_small_table_after_a_tracker_of_64_births(pkg):
    """rows K..63 of the link rows k_tr_ids reads belong to no contact: a K = 2 tracker whose scratch memory may be what a K = 64 tracker
    full of births left behind hands out the same ids"""
    far = [[(1 + 6 * c + 3 * (t % 2), 1 + 4 * r, 2 + 6 * c + 3 * (t % 2), 2 + 4 * r) for r in range(8) for c in range(8)] for t in range(5)]
    tr, _ = _check(pkg, TH.scene(H, W, far, 64), 64)                                 # no overlap between frames: 64 births in each
    assert (tr[:, :, T["events"]] == BORN).all() and tr[4, 63, T["track_id"]] == 5 * 64 - 1
    two = [(2, 2, 8, 8), (12, 2, 18, 8)]
    tr, _ = _check(pkg, TH.scene(H, W, [two, two, [], two, two], 2), 2)
    assert list(tr[3, :, T["track_id"]]) == [2, 3]


@pytest.mark.gpu
def test_full_histogram_of_64_contacts(pkg):
    K = 64
    rng = np.random.default_rng(64)
    frames = []
    for t in range(3):
        rects = [(1 + 6 * c + t, 1 + 4 * r, 3 + 6 * c + t, 3 + 4 * r) for r in range(8) for c in range(8)]
        frames.append([rects[k] for k in rng.permutation(64)])
    tr, fate = _check(pkg, TH.scene(H, W, frames, K), K)
    assert sorted(tr[2, :, T["track_id"]]) == list(range(64)) and (tr[2, :, T["age_frames"]] == 2).all()
    assert (tr[1:, :, T["overlap_px"]] == 6).all() and (tr[1:, :, T["dx"]] == 1.0).all() and sorted(fate[2]) == list(range(64))


@pytest.mark.gpu
@pytest.mark.parametrize("K,gate,seed", [(8, 0.0, 401), (4, 6.0, 402)])
def test_forty_random_frames(pkg, K, gate, seed):
    sc = TH.random_scene(H, W, 40, K, seed)
    tr, fate = _check(pkg, sc, K, gate)
    ev = tr[:, :, T["events"]]
    ev = ev[~np.isnan(ev)].astype(int)
    print("K", K, "gate", gate, "rows", ev.size, "born", (ev & BORN > 0).sum(), "split", (ev & SPLIT > 0).sum(), "merged", (ev & MERGED > 0).sum(),
          "gated", (ev & GATED > 0).sum(), "truncated frames", int((sc[2] > K).sum()))
    assert (ev == 0).sum() > 20 and (ev & BORN > 0).sum() > 5                        # the scene does exercise links and births


@pytest.mark.gpu
def test_batch_split_invariance_reset_and_one_frame_updates(pkg):
    """the carried state: 7 frames in one update against updates of (1, 6), (3, 4) and (1, 1, ..., 1)"""
    K, gate = 4, 5.0
    planes, tab, counts = TH.random_scene(H, W, 7, K, 413, max_rects=5)
    want = TH.numpy_tracks(planes, tab, counts, K, gate)
    whole = _run(pkg, planes, tab, counts, K, gate)
    assert TH.same_bits(whole[0], want[0]) and np.array_equal(whole[1], want[1])
    assert np.nanmax(whole[0][:, :, T["track_id"]]) >= 5 and np.nanmax(whole[0][:, :, T["age_frames"]]) >= 2
    for splits in ([1, 6], [3, 4], [1] * 7):
        got = _run(pkg, planes, tab, counts, K, gate, splits)
        assert np.array_equal(got[0].view(np.int64), whole[0].view(np.int64)), splits       # every bit, NaNs included
        assert np.array_equal(got[1], whole[1]), splits
    tr = pkg.ContactTracker(H, W, 7, K, gate)
    first = _run(pkg, planes, tab, counts, K, gate, tracker=tr)
    again = _run(pkg, planes, tab, counts, K, gate, tracker=tr)                      # goes on from the carried frame: new ids
    assert np.nanmin(again[0][:, :, T["track_id"]][again[0][:, :, T["events"]] == BORN]) > np.nanmax(first[0][:, :, T["track_id"]])
    tr.reset()
    fresh = _run(pkg, planes, tab, counts, K, gate, tracker=tr)                      # reset: ids restart at 0, nothing is carried
    tr.close()
    for got in (first, fresh):
        assert np.array_equal(got[0].view(np.int64), whole[0].view(np.int64)) and np.array_equal(got[1], whole[1])
    with pytest.raises(ValueError):
        pkg.ContactTracker(H, W, 2, K).update(planes[:3], tab[:3], counts[:3])       # batch > max_batch
    with pytest.raises(ValueError):
        pkg.ContactTracker(H, W, 2, 0)
    with pytest.raises(ValueError):
        pkg.ContactTracker(H, W, 2, K, gate_px=-1.0)


@pytest.mark.gpu
def test_two_trackers_give_the_same_bits(pkg):
    K = 8
    planes, tab, counts = TH.random_scene(H, W, 9, K, 404)
    a = _run(pkg, planes, tab, counts, K, 4.0)
    b = _run(pkg, planes, tab, counts, K, 4.0)
    assert np.array_equal(a[0].view(np.int64), b[0].view(np.int64)) and np.array_equal(a[1], b[1])


@pytest.mark.gpu
def test_chunked_tier_on_native_size_planes(pkg):
    n, K = 1182, 8
    f0 = [(100, 100, 400, 300), (700, 650, 1100, 1181), (0, 0, 15, 9), (500, 40, 520, 45)]
    f1 = [(690, 640, 1090, 1170), (110, 95, 410, 305), (1166, 1172, 1181, 1181), (3, 2, 18, 11)]
    tr, fate = _check(pkg, TH.scene(n, n, [f0, f1], K), K, 30.0)
    assert list(tr[1, :4, T["parent_row"]]) == [1, 0, -1, 2] and tr[1, 1, T["overlap_px"]] == 291 * 201 and list(fate[1, :4]) == [1, 0, 3, -1]


# ---------------------------------------------------------------------------------------------------------------- GPU, through the session
def _session(pkg, max_batch):
    n = TH.MOVING_N
    model, neg = pkg.load_calibration(os.path.join(G, "calibration_phase_to_height.json"))
    fm = pkg.load_force_calibration(os.path.join(G, "calibration_height_to_force.json"))["best_model"]
    return pkg.FtpSensor(pkg.synth.reference_frame(n), pkg.synth.roi_circle(n), pkg.FtpConfig.scaled(n), model, neg, fm, max_batch=max_batch)


_MOVING = {}


def _moving(pkg):
    """the 12 frames of the moving-bumps scene through FtpSensor.track(4), once in one call and once as 5 + 7; host arrays"""
    if not _MOVING:
        import torch
        frames = TH.moving_bumps_frames(pkg)
        keys = ("contact_index", "contacts", "count", "tracks", "fate")
        s = _session(pkg, TH.MOVING_B)
        s.predict_batch(frames)
        one = {k: v.cpu().numpy() for k, v in s.track(4).items()}
        s.close()
        s = _session(pkg, 7)
        parts = []
        for lo, hi in ((0, 5), (5, 12)):
            s.predict_batch(frames[lo:hi])
            parts.append(s.track(4))
        two = {k: torch.cat([p[k] for p in parts]).cpu().numpy() for k in keys}
        s.close()
        _MOVING.update(one=one, two=two)
    return _MOVING


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["one", "two"])
def test_session_track_equals_numpy_on_the_gpu_planes(pkg, how):
    r = _moving(pkg)[how]
    assert r["tracks"].shape == (TH.MOVING_B, 4, 16) and r["fate"].shape == (TH.MOVING_B, 4)
    want_t, want_f, _ = TH.numpy_tracks(r["contact_index"], r["contacts"], r["count"], 4, 0.0)
    for t in range(TH.MOVING_B):
        assert TH.same_bits(r["tracks"][t], want_t[t]), (t, r["tracks"][t, :, :10], want_t[t, :, :10])
    assert np.array_equal(r["fate"], want_f)
    if how == "two":
        one = _moving(pkg)["one"]
        for k in r:
            assert np.array_equal(r[k].view(np.uint8), one[k].view(np.uint8)), k       # 5 + 7 frames: the same bits as 12 at once


@pytest.mark.gpu
def test_session_track_follows_two_moving_contacts(pkg):
    r = _moving(pkg)["one"]
    print("counts", r["count"], "ids", r["tracks"][:, :2, T["track_id"]].tolist())
    assert (r["count"] == 2).all()                                                   # the scene keeps two contacts in every frame (checked with the oracle too)
    tr = r["tracks"]
    for t in range(TH.MOVING_B):
        assert sorted(tr[t, :2, T["track_id"]]) == [0, 1] and (tr[t, :2, T["age_frames"]] == t).all()
        assert (tr[t, :2, T["events"]] == (BORN if t == 0 else 0)).all()
    # the deeper bump (row 0 of frame 0) moves along +angle, the other one against it: about 2 px per frame each
    for tid in (0, 1):
        step = np.array([tr[t, list(tr[t, :2, T["track_id"]]).index(tid), [T["dx"], T["dy"]]] for t in range(1, TH.MOVING_B)])
        assert 1.0 < np.hypot(*step.mean(axis=0)) < 3.0, (tid, step)


@pytest.mark.gpu
def test_track_leaves_the_predict_path_alone(pkg):
    import torch
    n, nb = TH.MOVING_N, 4
    a, other = CH.multi_contact_batch(pkg, n, 0, nb), pkg.synth.deformed_batch(n, 0, nb)

    def snap(o):
        return {k: v.clone() for k, v in o.items()}

    def equal(x, y):
        return all(torch.equal(x[k].contiguous().view(torch.uint8), y[k].contiguous().view(torch.uint8)) for k in x)
    s1, s2 = _session(pkg, nb), _session(pkg, nb)
    with pytest.raises(RuntimeError):
        s1.track()                                       # no predict yet
    o = s1.predict_batch(a)
    before = snap(o)
    plain = snap(s1.contacts(8, index_plane=True))
    planes = {p: s1.intermediate(p, nb, torch.uint8).clone() for p in ("kept", "depth", "labels", "peak_bits")}
    got = s1.track(8, gate_px=3.0)
    assert set(got) == {"contacts", "count", "contact_index", "tracks", "fate"}
    s1.track(8, gate_px=3.0)
    with pytest.raises(ValueError):
        s1.track(4, gate_px=3.0)                         # another table size without reset
    with pytest.raises(ValueError):
        s1.track(8)                                      # another gate without reset
    again = s1.track(4, reset=True)
    torch.cuda.synchronize()
    assert (again["tracks"][:, :, T["track_id"]].nan_to_num(nan=0.0) < 4 * nb).all() and again["tracks"].shape == (nb, 4, 16)
    assert np.nanmin(again["tracks"][0, :, T["track_id"]].cpu().numpy()) == 0        # reset: ids restart at 0
    assert equal(o, before) and equal({k: got[k] for k in plain}, plain)
    for p, v in planes.items():
        assert torch.equal(s1.intermediate(p, nb, torch.uint8), v), p
    assert equal(snap(s1.contacts(8, index_plane=True)), plain)                      # a following contacts() is what it was
    after, fresh = snap(s1.predict_batch(other)), s2.predict_batch(other)
    torch.cuda.synchronize()
    assert equal(after, fresh)
    assert equal(s1.contacts(8, index_plane=True), s2.contacts(8, index_plane=True))
    s1.close()
    s2.close()
