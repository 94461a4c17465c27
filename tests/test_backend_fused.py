"""The back end of a predict: the one-launch tier (csrc/k_backend.hip, test hook "fused_backend" = 1, the default) against the separate
kernels it replaces (= 0), bit for bit; and the one-wave two-pass chamfer transform launched directly (vistaf_ftp_test_chamfer) against the
two sequential loops of cv::distanceTransform's 3x3 mask, exactly.  The frames are built as tests/test_config_surface.py builds its own, and
the CPU oracle confirms that each one has the property it is there for."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import ftp_oracle as O
import test_config_surface as S

G = os.path.join(os.path.dirname(__file__), "golden")
P1182 = 65.83619546657023 / 1182


@pytest.fixture(scope="module")
def cal(pkg):
    model, neg = pkg.load_calibration(os.path.join(G, "calibration_phase_to_height.json"))
    fm = pkg.load_force_calibration(os.path.join(G, "calibration_height_to_force.json"))["best_model"]
    return model, neg, fm


# =======================================================================================================================================
# 1. fused and separate back end agree

def _scene(h, w, kind, seed):
    """A frame of test_config_surface._frame's family at h x w, dents placed relative to the ROI circle (centre of the frame)."""
    circle = (w // 2, h // 2, min(h, w) // 2 - 1)
    n = min(h, w)
    s, cx, cy = n / 224.0, w / 2, h / 2
    period = None if n == 224 else P1182 * n
    dents = {
        "ref": (),
        # the main dent, a secondary one above a third of its depth and one below (S._multi_dent)
        "multi": ((cx - 32 * s, cy - 17 * s, 16 * s, 1.2), (cx + 38 * s, cy - 42 * s, 10 * s, 0.36, 0.4), (cx + 28 * s, cy + 48 * s, 10 * s, 0.31, 0.4)),
        "single": ((cx, cy, 20 * s, 1.0),),
        "pair": ((cx - 40 * s, cy, 14 * s, 1.0), (cx + 40 * s, cy, 14 * s, 0.9)),
        "bump": ((cx, cy, 20 * s, -1.0),),
    }
    if kind == "flat":          # no fringes at all
        return np.full((h, w), 128, np.uint8)
    return S._frame(h, w, circle, seed, dents=dents[kind], period=period)


def _props(o, roi):
    """(candidate pixels, candidate blobs, candidate pixels the filter removed, pixels kept) of an oracle result"""
    d = o["inter"]["depth_mm"]
    cand = roi & np.isfinite(d) & (d > 0.0)
    kept = o["contact_kept_by_depth"]
    peaks, _ = S._blobs(o, roi)
    return int(cand.sum()), len(peaks), int((cand & ~kept).sum()), int(kept.sum())


def _expect(prop, o, roi):
    if prop == "status":
        assert o is None
        return
    ncand, nblobs, removed, kept = _props(o, roi)
    if prop == "removed":       # several blobs, the filter removes some and keeps some
        assert nblobs >= 3 and removed > 0 and kept > 0, (ncand, nblobs, removed, kept)
    elif prop == "all_removed":
        assert ncand > 0 and kept == 0
    elif prop == "all_kept":
        assert nblobs >= 2 and removed == 0, (nblobs, removed)
    elif prop == "none":        # no candidate: empty label set, per-frame maximum 0
        assert ncand == 0
    else:
        raise AssertionError(prop)


# (id, h, w, overrides of the scaled constants, [(scene, seed, property)])
CASES = [
    ("64x64_b3", 64, 64, {}, [("multi", 901, "removed"), ("single", 902, "removed"), ("flat", 0, "none")]),
    ("64x64_b3_all_kept", 64, 64, dict(contact_blob_min_peak_mm=0.0, contact_blob_min_peak_rel_frac=0.0),
     [("multi", 901, "all_kept"), ("single", 902, "all_kept"), ("pair", 903, "all_kept")]),
    ("64x64_b3_status", 64, 64, dict(reliable_edge_margin_px=40), [("multi", 901, "status"), ("single", 902, "status"), ("flat", 0, "status")]),
    ("96x80_b2", 96, 80, {}, [("multi", 901, "removed"), ("bump", 904, "all_removed")]),
    ("224x224_removed", 224, 224, {}, [("multi", 901, "removed")]),
    # the fringe-free frame at 224 x 224 is NOT a frame without candidates (that one is the 64 x 64 case above): against this reference
    # the oracle finds two deep blobs in it, and the filter keeps both
    ("224x224_fringe_free_two_blobs_kept", 224, 224, {}, [("flat", 0, "all_kept")]),
]


def _run(sensor, frames, fused):
    sensor._test_set("fused_backend", fused)
    out = sensor.predict_batch(frames)
    ct = sensor.contacts(max_contacts=8, index_plane=True)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got.update({k: v.cpu().numpy() for k, v in ct.items()})
    got["kept"] = sensor.intermediate("kept", len(frames), torch.uint8).cpu().numpy()        # the mask the contacts read-out works on
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_fused_backend_equals_separate_kernels(pkg, cal, case):
    _, h, w, over, scenes = case
    circle = (w // 2, h // 2, min(h, w) // 2 - 1)
    cfg = pkg.FtpConfig.scaled(min(h, w))
    for k, v in over.items():
        setattr(cfg, k, v)
    ref = _scene(h, w, "ref", 900)
    frames = np.stack([_scene(h, w, kind, seed) for kind, seed, _ in scenes])
    # the frames are what they are meant to be
    rs = O.make_reference_state(ref, *circle, cfg)
    for f, (_, _, prop) in zip(frames, scenes):
        _expect(prop, O.process_frame(f, rs, cfg, *cal, keep_intermediates=True), rs["roi"])
    sensor = pkg.FtpSensor(ref, circle, cfg, cal[0], cal[1], cal[2], max_batch=len(frames))
    sensor._test_set("keep_planes", 1)
    a = _run(sensor, frames, 1)
    b = _run(sensor, frames, 0)
    c = _run(sensor, frames, 1)        # and again on the planes the separate kernels left behind
    want_status = 1 if scenes[0][2] == "status" else 0
    assert (b["status"] == want_status).all(), b["status"]
    assert set(a) == set(b) and {"height_map_mm", "output_reliable", "scalars", "status", "contacts", "count", "contact_index"} <= set(a)
    for key in b:
        for got in (a, c):
            assert got[key].dtype == b[key].dtype and got[key].shape == b[key].shape, key
            assert np.array_equal(got[key], b[key], equal_nan=got[key].dtype.kind == "f"), key
    if want_status == 0 and scenes[0][2] in ("removed", "all_kept"):
        assert (b["count"] > 0).any() and b["kept"].any()


# =======================================================================================================================================
# 2. the distance pair against the sequential two-pass reference

HV, DG, DIST_MAX = 62587, 89738, 0x7fffffff >> 2       # cvRound(0.955 * 65536), cvRound(1.3693 * 65536), cv's DIST_MAX


def two_pass_3x3(zero):
    """distanceTransform_3x3's two loops on a bordered int64 plane (values stay below 2^31), distance to the True pixels of `zero`;
    the result as cv stores it: min(d, DIST_MAX) / 65536 in float32"""
    h, w = zero.shape
    t = np.full((h + 2, w + 2), DIST_MAX, np.int64)
    for y in range(1, h + 1):
        for x in range(1, w + 1):
            if zero[y - 1, x - 1]:
                t[y, x] = 0
            else:
                t[y, x] = min(t[y - 1, x - 1] + DG, t[y - 1, x] + HV, t[y - 1, x + 1] + DG, t[y, x - 1] + HV)
    out = np.empty((h, w), np.int64)
    for y in range(h, 0, -1):
        for x in range(w, 0, -1):
            d = t[y, x]
            if d > HV:
                d = min(d, t[y + 1, x + 1] + DG, t[y + 1, x] + HV, t[y + 1, x - 1] + DG, t[y, x + 1] + HV)
                t[y, x] = d
            out[y - 1, x - 1] = min(d, DIST_MAX)
    return (out.astype(np.float32) * np.float32(1.0 / 65536.0)).astype(np.float32)


def _masks(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    corners = np.ones((h, w), np.uint8)
    corners[0, 0] = corners[0, w - 1] = corners[h - 1, 0] = corners[h - 1, w - 1] = 0
    return {
        "zeros": np.zeros((h, w), np.uint8),
        "ones": np.ones((h, w), np.uint8),
        "corners": corners,
        "checker": ((yy + xx) & 1).astype(np.uint8),
        "random50": (rng.random((h, w)) < 0.5).astype(np.uint8),
        "random1": (rng.random((h, w)) < 0.01).astype(np.uint8) * np.uint8(255),
    }


# (h, w, cap_px).  Ring depths of the kernel: 31 rows at up to 256 columns (4 per lane), 15 up to 512 (8 per lane), 6 beyond (20 per lane).
# 5 and 17 rows are below the ring, 33, 64 and 70 no multiple of it.  Rows that are a multiple of four columns take the dword / dwordx4
# accesses (17 x 64, 64 x 224, 70 x 260 with 8 per lane); 5 x 7 and 33 x 65 (ragged last lane) the element-wise fallback with 4 per lane,
# 70 x 262 and 40 x 301 with 8 per lane, 70 x 515 with 20 per lane (pair launch only, and only for a band beyond 64 rows: cap 70)
SHAPES = [(5, 7, 48), (17, 64, 48), (33, 65, 48), (64, 224, 48), (70, 260, 48), (70, 262, 48), (40, 301, 48), (70, 515, 70)]
_REF = {}


def _reference(h, w):
    if (h, w) not in _REF:
        ms = _masks(h, w, 1000 * h + w)
        _REF[(h, w)] = {k: (m, two_pass_3x3(m == 0), two_pass_3x3(m != 0)) for k, m in ms.items()}
    return _REF[(h, w)]


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,cap", SHAPES, ids=["%dx%d" % s[:2] for s in SHAPES])
def test_chamfer_pair_equals_the_sequential_two_pass(pkg, h, w, cap):
    ref = _reference(h, w)
    names = list(ref)
    lib = pkg._lib.load()
    for i in range(0, len(names), 3):           # B = 3: both sets of three masks from one launch
        grp = names[i:i + 3]
        mask = torch.from_numpy(np.stack([ref[k][0] for k in grp])).cuda()
        da = torch.full((3, h, w), -1.0, dtype=torch.float32, device="cuda")
        db = torch.full((3, h, w), -1.0, dtype=torch.float32, device="cuda")
        pkg._lib.check(lib.vistaf_ftp_test_chamfer(ctypes.c_void_p(mask.data_ptr()), 1, 0, ctypes.c_void_p(da.data_ptr()), ctypes.c_void_p(db.data_ptr()),
                                                   3, h, w, cap, None))
        da, db = da.cpu().numpy(), db.cpu().numpy()
        for j, k in enumerate(grp):
            assert np.array_equal(da[j], ref[k][1]), (k, "to the zero pixels")
            assert np.array_equal(db[j], ref[k][2]), (k, "to the non-zero pixels")
        # the single-set launcher (the hole stage's and the erosion fallback's), both polarities
        if w <= 512:
            for inv, col in ((0, 1), (1, 2)):
                d1 = torch.full((3, h, w), -1.0, dtype=torch.float32, device="cuda")
                pkg._lib.check(lib.vistaf_ftp_test_chamfer(ctypes.c_void_p(mask.data_ptr()), 0, inv, ctypes.c_void_p(d1.data_ptr()), None, 3, h, w, cap, None))
                d1 = d1.cpu().numpy()
                for j, k in enumerate(grp):
                    assert np.array_equal(d1[j], ref[k][col]), (k, inv)


def test_two_pass_restatement_matches_the_oracle_transform():
    """the restatement above is the transform the oracle uses (oracle/cvlite.py), where that one is exact: no GPU involved"""
    from oracle import cvlite
    for name, m in _masks(33, 65, 7).items():
        assert np.array_equal(two_pass_3x3(m == 0), np.asarray(cvlite.dist_l2_3x3(m), np.float32)), name
