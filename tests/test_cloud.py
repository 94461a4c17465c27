"""Point-cloud read-out (include/vistaf_cloud.h, cloud.CloudReadout, FtpSensor.cloud): the contact surface as points, normals, curvature.

tests/cloud_helpers.py restates the definition (`numpy_cloud`, the reference of every GPU test), builds the planes and holds the bars: the
offsets, pixel, label, every count, MAX_SLOPE_INDEX, the NaN pattern and all eight float32 fields of every point must be equal bit for bit
(every operation of the definition is a correctly rounded float64 + - * / or sqrt); the float64 sums of a frame row and the angles behind
them must lie within max(4 x the distance of two restatements that add in different orders, 64 ulps) of the field's scale.  The direct GPU
tests hand the read-out hand-made planes (no FTP session): 37 x 53 (an odd pixel count, every frame base misaligned: one pixel per thread)
and 40 x 52 (a multiple of 4: four pixels per thread), and 257 x 257 x 4, whose 259 chunks take the row kernel (256 chunks a round) round
its loop twice and whose 1036 counts take the scan (1024 a round) round its loop twice.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import cloud_helpers as CL
from cloud_helpers import F_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
INCLUDE = os.path.join(ROOT, "include")
SHAPES = {"37x53": (37, 53), "40x52": (40, 52)}
CANARY_F32, CANARY_I32, CANARY_I8 = np.uint32(0x7FC0BEEF), np.int32(-123456789), np.int8(0x55)
_CASES, _REF = {}, {}


def _case(shape):
    if shape not in _CASES:
        _CASES[shape] = CL.hard_batch(*SHAPES[shape])
    return _CASES[shape]


def _reference(shape, stride=1, origin=None, summer="fsum"):
    key = (shape, stride, origin, summer)
    if key not in _REF:
        c = _case(shape)
        _REF[key] = CL.numpy_cloud(c["depth"], c["mpp"], c["eps"], c["status"], c["index"], stride=stride, origin=origin,
                                   summer=CL.fsum if summer == "fsum" else CL.reversed_chunk_sum)
    return _REF[key]


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_cloud_names_and_field_counts_follow_the_header(pkg):
    hdr = open(os.path.join(INCLUDE, "vistaf_cloud.h")).read()
    pt = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define VISTAF_CLOUD_(N?[XYZ]|CURVATURE|GAUSSIAN_CURVATURE)\s+(\d+)\b", hdr)}
    assert sorted(pt.values()) == list(range(8)) and all(pkg.CLOUD_POINT_NAMES[i] == name for name, i in pt.items())
    fr = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define VISTAF_CLOUDFRAME_(\w+)\s+(\d+)\b", hdr)}
    assert sorted(fr.values()) == list(range(12)) and fr.pop("reserved") == 11
    assert all(pkg.CLOUD_FRAME_NAMES[i] == name for name, i in fr.items())
    assert list(pkg.CLOUD_POINT_NAMES) == list(pkg._lib.CLOUD_POINT_NAMES) == list(pkg.writers.CLOUD_POINT_FIELDS) == list(CL.POINT_NAMES)
    assert list(pkg.CLOUD_FRAME_NAMES) == list(pkg._lib.CLOUD_FRAME_NAMES) == list(pkg.writers.CLOUD_FRAME_FIELDS) == list(CL.FRAME_NAMES)
    assert int(re.search(r"#define VISTAF_NCLOUD_POINT\s+(\d+)", hdr).group(1)) == pkg._lib.NCLOUD_POINT == CL.NPOINT == 8
    assert int(re.search(r"#define VISTAF_NCLOUD_FRAME\s+(\d+)", hdr).group(1)) == pkg._lib.NCLOUD_FRAME == CL.NFRAME == 12
    geom = tuple(int(re.search(r"#define VISTAF_CLOUD_%s\s+(\d+)" % n, hdr).group(1)) for n in ("CHUNK_THREADS", "SCAN_THREADS", "ROW_LANES", "ROW_UNROLL"))
    assert geom == (pkg._lib.CLOUD_CHUNK_THREADS, pkg._lib.CLOUD_SCAN_THREADS, pkg._lib.CLOUD_ROW_LANES, pkg._lib.CLOUD_ROW_UNROLL)
    for name in ("cloud", "CloudReadout", "CLOUD_POINT_NAMES", "CLOUD_FRAME_NAMES", "cloud_frame_record", "write_cloud_ply"):
        assert name in pkg.__all__ and hasattr(pkg, name)


def test_library_has_the_declared_cloud_symbols_and_no_other_header_names_them(pkg):
    hdr = open(os.path.join(INCLUDE, "vistaf_cloud.h")).read()
    declared = sorted(set(re.findall(r"\b(vistaf_cloud_\w+)\s*\(", hdr)))
    assert declared == sorted(["vistaf_cloud_create", "vistaf_cloud_measure", "vistaf_cloud_destroy"])
    lib = pkg._lib.load()
    for name in declared:
        assert hasattr(lib, name), name
    assert sorted(pkg._lib.CLOUD_EXPORTS) == declared
    for other in sorted(os.listdir(INCLUDE)):
        if other != "vistaf_cloud.h":
            assert "vistaf_cloud" not in open(os.path.join(INCLUDE, other)).read(), other             # its own header; the others are unchanged


def test_cloud_c_abi_refuses_bad_arguments_without_a_device(pkg):
    lib = pkg._lib.load()
    E_INVALID = -1
    h = ctypes.c_void_p()
    nan, inf = float("nan"), float("inf")
    good = dict(h=4, w=5, max_batch=2, max_points=10, stride=1, origin_x=2.0, origin_y=1.5)

    def create(out=None, **kw):
        a = dict(good, **kw)
        return lib.vistaf_cloud_create(a["h"], a["w"], a["max_batch"], a["max_points"], a["stride"], a["origin_x"], a["origin_y"],
                                       ctypes.byref(h) if out is None else out)
    assert lib.vistaf_cloud_create(4, 5, 2, 10, 1, 2.0, 1.5, None) == E_INVALID and b"out" in lib.vistaf_ftp_last_error()
    bad = [("h", 0), ("h", -1), ("h", 65537), ("w", 0), ("w", 65537), ("max_batch", 0), ("max_batch", -2), ("max_batch", 65536),
           ("max_points", 0), ("max_points", -5), ("stride", 0), ("stride", -1), ("stride", 65)] + \
          [("origin_x", v) for v in (nan, inf, -inf)] + [("origin_y", v) for v in (nan, inf, -inf)]
    for name, v in bad:
        assert create(**{name: v}) == E_INVALID, (name, v)
        msg = lib.vistaf_ftp_last_error()
        assert not h.value and (name.encode() in msg or (name in ("h", "w") and b"frame size" in msg)), (name, v, msg)
    assert create(h=65536, w=32768) == E_INVALID and b"frame size" in lib.vistaf_ftp_last_error()    # 2^31 pixels
    assert create(h=32768, w=65535, max_batch=65535) == E_INVALID and b"max_batch" in lib.vistaf_ftp_last_error()   # 2^21 chunks x 65535 frames
    assert create(stride=64, max_points=1, max_batch=65535, origin_x=-1e9) == 0 and h.value          # the ends of the ranges that are inside
    lib.vistaf_cloud_destroy(h)
    assert create(max_points=2 ** 40) == 0 and h.value                                              # a 64-bit capacity
    lib.vistaf_cloud_destroy(h)
    assert create() == 0 and h.value
    # create touches no device, so the checks of measure run without one; nothing is launched for a refused call
    f32, mpp, st, ci = (ctypes.c_float * 64)(), (ctypes.c_double * 4)(), (ctypes.c_int32 * 4)(), (ctypes.c_int8 * 64)()
    pts, pix, lab, off, fr = (ctypes.c_float * 128)(), (ctypes.c_int32 * 16)(), (ctypes.c_int8 * 16)(), (ctypes.c_int64 * 4)(), (ctypes.c_double * 32)()

    def al(buf, at=16):
        a = ctypes.addressof(buf)
        return a + (at - a % at) % at
    dep, p16 = ctypes.c_void_p(al(f32)), ctypes.c_void_p(al(pts))                                    # h * w = 20 is a multiple of 4: 16-byte loads
    args = dict(cl=h, depth=dep, mpp=mpp, status=st, index=ci, eps=0.01, batch=1, points=p16, pixel=pix, label=lab, offsets=off, frame=fr)

    def measure(**kw):
        a = dict(args, **kw)
        return lib.vistaf_cloud_measure(a["cl"], a["depth"], a["mpp"], a["status"], a["index"], a["eps"], a["batch"], a["points"], a["pixel"],
                                        a["label"], a["offsets"], a["frame"], None)
    for name, word in (("cl", b"handle"), ("depth", b"depth_mm"), ("mpp", b"mm_per_px"), ("points", b"points"), ("pixel", b"pixel"),
                       ("offsets", b"offsets"), ("frame", b"frame")):
        assert measure(**{name: None}) == E_INVALID and word in lib.vistaf_ftp_last_error(), name
    for batch in (0, 3, -1):
        assert measure(batch=batch) == E_INVALID and b"batch" in lib.vistaf_ftp_last_error()
    for shift in (4, 8, 12):
        assert measure(points=ctypes.c_void_p(p16.value + shift)) == E_INVALID
        assert b"points" in lib.vistaf_ftp_last_error() and b"aligned" in lib.vistaf_ftp_last_error()
    assert measure(depth=ctypes.c_void_p(dep.value + 4)) == E_INVALID and b"depth_mm" in lib.vistaf_ftp_last_error() and b"aligned" in lib.vistaf_ftp_last_error()
    assert measure(pixel=ctypes.c_void_p(al(pix) + 2)) == E_INVALID and b"aligned" in lib.vistaf_ftp_last_error()
    lib.vistaf_cloud_destroy(h)
    lib.vistaf_cloud_destroy(None)


def test_readout_object_refuses_bad_arguments_and_needs_a_device_to_measure(pkg):
    import torch
    for kw in (dict(max_points=0), dict(stride=0), dict(stride=65), dict(origin=(float("nan"), 0.0)), dict(max_batch=0), dict(h=0)):
        with pytest.raises(ValueError):
            pkg.CloudReadout(**dict(dict(h=8, w=8, max_batch=1, max_points=16), **kw))
    rd = pkg.CloudReadout(9, 8, 1, 16)
    assert rd.origin == (3.5, 4.0) and pkg.CloudReadout(9, 8, 1, 16, origin=(1, 2)).origin == (1.0, 2.0)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):
            rd.measure(np.zeros((1, 9, 8), np.float32), np.array([0.05]), 0.01)
    rd.close()
    rd.close()


def test_cloud_ply_round_trip_and_frame_record(pkg, tmp_path):
    rng = np.random.default_rng(2)
    pts = rng.standard_normal((37, 8)).astype(np.float32)
    lab = rng.integers(-1, 5, 37).astype(np.int8)
    for label in (None, lab):
        path = pkg.write_cloud_ply(str(tmp_path / ("a.ply" if label is None else "b.ply")), pts, label)
        raw = open(path, "rb").read()
        end = raw.index(b"end_header\n") + len(b"end_header\n")
        head = raw[:end].decode("ascii").split("\n")
        assert head[0] == "ply" and head[1] == "format binary_little_endian 1.0" and "element vertex 37" in head
        props = [ln.split() for ln in head if ln.startswith("property")]
        want = [["property", "float", n] for n in pkg.CLOUD_POINT_NAMES] + ([["property", "char", "label"]] if label is not None else [])
        assert props == want
        dt = np.dtype([(p[2], "<f4" if p[1] == "float" else "i1") for p in props])
        body = np.fromfile(path, dtype=dt, offset=end)
        assert body.shape == (37,) and len(raw) == end + 37 * dt.itemsize
        for i, n in enumerate(pkg.CLOUD_POINT_NAMES):
            assert CL.same_bits(body[n], pts[:, i]), n
        if label is not None:
            assert np.array_equal(body["label"], lab)
    assert len(open(pkg.write_cloud_ply(str(tmp_path / "empty.ply"), np.zeros((0, 8), np.float32)), "rb").read().split(b"end_header\n")[1]) == 0
    with pytest.raises(ValueError):
        pkg.write_cloud_ply(str(tmp_path / "c.ply"), pts[:, :7])
    with pytest.raises(ValueError):
        pkg.write_cloud_ply(str(tmp_path / "c.ply"), pts, lab[:5])
    row = np.array([12, 3, 2, 0.03, 0.04, 0.0, 0.6, 0.8, 36.87, 12.5, 417, np.nan])
    rec = pkg.cloud_frame_record(row)
    assert list(rec) == list(pkg.CLOUD_FRAME_NAMES) and rec["surface_pixels"] == 12 and rec["points_written"] == 2 and rec["max_slope_index"] == 417
    assert all(isinstance(rec[k], int) for k in pkg.writers.CLOUD_FRAME_INT_FIELDS) and rec["tilt_deg"] == 36.87
    none = pkg.cloud_frame_record(np.full(12, np.nan))
    assert none["surface_pixels"] == -1 and none["max_slope_index"] == -1 and np.isnan(none["mean_normal_z"])
    with pytest.raises(ValueError):
        pkg.cloud_frame_record(row[:5])


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("s", [0.1, 0.0625])
def test_reference_on_a_spherical_cap_against_analysis(shape, s):
    err, inner, total = CL.cap_errors(*SHAPES[shape], s)
    print(shape, s, "points", total, "with a positive neighbourhood", inner, "errors", err, "bars", CL.CAP_BARS)
    assert inner > 1500 and total > inner
    for k, bar in CL.CAP_BARS.items():
        assert err[k] <= bar, (k, err[k], bar)


def test_reference_cases_cover_the_definition():
    for shape in SHAPES:
        c, ref = _case(shape), _reference(shape)
        h, w = c["shape"]
        fr, off = ref["frame"], ref["offsets"]
        n = fr[:, F_["surface_pixels"]]
        assert n[0] == 0 and np.isnan(fr[0, 5:]).all() and not fr[0, :5].any()                       # the empty frame
        assert np.isnan(fr[6]).all() and off[7] == off[6]                                            # the skipped frame, full of garbage
        assert (n[[1, 2, 3, 5, 7, 8]] > 100).all() and off[-1] == len(ref["pixel"]) == np.nansum(n)
        pix2 = ref["pixel"][off[2]:off[3]]
        y2, x2 = pix2 // w, pix2 % w
        assert (y2 == 0).any() and (y2 == h - 1).any() and (x2 == 0).any() and (x2 == w - 1).any() and pix2[-1] == h * w - 1   # borders, corner
        q_first = int(fr[3, F_["max_slope_index"]])
        assert q_first == 9 * w + 12                                                                 # the plateau's first corner of four that tie
        e = np.float32(c["eps"])
        assert n[4] == 6 and (c["depth"][4] == e).sum() == 6                                          # at eps: not surface; one step above: surface
        assert np.isnan(c["depth"][5]).any() and np.isposinf(c["depth"][5]).any() and np.isneginf(c["depth"][5]).any() and (c["depth"][5] < 0).any()
        assert np.isfinite(ref["points"]).all()
        for stride in (2, 3):
            r = _reference(shape, stride)
            assert 0 < len(r["pixel"]) < len(ref["pixel"]) and ((r["pixel"] % w) % stride == 0).all() and ((r["pixel"] // w) % stride == 0).all()
            assert np.array_equal(r["frame"][:, [0, 3, 10]], fr[:, [0, 3, 10]], equal_nan=True)      # the frame row ignores the stride
        other = _reference(shape, summer="reversed")
        assert CL.exact_frame_equal(other["frame"], fr) and CL.same_bits(other["points"], ref["points"])


# ---------------------------------------------------------------------------------------------------------------- GPU, direct
def _run(pkg, c, frames=None, max_points=None, stride=1, origin=None, extra=64, reader=None, labels=True):
    """frames (a list; None: all) of case c through one read-out; host arrays, the outputs `extra` entries longer than max_points and
    filled with a canary beforehand"""
    import torch
    sel = list(range(c["depth"].shape[0])) if frames is None else list(frames)
    depth, mpp = c["depth"][sel], c["mpp"][sel]
    status = None if c["status"] is None else c["status"][sel]
    index = c["index"][sel] if (labels and c["index"] is not None) else None
    if max_points is None:
        max_points = depth.size
    rd = reader or pkg.CloudReadout(*c["shape"], len(sel), max_points, stride, origin)
    n = max_points + extra
    out = {"points": torch.from_numpy(np.full((n, 8), CANARY_F32, np.uint32).view(np.float32)).cuda(),
           "pixel": torch.full((n,), int(CANARY_I32), dtype=torch.int32, device="cuda"),
           "label": torch.full((n,), int(CANARY_I8), dtype=torch.int8, device="cuda")}
    res = rd.measure(depth, mpp, c["eps"], status, index, out=out)
    torch.cuda.synchronize()
    assert res["points"].data_ptr() == out["points"].data_ptr() and ("label" in res) == (index is not None)
    tr = rd.trim(res)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got.update(offsets=res["offsets"].cpu().numpy(), frame=res["frame"].cpu().numpy(), total=tr["total"], overflow=tr["overflow"],
               trimmed=len(tr["points"]), labelled=index is not None)
    if reader is None:
        rd.close()
    return got


def _against_reference(got, want, other, max_points, what):
    """want / other: numpy_cloud of the same frames with fsum and with the reversed chunks"""
    total = int(want["offsets"][-1])
    n = min(total, max_points)
    assert got["offsets"].dtype == np.int64 and np.array_equal(got["offsets"], want["offsets"]), what          # never capped
    assert got["total"] == total and got["overflow"] == (total > max_points) and got["trimmed"] == n
    assert CL.same_bits(got["points"][:n], want["points"][:n]), what                                           # eight float32 fields, bit for bit
    assert got["pixel"].dtype == np.int32 and np.array_equal(got["pixel"][:n], want["pixel"][:n]), what
    assert (got["points"][n:].view(np.uint32) == CANARY_F32).all() and (got["pixel"][n:] == CANARY_I32).all(), what   # nothing beyond is touched
    if got["labelled"]:
        assert np.array_equal(got["label"][:n], want["label"][:n]) and (got["label"][n:] == CANARY_I8).all(), what
    else:
        assert (got["label"] == CANARY_I8).all(), what
    fr, wfr = got["frame"], CL.capped(want, max_points)
    assert fr.dtype == np.float64 and CL.exact_frame_equal(fr, wfr), (what, fr, wfr)
    assert CL.exact_frame_equal(other["frame"], want["frame"])
    bar, dist = CL.bars(want["frame"], other["frame"]), CL.distances(fr, wfr)
    print(what, "distance to numpy_cloud", dist, "bar", bar)
    for k in bar:
        assert dist[k] <= bar[k], (what, k, dist[k], bar[k])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("stride,origin", [(1, None), (2, None), (3, (7.25, -3.5))])
def test_direct_planes_equal_numpy_cloud(pkg, shape, stride, origin):
    c = _case(shape)
    want, other = _reference(shape, stride, origin), _reference(shape, stride, origin, "reversed")
    got = _run(pkg, c, stride=stride, origin=origin)
    _against_reference(got, want, other, c["depth"].size, "%s stride %d" % (shape, stride))
    if stride == 1:
        bare = _run(pkg, c, labels=False)                                                           # without a plane no label is written
        _against_reference(bare, want, other, c["depth"].size, shape + " no labels")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_capacity_is_a_guard_not_an_error(pkg, shape):
    c = _case(shape)
    want, other = _reference(shape), _reference(shape, summer="reversed")
    off = want["offsets"]
    total = int(off[-1])
    inside = int(off[3] + (off[4] - off[3]) // 2)                                                    # a cut inside frame 3
    for max_points in (total, total - 1, inside, int(off[5]), int(off[2]), 7, 1):                    # .. and cuts exactly at frame boundaries
        got = _run(pkg, c, max_points=max_points)
        _against_reference(got, want, other, max_points, "%s max_points %d of %d" % (shape, max_points, total))
    assert off[2] == off[1] + want["frame"][1, F_["points"]] and off[5] < total


@pytest.mark.gpu
def test_scan_and_row_kernels_go_round_their_loops(pkg):
    h, w = 257, 257
    chunk = pkg._lib.CLOUD_CHUNK_THREADS * (4 if (h * w) % 4 == 0 else 1)
    nchunks = -(-h * w // chunk)
    B = pkg._lib.CLOUD_SCAN_THREADS // nchunks + 1
    row_round = pkg._lib.CLOUD_ROW_LANES * pkg._lib.CLOUD_ROW_UNROLL                                 # chunks a round of the row kernel's loop
    assert row_round < nchunks < 2 * row_round and nchunks % pkg._lib.CLOUD_ROW_LANES not in (0, 1)  # a second, partly filled round, lanes > 0 in it
    assert B * nchunks > pkg._lib.CLOUD_SCAN_THREADS                                                 # the scan takes a second round
    c = CL.sparse_batch(h, w, B)
    want = CL.numpy_cloud(c["depth"], c["mpp"], c["eps"])
    other = CL.numpy_cloud(c["depth"], c["mpp"], c["eps"], summer=CL.reversed_chunk_sum)
    P = h * w
    for b in (0, B - 1):
        pix = want["pixel"][want["offsets"][b]:want["offsets"][b + 1]]
        assert pix[0] == 0 and pix[-1] == P - 1
    assert want["offsets"][2] == want["offsets"][1] and want["offsets"][-1] > 3000
    got = _run(pkg, c, max_points=int(want["offsets"][-1]) + 5)
    _against_reference(got, want, other, int(want["offsets"][-1]) + 5, "257x257x%d" % B)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_a_frame_does_not_depend_on_its_batch(pkg, shape):
    c = _case(shape)
    F = 2                                                                                           # the frame cut by the borders
    alone = _run(pkg, c, frames=[F])
    first = _run(pkg, c, frames=[F, 6, 1, 5])
    last = _run(pkg, c, frames=[7, 6, 8, 3, F])
    n = int(alone["offsets"][1])
    assert n > 100 and alone["offsets"][0] == 0
    for got, b in ((first, 0), (last, 4)):
        lo, hi = (int(v) for v in got["offsets"][b:b + 2])
        assert hi - lo == n and (b == 0) == (lo == 0)                                               # shifted by the frames before it
        for k in ("points", "pixel", "label"):
            assert CL.same_bits(got[k][lo:hi], alone[k][:n]), (b, k)
        assert CL.same_bits(got["frame"][b], alone["frame"][0]), b                                  # the same bits in the row, sums included
    rd = pkg.CloudReadout(*c["shape"], 9, c["depth"].size)
    one, two, three = _run(pkg, c, reader=rd), _run(pkg, c, reader=rd), _run(pkg, c)
    rd.close()
    for k in ("points", "pixel", "label", "offsets", "frame"):
        assert CL.same_bits(one[k], two[k]) and CL.same_bits(one[k], three[k]), k                  # two calls, two handles
    with pytest.raises(ValueError):
        pkg.CloudReadout(*c["shape"], 2, 100).measure(c["depth"][:3], c["mpp"][:3], c["eps"])       # batch > max_batch
    with pytest.raises(ValueError):
        pkg.CloudReadout(*c["shape"], 2, 100).measure(c["depth"][:2, :-1], c["mpp"][:2], c["eps"])


# ---------------------------------------------------------------------------------------------------------------- GPU, through the session
def _session(pkg, n, max_batch):
    model, neg = pkg.load_calibration(os.path.join(G, "calibration_phase_to_height.json"))
    fm = pkg.load_force_calibration(os.path.join(G, "calibration_height_to_force.json"))["best_model"]
    return pkg.FtpSensor(pkg.synth.reference_frame(n), pkg.synth.roi_circle(n), pkg.FtpConfig.scaled(n), model, neg, fm, max_batch=max_batch)


@pytest.mark.gpu
def test_session_cloud_and_predict_argument(pkg):
    import torch
    import contacts_helpers as CH
    n, nb = 224, 4
    s = _session(pkg, n, nb)
    with pytest.raises(RuntimeError):
        s.cloud()                                                                                   # no predict yet
    o = s.predict_batch(CH.multi_contact_batch(pkg, n, 0, nb))
    before = {k: v.clone() for k, v in o.items()}
    r = s.cloud()
    assert set(r) == {"points", "pixel", "offsets", "frame"} and tuple(r["frame"].shape) == (nb, 12)
    assert s._cloud.max_points == n * n and tuple(r["points"].shape) == (n * n, 8)                    # the larger of one frame and an eighth of nb
    r = s.cloud(max_points=nb * n * n, labels=True)                                                  # room for every pixel: no overflow
    torch.cuda.synchronize()
    assert set(r) == {"points", "pixel", "label", "offsets", "frame"} and s._cloud.max_points == nb * n * n
    t = s._cloud.trim(r)
    print("surface pixels", r["frame"][:, 0].tolist(), "total", t["total"])
    assert not t["overflow"] and t["total"] == len(t["points"]) == len(t["pixel"]) == len(t["label"]) > 100
    sc, hm = o["scalars"].cpu().numpy(), o["height_map_mm"].cpu().numpy()
    mpp = sc[:, pkg.SCALAR_NAMES.index("mm_per_px")]
    idx = s.contacts(8, index_plane=True)["contact_index"].cpu().numpy()
    pts, pix, lab, off, fr = (t[k].cpu().numpy() for k in ("points", "pixel", "label", "offsets", "frame"))
    assert (o["status"].cpu().numpy() == 0).all()
    for b in range(nb):
        area = sc[b, pkg.SCALAR_NAMES.index("contact_area_mm2")]
        assert fr[b, F_["surface_pixels"]] == round(area / (mpp[b] * mpp[b])) == off[b + 1] - off[b] > 0   # the tail's contact pixels
        p = pix[off[b]:off[b + 1]]
        assert np.array_equal(lab[off[b]:off[b + 1]], idx[b].ravel()[p])                              # the index plane at the pixel
        assert CL.same_bits(-pts[off[b]:off[b + 1], 2], hm[b].ravel()[p])                             # -Z is the height map at the pixel
    length = np.sqrt((pts[:, 3:6].astype(np.float64) ** 2).sum(axis=1))
    assert np.abs(length - 1.0).max() <= 2.0 * 2.0 ** -23                                             # unit normals within 2 float32 ulps
    want = CL.numpy_cloud(hm, mpp, s.config.depth_eps_mm, o["status"].cpu().numpy(), idx)
    assert CL.same_bits(pts, want["points"]) and np.array_equal(pix, want["pixel"]) and np.array_equal(off, want["offsets"])
    assert all(CL.same_bits(o[k].cpu().numpy(), before[k].cpu().numpy()) for k in o)                 # the predict's tensors are what they were
    first = s._cloud
    s.cloud(max_points=nb * n * n, labels=True)
    assert s._cloud is first
    small = s.cloud(max_points=50, stride=2)
    assert s._cloud is not first and "label" not in small and s._cloud.trim(small)["overflow"]       # rebuilt; overflow reported, not raised
    assert int(small["offsets"][-1]) > 50 and len(s._cloud.trim(small)["points"]) == 50
    s.close()
    assert s._cloud is None
    s = _session(pkg, n, 1)
    frame = pkg.synth.deformed_frame(n, 0)
    plain = s.predict(frame)
    res = s.predict(frame, cloud=dict(stride=2))
    assert set(res) == set(plain) | {"cloud", "cloud_pixel", "cloud_frame"} and set(s.predict(frame)) == set(plain)
    assert not {"cloud", "cloud_pixel", "cloud_frame"} & set(plain)
    assert res["cloud"].dtype == np.float32 and res["cloud"].shape == (len(res["cloud_pixel"]), 8) and len(res["cloud_pixel"]) > 10
    assert list(res["cloud_frame"]) == list(pkg.CLOUD_FRAME_NAMES) and res["cloud_frame"]["points"] == len(res["cloud_pixel"])
    assert ((res["cloud_pixel"] % n) % 2 == 0).all() and ((res["cloud_pixel"] // n) % 2 == 0).all()
    assert CL.same_bits(-res["cloud"][:, 2], plain["height_map_mm_crop"].ravel()[res["cloud_pixel"]])
    assert "cloud_label" in s.predict(frame, cloud=dict(labels=True))
    s.close()
