"""The camera-native input formats (VISTAF_FMT_RGB_U8 .. VISTAF_FMT_BAYER_BGGR_U8, include/vistaf_ftp.h): RGB(A), packed YUV 4:2:2, NV12 and
the four Bayer mosaics.

The definitions of the header's table are restated here in NumPy (`gray_of_frames`; the demosaic through np.pad(..., mode="reflect")) and the
restatement is itself pinned by a 4 x 4 mosaic worked out by hand.  Every format lands on the plane GRAY_U8 lands on, so the whole
correctness statement is "the bits of the equivalent GRAY_U8 frame": the gray plane (`intermediate("img")` with the bad-pixel stage off is
exactly what launch_to_gray wrote) bit for bit, and every output of a predict bit for bit.  There is no tolerance anywhere in this file.
The Bayer demosaic is the project's own definition (the reference never sees a mosaic): its parity is unpinned.

Sizes: 64 x 64; 151 x 203 (odd both ways: ragged quads, all four borders and corners, more than one block); 151 x 202 for the 4:2:2 formats
(frame stride = 4 mod 8) and 150 x 202 for NV12 (frame stride = 2 mod 4), so the frames behind the first hold no more than the format's
own alignment; and each once more from a view that starts 4 bytes (formats 5..8) or 1 byte (the others) into its storage."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
NEW = ["rgb", "bgra", "rgba", "yuyv", "uyvy", "nv12", "bayer_rggb", "bayer_grbg", "bayer_gbrg", "bayer_bggr"]
ALL = ["gray", "bgr", "gray_f16", "bgr_f16"] + NEW
PERIOD_160 = 65.83619546657023 * 160 / 1182            # the fringe period of the 151 x 203 scenes of test_config_surface
CIRCLE_ODD = (98, 74, 66)                              # their ROI: off centre, touching no border of 150..151 x 202..203


# ---- the header's table in NumPy ----------------------------------------------------------------------------------------------------------
def GRAY(b, g, r):
    b, g, r = (np.asarray(v).astype(np.int64) for v in (b, g, r))
    return (b * 3735 + g * 19235 + r * 9798 + 16384) >> 15


def demosaic_gray(m, pattern):
    """m [h,w] uint8, pattern the colours of the top-left 2 x 2 block in reading order ("rggb", ...): the header's demosaic, then GRAY"""
    h, w = m.shape
    p = np.pad(m.astype(np.int64), 1, mode="reflect")
    C, N, S, W, E = p[1:-1, 1:-1], p[:-2, 1:-1], p[2:, 1:-1], p[1:-1, :-2], p[1:-1, 2:]
    NW, NE, SW, SE = p[:-2, :-2], p[:-2, 2:], p[2:, :-2], p[2:, 2:]
    cross, diag, hor, ver = (N + S + W + E + 2) >> 2, (NW + NE + SW + SE + 2) >> 2, (W + E + 1) >> 1, (N + S + 1) >> 1
    yy, xx = np.mgrid[:h, :w]
    site = np.array(list(pattern)).reshape(2, 2)[yy & 1, xx & 1]
    red_row = (yy & 1) == pattern.index("r") // 2
    r = np.select([site == "r", site == "b", red_row], [C, diag, hor], ver)
    g = np.where(site == "g", C, cross)
    b = np.select([site == "b", site == "r", red_row], [C, diag, ver], hor)
    return GRAY(b, g, r)


def gray_of_frames(frames, fmt, h, w):
    """[B, ...] frames in `fmt` (the shapes of ftp.frame_layout) -> [B,h,w] uint8, the equivalent GRAY_U8 frames"""
    f = np.asarray(frames)
    if fmt == "rgb" or fmt == "rgba":
        g = GRAY(f[..., 2], f[..., 1], f[..., 0])
    elif fmt == "bgra":
        g = GRAY(f[..., 0], f[..., 1], f[..., 2])
    elif fmt in ("yuyv", "uyvy"):
        g = f.reshape(f.shape[0], h, w // 2, 4)[..., [0, 2] if fmt == "yuyv" else [1, 3]].reshape(f.shape[0], h, w)
    elif fmt == "nv12":
        g = f.reshape(f.shape[0], 3 * h // 2, w)[:, :h]
    else:
        g = np.stack([demosaic_gray(m, fmt[len("bayer_"):]) for m in f])
    assert g.shape == (f.shape[0], h, w) and g.min() >= 0 and g.max() <= 255
    return g.astype(np.uint8)


def frames_around(gray, fmt, rng, spread=6):
    """frames in `fmt` whose planes follow `gray` [B,h,w] uint8: colour channels and mosaic sites within +-spread of it, the Y of a YUV
    frame equal to it; alpha and chroma are random bytes"""
    B, h, w = gray.shape

    def near(shape_tail=()):
        return np.clip(gray.reshape(B, h, w, *([1] * len(shape_tail))).astype(np.int32) + rng.integers(-spread, spread + 1, size=(B, h, w) + shape_tail), 0,
                       255).astype(np.uint8)
    if fmt == "rgb":
        return near((3,))
    if fmt in ("bgra", "rgba"):
        f = rng.integers(0, 256, size=(B, h, w, 4), dtype=np.uint8)
        f[..., :3] = near((3,))
        return f
    if fmt in ("yuyv", "uyvy"):
        f = rng.integers(0, 256, size=(B, h, w // 2, 4), dtype=np.uint8)
        f[..., [0, 2] if fmt == "yuyv" else [1, 3]] = gray.reshape(B, h, w // 2, 2)
        return f
    if fmt == "nv12":
        f = rng.integers(0, 256, size=(B, 3 * h // 2, w), dtype=np.uint8)
        f[:, :h] = gray
        return f
    return near()


# ---- without a device ---------------------------------------------------------------------------------------------------------------------
def test_formats_table_matches_the_header(pkg):
    hdr = open(os.path.join(ROOT, "include", "vistaf_ftp.h")).read()
    defines = re.findall(r"^#define VISTAF_FMT_(\w+)\s+(\d+)", hdr, flags=re.M)
    assert len(defines) == 14
    want = {(name[:-3] if name.endswith("_U8") else name).lower(): int(code) for name, code in defines}
    assert pkg._lib.FORMATS == want and list(pkg._lib.FORMATS) == ALL and sorted(want.values()) == list(range(14))
    for name, code in defines:
        assert getattr(pkg._lib, "FMT_" + name) == int(code)


def test_frame_layout(pkg):
    fl, u8, f16 = pkg.ftp.frame_layout, torch.uint8, torch.float16
    h, w = 150, 202
    want = {"gray": ((h, w), u8, h * w), "bgr": ((h, w, 3), u8, 3 * h * w), "gray_f16": ((h, w), f16, 2 * h * w), "bgr_f16": ((h, w, 3), f16, 6 * h * w),
            "rgb": ((h, w, 3), u8, 3 * h * w), "bgra": ((h, w, 4), u8, 4 * h * w), "rgba": ((h, w, 4), u8, 4 * h * w),
            "yuyv": ((h, w // 2, 4), u8, 2 * h * w), "uyvy": ((h, w // 2, 4), u8, 2 * h * w), "nv12": ((3 * h // 2, w), u8, 45450)}
    want.update({"bayer_" + p: ((h, w), u8, h * w) for p in ("rggb", "grbg", "gbrg", "bggr")})
    assert sorted(want) == sorted(ALL)
    for name, expect in want.items():
        assert fl(name, h, w) == expect, name
        assert fl(pkg._lib.FORMATS[name], h, w) == expect, name
    assert fl("yuyv", 151, 202) == ((151, 101, 4), u8, 61004) and 61004 % 8 == 4 and 45450 % 4 == 2
    for name in ("rgb", "bgra", "rgba", "bayer_rggb", "bayer_grbg", "bayer_gbrg", "bayer_bggr"):
        assert fl(name, 151, 203)[2] == 151 * 203 * {"rgb": 3, "bgra": 4, "rgba": 4}.get(name, 1)          # odd sizes are legal
    assert fl("bayer_bggr", 2, 2) == ((2, 2), u8, 4)
    for name, hh, ww in (("yuyv", 151, 203), ("uyvy", 64, 63), ("nv12", 151, 202), ("nv12", 150, 203), ("nv12", 151, 203), ("bayer_rggb", 1, 8),
                         ("bayer_gbrg", 8, 1), ("gray", 0, 8)):
        with pytest.raises(ValueError):
            fl(name, hh, ww)
    for bad in ("nv21", "YUYV", "", 14, -1, 4.0, None, True):
        with pytest.raises(ValueError):
            fl(bad, 64, 64)


def test_reference_size_from_its_shape(pkg):
    size, F = pkg.ftp._frame_size, pkg._lib.FORMATS
    assert size(F["rgb"], (151, 203, 3)) == (151, 203) and size(F["rgba"], (1, 151, 203, 4)) == (151, 203)
    assert size(F["yuyv"], (151, 101, 4)) == (151, 202) and size(F["uyvy"], (151, 404)) == (151, 202) and size(F["yuyv"], (1, 151, 101, 4)) == (151, 202)
    assert size(F["nv12"], (225, 202)) == (150, 202) and size(F["bayer_grbg"], (1, 151, 203)) == (151, 203)
    for code, shape in ((F["rgb"], (151, 203)), (F["yuyv"], (151, 203)), (F["nv12"], (224, 202)), (F["nv12"], (45450,)), (F["bayer_rggb"], (2, 151, 203))):
        with pytest.raises(ValueError):
            size(code, shape)


MOSAIC = np.array([[10, 200, 30, 90], [120, 60, 250, 0], [70, 180, 20, 140], [255, 40, 110, 230]], dtype=np.uint8)
# worked out by hand from the header's table.  E.g. rggb (0,0), a red site: r = 10; N = S = 120 (row -1 is row 1), W = E = 200, so
# g = (640 + 2) >> 2 = 160; all four diagonals are (1,1) = 60, so b = 60; GRAY = (224100 + 3077600 + 97980 + 16384) >> 15 = 104.  rggb (0,3),
# a green site beside red: g = 90, r = (30 + 30 + 1) >> 1 = 30 (column 4 is column 2), b = (0 + 0 + 1) >> 1 = 0; GRAY = 62.
BY_HAND = {
    "rggb": [[104, 130, 129, 62], [89, 127, 158, 115], [135, 125, 115, 101], [175, 124, 86, 106]],
    "grbg": [[79, 104, 89, 64], [100, 113, 91, 63], [116, 103, 80, 102], [115, 98, 106, 189]],
    "gbrg": [[65, 102, 109, 94], [87, 112, 109, 88], [118, 104, 84, 110], [129, 99, 97, 184]],
    "bggr": [[113, 138, 129, 56], [93, 132, 159, 110], [131, 126, 127, 119], [170, 123, 107, 144]],
}


@pytest.mark.parametrize("pattern", sorted(BY_HAND))
def test_inline_demosaic_against_the_hand_computed_mosaic(pattern):
    assert demosaic_gray(MOSAIC, pattern).tolist() == BY_HAND[pattern]


def test_inline_packed_definitions():
    px = np.array([[[[10, 200, 30, 77]]]], dtype=np.uint8)                                 # one pixel, four bytes
    assert gray_of_frames(px[..., :3], "rgb", 1, 1).item() == (30 * 3735 + 200 * 19235 + 10 * 9798 + 16384) >> 15 == 124
    assert gray_of_frames(px, "rgba", 1, 1).item() == 124 and gray_of_frames(px, "bgra", 1, 1).item() == (10 * 3735 + 200 * 19235 + 30 * 9798 + 16384) >> 15
    assert gray_of_frames(px, "yuyv", 1, 2).tolist() == [[[10, 30]]] and gray_of_frames(px, "uyvy", 1, 2).tolist() == [[[200, 77]]]
    nv = np.arange(12, dtype=np.uint8).reshape(1, 3, 4)
    assert gray_of_frames(nv, "nv12", 2, 4).tolist() == [[[0, 1, 2, 3], [4, 5, 6, 7]]]


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cal(pkg):
    model, neg = pkg.load_calibration(os.path.join(G, "calibration_phase_to_height.json"))
    return model, neg, pkg.load_force_calibration(os.path.join(G, "calibration_height_to_force.json"))["best_model"]


def _fringes(h, w, period, seed):
    rng = np.random.default_rng(seed)
    xx = np.arange(w, dtype=np.float64)[None, :]
    return np.clip(np.rint(128.0 * (0.55 + 0.35 * np.cos(2.0 * np.pi * xx / period)) + rng.normal(0.0, 2.0, size=(h, w))), 0, 255).astype(np.uint8)


_PLANE_SESSIONS = {}


@pytest.fixture(scope="module")
def plane_session(pkg, cal):
    """sessions of the gray-plane tests, one per size, bad-pixel stage off so that "img" is launch_to_gray's output untouched"""
    def get(h, w):
        if (h, w) not in _PLANE_SESSIONS:
            if h == w:
                cfg, ref, circle = pkg.FtpConfig.scaled(h), pkg.synth.reference_frame(h), pkg.synth.roi_circle(h)
            else:
                cfg, ref, circle = pkg.FtpConfig.scaled(160), _fringes(h, w, PERIOD_160, 11), CIRCLE_ODD
            cfg.bad_pixel_enable = 0
            _PLANE_SESSIONS[(h, w)] = pkg.FtpSensor(ref, circle, cfg, *cal, max_batch=3)
        return _PLANE_SESSIONS[(h, w)]
    yield get
    for s in _PLANE_SESSIONS.values():
        s.close()
    _PLANE_SESSIONS.clear()


def _odd_size(fmt):
    return {"yuyv": (151, 202), "uyvy": (151, 202), "nv12": (150, 202)}.get(fmt, (151, 203))


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", NEW)
def test_gray_plane_bit_for_bit(pkg, plane_session, fmt):
    B = 3
    code = pkg._lib.FORMATS[fmt]
    off = 4 if 5 <= code <= 8 else 1
    for (h, w) in ((64, 64), _odd_size(fmt)):
        sensor = plane_session(h, w)
        shape, dtype, nbytes = pkg.ftp.frame_layout(fmt, h, w)
        frames = np.random.default_rng(100 * code + h).integers(0, 256, size=(B,) + shape, dtype=np.uint8)      # chroma and alpha are garbage
        want = gray_of_frames(frames, fmt, h, w).astype(np.float32)
        store = torch.zeros(B * nbytes + off, dtype=torch.uint8, device="cuda")
        store[off:] = torch.from_numpy(frames).reshape(-1).cuda()
        view = store[off:].view(B, *shape)
        assert view.data_ptr() % (2 * off) == off                   # no more than the promised alignment: 4 mod 8, or odd
        for name, given in (("aligned", frames), ("view", view), ("code", torch.from_numpy(frames).cuda())):
            sensor.predict_batch(given, format=code if name == "code" else fmt)
            got = sensor.intermediate("img", B).cpu().numpy().reshape(B, h, w)
            bad = np.argwhere(got != want)
            assert bad.size == 0, (fmt, h, w, name, len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
        # one frame without the batch dimension, and the flat spellings of the packed layouts
        alts = [frames[0]]
        if fmt in ("yuyv", "uyvy"):
            alts.append(frames.reshape(B, h, 2 * w))
        if fmt == "nv12":
            alts.append(frames.reshape(B, nbytes))
        for given in alts:
            sensor.predict_batch(given, format=fmt)
            n = 1 if given is alts[0] else B
            assert np.array_equal(sensor.intermediate("img", n).cpu().numpy().reshape(n, h, w), want[:n])


def _same(a, b):
    torch.cuda.synchronize()
    for key in ("height_map_mm", "output_reliable", "scalars", "status"):
        x, y = a[key].cpu().numpy(), b[key].cpu().numpy()
        assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), key


@pytest.fixture(scope="module")
def scene(pkg):
    n, nb = 128, 2
    return n, nb, pkg.FtpConfig.scaled(n), pkg.synth.reference_frame(n), pkg.synth.deformed_batch(n, 7, nb), pkg.synth.roi_circle(n)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", NEW)
def test_end_to_end_equals_the_gray_frames(pkg, cal, scene, fmt):
    n, nb, cfg, ref, g, circle = scene
    rng = np.random.default_rng(pkg._lib.FORMATS[fmt])
    ref_x, frames = frames_around(ref[None], fmt, rng)[0], frames_around(g, fmt, rng)
    ref_g, gray_u8 = gray_of_frames(ref_x[None], fmt, n, n)[0], gray_of_frames(frames, fmt, n, n)
    if fmt in ("yuyv", "uyvy", "nv12"):
        assert np.array_equal(gray_u8, g)
    else:
        assert not np.array_equal(gray_u8, g)                                                       # perturbed: the conversion has work to do
    sensor = pkg.FtpSensor(ref_x, circle, cfg, *cal, max_batch=nb, format=fmt)
    plain = pkg.FtpSensor(ref_g, circle, cfg, *cal, max_batch=nb)
    assert (sensor.h, sensor.w) == (n, n) and sensor.reference_info == plain.reference_info
    a = sensor.predict_batch(frames, format=fmt)
    assert set(a["status"].tolist()) == {0}
    _same(a, sensor.predict_batch(gray_u8))
    _same(a, plain.predict_batch(gray_u8))
    one = sensor.predict(frames[1], format=fmt)
    assert np.array_equal(one["height_map_mm_crop"], a["height_map_mm"][1].cpu().numpy(), equal_nan=True)
    sensor.close()
    plain.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,max_batch", [("yuyv", 4), ("bayer_grbg", 4), ("bayer_grbg", 2)])
def test_pairs_equal_the_gray_pairs(pkg, cal, scene, fmt, max_batch):
    """max_batch 4: both frame sets go through the same launches, the second launch_to_gray writing behind the first; 2: one after the other"""
    n, nb, cfg, ref, g, circle = scene
    rng = np.random.default_rng(50 + pkg._lib.FORMATS[fmt])
    refs = frames_around(np.stack([ref, pkg.synth.reference_frame(n, config=1)]), fmt, rng)
    frames = frames_around(g, fmt, rng)
    sensor = pkg.FtpSensor(None, circle, cfg, *cal, max_batch=max_batch, frame_shape=(n, n))
    a = sensor.predict_pairs(refs, frames, format=fmt)
    info = sensor.pair_info(nb)
    assert set(a["status"].tolist()) == {0}
    _same(a, sensor.predict_pairs(gray_of_frames(refs, fmt, n, n), gray_of_frames(frames, fmt, n, n)))
    assert sensor.pair_info(nb) == info
    with pytest.raises(ValueError):
        sensor.predict_pairs(refs, frames[:1], format=fmt)
    sensor.close()


@pytest.mark.gpu
def test_refusals_on_a_live_handle(pkg, plane_session):
    lib = pkg._lib.load()

    def raw(sensor, buf, code):
        out = sensor._new_out(2)
        rc = lib.vistaf_ftp_predict_batch(sensor._h, buf.data_ptr(), code, 2, out["height_map_mm"].data_ptr(), out["output_reliable"].data_ptr(),
                                          out["scalars"].data_ptr(), out["status"].data_ptr(), None)
        return rc, lib.vistaf_ftp_last_error().decode()
    for (h, w), fmt, word in (((151, 203), "yuyv", "YUYV"), ((151, 203), "uyvy", "UYVY"), ((151, 202), "nv12", "NV12")):
        sensor = plane_session(h, w)
        frames = np.stack([_fringes(h, w, PERIOD_160, 21), _fringes(h, w, PERIOD_160, 22)])
        before = sensor.predict_batch(frames)
        buf = torch.zeros(2 * 4 * h * w + 8, dtype=torch.uint8, device="cuda")                           # room for two frames of any 8-bit format
        with pytest.raises(ValueError, match=fmt):
            sensor.predict_batch(buf[:2 * 2 * h * w].view(2, h, -1), format=fmt)                         # refused before the library is called ...
        rc, msg = raw(sensor, buf, pkg._lib.FORMATS[fmt])
        assert rc == -1 and word in msg                                                                  # ... and by the library itself
        for bad in (14, -1, 255):
            with pytest.raises(ValueError):
                sensor.predict_batch(frames, format=bad)
            rc, msg = raw(sensor, buf, bad)
            assert rc == -1 and "format" in msg
        with pytest.raises(ValueError, match="nv21"):
            sensor.predict_batch(frames, format="nv21")
        with pytest.raises(ValueError):
            sensor.predict_batch(frames[:, :-1], format="bayer_rggb")                                    # not the session's size
        with pytest.raises(ValueError):
            sensor.predict_batch(frames.astype(np.float16), format="bayer_rggb")                         # not the format's dtype
        rc, msg = raw(sensor, buf[2:], pkg._lib.FORMATS["bgra"])                                         # below the 4 bytes BGRA owes
        assert rc == -1 and "aligned" in msg
        _same(before, sensor.predict_batch(frames))                                                      # the session is none the worse


@pytest.mark.gpu
def test_decoded_formats_unchanged_by_an_explicit_format(pkg, plane_session):
    n, B = 64, 3
    sensor = plane_session(n, n)
    g = pkg.synth.deformed_batch(n, 3, B)
    bgr = np.clip(np.repeat(g[..., None], 3, axis=-1).astype(np.int32) + np.random.default_rng(4).integers(-6, 7, size=(B, n, n, 3)), 0, 255).astype(np.uint8)
    given = {"gray": g, "bgr": bgr, "gray_f16": torch.from_numpy(g).to(torch.float16), "bgr_f16": torch.from_numpy(bgr).to(torch.float16)}
    for code, (name, frames) in enumerate(given.items()):
        a = sensor.predict_batch(frames)
        img = sensor.intermediate("img", B).clone()
        for fmt in (name, code):
            _same(a, sensor.predict_batch(frames, format=fmt))
            assert torch.equal(img, sensor.intermediate("img", B))
        with pytest.raises(ValueError):
            sensor.predict_batch(frames, format="bgr" if name == "gray" else "gray")
