"""The temperature modality end to end (tempsensor.py, include/vistaf_tempsensor.h) and its NumPy-exact map statistics.

CPU: the C ABI's export list and argument checks, the default constants.  GPU: the statistics against writers.temperature_statistics by bit
pattern; the chain against the public stage calls in sequence, bit for bit; the map stages against the oracle on the GPU model maps; the
reference-held pins on FINAL_E (stored masks, number of valid pixels); one session reused over several frames.
Models come from tests/golden/tempmodel_fixture.npz: a 4-feature wide model and a 3-feature colour model whose isotonic step is NaN out of
bounds, its table narrowed to [36.5, 39.5] so that the colour map has holes to inpaint.
"""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from oracle import align_oracle as A
from oracle import temp_oracle as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
HDR = os.path.join(ROOT, "include", "vistaf_tempsensor.h")
WIDE, COLOR = "labg_d3_nobias", "lab_d2_nan"
STAT_KEYS = ("mean_C", "median_C", "std_C", "min_C", "max_C", "valid_pixels")


def _models(pkg):
    z = np.load(os.path.join(G, "tempmodel_fixture.npz"))
    models = json.loads(str(z["models_json"]))
    cd = json.loads(json.dumps(models[COLOR]))
    iso = cd["isotonic"]          # the synthetic frames' colour predictions lie inside the table: narrow it so that some fall outside
    keep = [i for i, x in enumerate(iso["x_thresholds"]) if 36.5 <= x <= 39.5]
    iso["x_thresholds"], iso["y_thresholds"] = [iso["x_thresholds"][i] for i in keep], [iso["y_thresholds"][i] for i in keep]
    wide, col = pkg.TempModel.from_dict(models[WIDE]), pkg.TempModel.from_dict(cd)
    assert len(wide.features) == 4 and len(col.features) == 3 and col.isotonic["out_of_bounds"] == "nan"
    return wide, col


def _frame(h, w, seed):
    """stripes of period ~20 px under a slow illumination field, a saturated blob and a colour tint that varies across the frame"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    s = 1.0 + 0.2 * np.cos(np.pi * np.hypot(xx - w / 2, yy - h / 2) / (0.7 * w))
    g = 120.0 * s * (0.6 + 0.3 * np.sign(np.cos(2 * np.pi * (xx + 0.08 * yy) / 20.3))) + rng.normal(0, 3.0, (h, w))
    g[(xx - 0.62 * w) ** 2 + (yy - 0.4 * h) ** 2 <= 14 ** 2] = 255.0
    t = 0.5 + 0.5 * np.sin(xx / 41.0 + 0.7 * seed) * np.cos(yy / 53.0)
    img = np.stack([g * (0.75 + 0.5 * t), g, g * (1.25 - 0.5 * t)], axis=-1)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def _disc(h, w, frac=0.45):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((yy - h / 2) ** 2 + (xx - w / 2) ** 2) < (frac * min(h, w)) ** 2


def _same_stats(got, want):
    """equal to the last bit (NaN == NaN), keys in the same order"""
    assert list(got) == list(want) == list(STAT_KEYS)
    assert got["valid_pixels"] == want["valid_pixels"]
    for k in STAT_KEYS[:5]:
        a, b = np.float64(got[k]), np.float64(want[k])
        assert (np.isnan(a) and np.isnan(b)) or a.view(np.int64) == b.view(np.int64), (k, float(a), float(b))


def _bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int32), np.asarray(b).view(np.int32))


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------
def test_header_functions_are_exported(pkg):
    decl = re.findall(r"\b(vistaf_tsensor_\w+)\s*\(", open(HDR).read())
    names = list(dict.fromkeys(decl))
    assert names == pkg._lib.TSENSOR_EXPORTS
    lib = pkg._lib.load()
    for n in names:
        getattr(lib, n)


def test_default_config_is_the_shipped_constants(pkg):
    lib = pkg._lib.load()
    c = pkg._lib.CTSensorConfig()
    assert lib.vistaf_tsensor_default_config(ctypes.byref(c)) == 0
    py = pkg.TempSensorConfig()
    for f in ("seg_band_radius", "seg_dc_exclusion", "seg_illum_sigma", "sat_thresh_gray", "sat_dilate_ksize", "post_close_kx", "post_close_ky",
              "post_open_kx", "post_open_ky", "n_peaks", "seg_peak_max_dy_from_center"):
        assert getattr(c.seg, f) == getattr(T.TempSegConfig(), f) == getattr(py.seg, f), f
    assert (c.fuse.color_t_min, c.fuse.color_t_max) == (T.COLOR_T_MIN, T.COLOR_T_MAX) == (py.color_t_min, py.color_t_max)
    assert (c.fuse.color_guard_band, c.fuse.switch_margin_c) == (T.COLOR_GUARD_BAND, T.SWITCH_MARGIN_C) == (py.color_guard_band, py.switch_margin_c)
    assert (c.fuse.final_t_min, c.fuse.final_t_max) == (T.FINAL_T_MIN, T.FINAL_T_MAX) == (py.final_t_min, py.final_t_max)
    assert (c.smooth_sigma_across, c.smooth_sigma_along) == (T.FINAL_SMOOTH_SIGMA_ACROSS, T.FINAL_SMOOTH_SIGMA_ALONG) == \
        (py.smooth_sigma_across, py.smooth_sigma_along)
    assert c.blur_ksize == T.TempSegConfig().blur_ksize == pkg.tempseg.BLUR_KSIZE == py.blur_ksize
    assert c.color_chroma_min == T.TempSegConfig().color_chroma_min == pkg.tempseg.COLOR_CHROMA_MIN == py.color_chroma_min
    assert c.color_support_dilate == T.TempSegConfig().color_support_dilate == pkg.tempseg.COLOR_SUPPORT_DILATE == py.color_support_dilate
    # main() :835-845: inpaint radii 7 (wide) and 5 (colour), colour clamp band COLOR_T_MIN - 5 .. COLOR_T_MAX + 5
    assert (c.wide_inpaint_radius, c.color_inpaint_radius, c.color_clamp_pad) == (7, 5, 5.0) == \
        (py.wide_inpaint_radius, py.color_inpaint_radius, py.color_clamp_pad)
    for f, _ in pkg._lib.CTSensorConfig._fields_[2:]:
        assert getattr(c, f) == getattr(py.to_c(), f), f


def test_create_refuses_bad_arguments_before_device_work(pkg):
    lib = pkg._lib.load()
    c = pkg._lib.CTSensorConfig()
    lib.vistaf_tsensor_default_config(ctypes.byref(c))
    dummy = ctypes.create_string_buffer(64)          # never dereferenced: every check below returns first
    fake = ctypes.cast(dummy, ctypes.c_void_p)
    h = ctypes.c_void_p()

    def refused(H, W, wm, cm, what):
        rc = lib.vistaf_tsensor_create(ctypes.byref(c), H, W, wm, cm, ctypes.byref(h))
        assert rc == -1 and not h.value
        msg = lib.vistaf_ftp_last_error().decode()
        assert what in msg, msg

    refused(256, 320, None, fake, "model")
    refused(256, 320, fake, None, "model")
    refused(250, 320, fake, fake, "multiple of 16")
    refused(48, 320, fake, fake, "multiple of 16")
    refused(256, 63, fake, fake, ">= 64")
    c.wide_inpaint_radius = 0
    refused(256, 320, fake, fake, "inpaint radius")
    lib.vistaf_tsensor_default_config(ctypes.byref(c))
    c.blur_ksize = 3
    refused(256, 320, fake, fake, "blur_ksize")
    s = ctypes.c_void_p()
    assert lib.vistaf_tsensor_stats_create(0, 5, ctypes.byref(s)) == -1 and not s.value
    assert lib.vistaf_tsensor_map_statistics(None, None, None, None, None, None) == -1


# ---- GPU: statistics ------------------------------------------------------------------------------------------------------------------
def _masked_case(h, w, n, seed, mode):
    """a map with exactly n valid pixels: ties and repeated values, negatives; NaN (and +-inf) outside the mask"""
    rng = np.random.default_rng(seed)
    m = (rng.standard_normal((h, w)) * 7.0 + 25.0).astype(np.float32)
    if mode == "ties":
        m = (np.round(m * 4.0) / 4.0).astype(np.float32)
    elif mode == "negative":
        m = (m - 40.0).astype(np.float32)
    elif mode == "const":
        m[:] = np.float32(-3.125)
    valid = np.zeros(h * w, bool)
    valid[rng.choice(h * w, size=n, replace=False)] = True
    valid = valid.reshape(h, w)
    out = ~valid
    m[out & (rng.random((h, w)) < 0.5)] = np.nan
    m[out & (rng.random((h, w)) < 0.05)] = np.inf
    return m, valid


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 127, 128, 129, 136, 255, 256, 1000, 4095, 4096, 4097])
def test_gpu_map_statistics_match_numpy_bit_for_bit(pkg, n):
    for seed, mode in ((n, "plain"), (n + 1, "ties"), (n + 2, "negative"), (n + 3, "const")):
        m, valid = _masked_case(151, 203, n, seed, mode)
        _same_stats(pkg.map_statistics(m, valid), pkg.temperature_statistics(m, valid))
        # isfinite mode: the same pixels valid, everything else NaN
        mf = np.where(valid, m, np.float32(np.nan)).astype(np.float32)
        _same_stats(pkg.map_statistics(mf), pkg.temperature_statistics(mf, np.isfinite(mf)))


@pytest.mark.gpu
def test_gpu_map_statistics_edges(pkg):
    import torch
    one = np.array([[36.6]], np.float32)
    _same_stats(pkg.map_statistics(one), pkg.temperature_statistics(one, np.isfinite(one)))
    nan1 = np.array([[np.nan]], np.float32)
    _same_stats(pkg.map_statistics(nan1), pkg.temperature_statistics(nan1, np.isfinite(nan1)))
    _same_stats(pkg.map_statistics(one, np.zeros((1, 1), bool)), pkg.temperature_statistics(one, np.zeros((1, 1), bool)))
    # a NaN inside an explicit mask: NumPy's statistics are NaN, the count is the mask's
    m, valid = _masked_case(151, 203, 1000, 5, "plain")
    m[valid.nonzero()[0][17], valid.nonzero()[1][17]] = np.nan
    _same_stats(pkg.map_statistics(m, valid), pkg.temperature_statistics(m, valid))
    # a zero median from -0 values, mixed magnitudes (pairwise summation order matters), device tensors in
    z = np.full((64, 64), -0.0, np.float32)
    _same_stats(pkg.map_statistics(z), pkg.temperature_statistics(z, np.isfinite(z)))
    rng = np.random.default_rng(3)
    big = (rng.standard_normal((151, 203)) * np.float32(1e4) + rng.standard_normal((151, 203)) * 1e-3).astype(np.float32)
    _same_stats(pkg.map_statistics(torch.from_numpy(big).cuda()), pkg.temperature_statistics(big, np.isfinite(big)))


@pytest.mark.gpu
def test_gpu_map_statistics_photograph_roi(pkg):
    """3840 x 2160 with the photograph's ROI disc (1 576 625 pixels): the multi-kernel selection and ~190 summation buffers"""
    h, w = 2160, 3840
    roi = pkg.tempseg.roi_mask_from_circle(h, w, *pkg.tempseg.OUTER_CIRCLE)
    assert int(roi.sum()) == 1576625
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:h, 0:w]
    m = (20.0 + 11.0 * np.sin(xx / 300.0) ** 2 + 0.05 * rng.standard_normal((h, w))).astype(np.float32)
    m = np.maximum(m, np.float32(20.0))                                            # many ties at the clamp floor, as a final map has
    mf = np.where(roi, m, np.float32(np.nan)).astype(np.float32)
    _same_stats(pkg.map_statistics(mf), pkg.temperature_statistics(mf, np.isfinite(mf)))
    _same_stats(pkg.map_statistics(m, roi), pkg.temperature_statistics(m, roi))
    even = roi.copy()
    even[roi.nonzero()[0][0], roi.nonzero()[1][0]] = False                          # an even count: two middle values
    _same_stats(pkg.map_statistics(m, even), pkg.temperature_statistics(m, even))


# ---- GPU: the chain -------------------------------------------------------------------------------------------------------------------
def _stages(pkg, img, roi, wide_m, col_m, seg=None):
    """temperature_sensor.main() as the existing public stage calls, with their host round trips (a fresh segmentation session unless
    one is passed)"""
    h, w = img.shape[:2]
    own = seg is None
    seg = seg or pkg.TempSegmenter(h, w)
    dark, light, pack = seg.segment(img, roi)
    planes = seg.feature_planes_device(img)
    support, _ = seg.color_support(planes, light, pack["roi_eff"], pack["sat"])
    wide_raw, color_raw = pkg.predict_maps(planes, (wide_m, pack["roi_eff"]), (col_m, support))
    wide_raw, color_raw = wide_raw.cpu().numpy(), color_raw.cpu().numpy()
    wide = seg.clamp_map(seg.inpaint_temperature_map(wide_raw, roi, 7), roi, T.FINAL_T_MIN, T.FINAL_T_MAX)
    color = seg.clamp_map(seg.inpaint_temperature_map(color_raw, support, 5), support, T.COLOR_T_MIN - 5.0, T.COLOR_T_MAX + 5.0)
    fused, source, counts = seg.fuse_maps_per_pixel(roi, wide, color)
    final = seg.oriented_gaussian_blur_float(fused, roi, pack["angle_rad"], T.FINAL_SMOOTH_SIGMA_ACROSS, T.FINAL_SMOOTH_SIGMA_ALONG)
    if own:
        seg.close()
    return {"dark": dark, "light": light, "roi_eff": pack["roi_eff"], "sat": pack["sat"], "color_support": support, "dbg": pack["dbg"],
            "wide_raw": wide_raw, "color_raw": color_raw, "wide": wide, "color": color, "fused": fused, "source": source, "counts": counts,
            "final": final, "statistics": pkg.temperature_statistics(final, np.isfinite(final))}


def _check_chain(res, ref):
    for k in ("roi_eff", "sat", "dark", "light", "color_support"):
        assert np.array_equal(res["masks"][k], ref[k]), k
    assert _bits(res["wide_map_C"], ref["wide"]) and _bits(res["color_map_C"], ref["color"])
    assert _bits(res["temperature_map_C"], ref["final"])
    assert np.array_equal(res["source_map"], ref["source"])
    assert res["dbg"]["fusion"] == ref["counts"]
    assert {k: v for k, v in res["dbg"].items() if k != "fusion"} == ref["dbg"]
    _same_stats(res["statistics"], ref["statistics"])


@pytest.fixture(scope="module")
def synth(pkg):
    wide_m, col_m = _models(pkg)
    h, w = 256, 320
    roi = _disc(h, w)
    sensor = pkg.TempSensor(wide_m, col_m, (h, w), roi_full=roi)
    return sensor, roi, wide_m, col_m


@pytest.mark.gpu
def test_gpu_chain_equals_its_stages_synthetic(pkg, synth):
    sensor, roi, wide_m, col_m = synth
    img = _frame(256, 320, 1)
    res = sensor.predict(img)
    ref = _stages(pkg, img, roi, wide_m, col_m)
    assert ref["color_support"].sum() > 0 and np.isnan(ref["color_raw"][ref["color_support"]]).any()   # holes to inpaint
    assert ref["counts"]["roi_pixels"] == int(roi.sum())
    _check_chain(res, ref)
    assert np.array_equal(res["masks"]["roi_full"], roi)
    # device tensors in: device tensors out, the same bits
    import torch
    dres = sensor.predict(torch.from_numpy(img).cuda())
    assert dres["temperature_map_C"].is_cuda and dres["masks"]["dark"].is_cuda
    assert _bits(dres["temperature_map_C"].cpu().numpy(), res["temperature_map_C"]) and dres["statistics"] == res["statistics"]


@pytest.mark.gpu
def test_gpu_chain_against_the_oracle(pkg, synth):
    """the oracle's map stages on the GPU model maps (pinned against scikit-learn elsewhere): clamp / inpaint / fuse exact, the smoothing at
    1e-5 relative, the statistics of the GPU final map exactly NumPy's"""
    sensor, roi, wide_m, col_m = synth
    img = _frame(256, 320, 2)
    res = sensor.predict(img)
    ref = _stages(pkg, img, roi, wide_m, col_m)
    support = ref["color_support"]
    wide_o = T.clamp_map(T.inpaint_temperature_map(ref["wide_raw"], roi, 7), roi, T.FINAL_T_MIN, T.FINAL_T_MAX)
    color_o = T.clamp_map(T.inpaint_temperature_map(ref["color_raw"], support, 5), support, T.COLOR_T_MIN - 5.0, T.COLOR_T_MAX + 5.0)
    assert np.array_equal(res["wide_map_C"], wide_o, equal_nan=True) and np.array_equal(res["color_map_C"], color_o, equal_nan=True)
    f_o, src_o, dbg_o = T.fuse_maps_per_pixel(roi, wide_o, color_o)
    assert np.array_equal(res["source_map"], src_o) and res["dbg"]["fusion"] == dbg_o
    o = T.oriented_gaussian_blur_float(f_o, roi, res["dbg"]["carrier_angle_rad"], T.FINAL_SMOOTH_SIGMA_ACROSS, T.FINAL_SMOOTH_SIGMA_ALONG)
    g = res["temperature_map_C"]
    assert np.array_equal(np.isnan(g), np.isnan(o))
    fin = np.isfinite(o)
    assert np.abs(g[fin] - o[fin]).max() <= 1e-5 * np.abs(o[fin]).max()
    _same_stats(res["statistics"], pkg.temperature_statistics(g, np.isfinite(g)))


@pytest.mark.gpu
def test_gpu_session_reuse_equals_fresh_sessions(pkg, synth):
    sensor, roi, wide_m, col_m = synth
    frames = [_frame(256, 320, s) for s in (3, 4, 5)]
    runs = [sensor.predict(f) for f in frames]
    for f, r in zip(frames, runs):
        fresh = pkg.TempSensor(wide_m, col_m, (256, 320), roi_full=roi)
        q = fresh.predict(f)
        fresh.close()
        for k in ("temperature_map_C", "wide_map_C", "color_map_C"):
            assert _bits(r[k], q[k]), k
        assert np.array_equal(r["source_map"], q["source_map"]) and r["dbg"] == q["dbg"] and r["statistics"] == q["statistics"]
        for k in r["masks"]:
            assert np.array_equal(r["masks"][k], q["masks"][k]), k


@pytest.mark.gpu
def test_gpu_chain_on_the_reference_photograph(pkg):
    """FINAL_E at 3840 x 2160: the chain equals its stages; the stored masks inside the bbox; the stored summary's valid-pixel count (the
    chain fills every ROI pixel and the carrier angle is 0 there, so it does not depend on the model parameters); the summary builds"""
    wide_m, col_m = _models(pkg)
    img = A.imread_bgr(os.path.join(G, "FINAL_E_deformed.jpg"))
    h, w = img.shape[:2]
    sensor = pkg.TempSensor(wide_m, col_m, (h, w))
    res = sensor.predict(img)
    roi = pkg.tempseg.roi_mask_from_circle(h, w, *pkg.tempseg.OUTER_CIRCLE)
    ref = _stages(pkg, img, roi, wide_m, col_m)
    _check_chain(res, ref)
    z = np.load(os.path.join(G, "temp_seg_FINAL_E.npz"))
    shape = tuple(int(v) for v in z["shape"])
    bbox = tuple(int(v) for v in z["bbox"])
    for k in ("roi", "roi_eff", "sat", "dark", "light", "color_support"):
        stored = np.unpackbits(z[k + "_bits"])[:shape[0] * shape[1]].reshape(shape).astype(bool)
        got = res["masks"]["roi_full" if k == "roi" else k]
        assert np.array_equal(pkg.tempseg.crop2d(got, bbox), stored), k
    summary = json.load(open(os.path.join(G, "ref_multimodal_summary_FINAL_E.json")))
    assert res["dbg"]["carrier_angle_rad"] == 0.0
    assert res["statistics"]["valid_pixels"] == summary["sensor_readings"]["temperature"]["valid_pixels"] == 1576625
    force = {"force_N": 1.0, "volume_cm3": 0.1, "contact_area_mm2": 3.0, "max_depth_mm": 0.5, "mm_per_px": 0.03}
    s = pkg.multimodal_summary("s", "t", "r.jpg", "d.jpg", "o", force, res["statistics"], None, None, None, None, "a", "b", "c")
    assert s["sensor_readings"]["temperature"] == res["statistics"]
    json.dumps(s)
    sensor.close()
