"""Inputs the reference processes and the library used to refuse.

1. Pair mode (vistaf_ftp_predict_pairs) with a carrier whose patch is clipped by the spectrum border: processed as upstream and as session
   mode do, with the bits of a session built on the sample's own reference.
2. Native-size (1182 x 1182) frames whose big-cluster inpaint march outgrows its queue: handed to the whole-frame kernel, same bits as an
   un-overflowed march.
3. The temperature map stages (clamp, inpaint, fusion, oriented smoothing) at any frame size; only the segmentation keeps its size limit.
"""
import os
import re

import numpy as np
import pytest

from oracle import ftp_oracle as O
from oracle import temp_oracle as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "vistaf-roboskin-vision-integrated-multimodal-sensor_amd")
G = os.path.join(os.path.dirname(__file__), "golden")
RTOL = 1e-4

_FORCE_MODEL = [None]


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


# ---------------------------------------------------------------------------------------------------------------------------------------
# CPU: the test hooks and the header comments say what the code does


def test_test_hooks_header_names_every_accepted_hook():
    hooks_h = _read(PKG_DIR, "csrc", "test_hooks.h")
    api = _read(PKG_DIR, "csrc", "api.hip")
    body = api[api.index("int vistaf_ftp_test_set("):]
    body = body[:body.index("\n}\n")]
    accepted = set(re.findall(r'n == "([a-z0-9_]+)"', body))
    documented = set(re.findall(r'^\s*/?\*\s*(?:name:)?\s*"([a-z0-9_]+)"', hooks_h, re.M))
    assert {"big_gq_cap", "big_fallback"} <= accepted
    assert accepted == documented, (accepted ^ documented)


def test_header_comments_state_what_is_refused():
    ftp_h = _read(ROOT, "include", "vistaf_ftp.h")
    nc = ftp_h[ftp_h.index("#define VISTAF_FRAME_NO_CARRIER"):]
    nc = nc[:nc.index("*/")]
    assert "DELIBERATE RESTRICTION" not in nc and "clipped" in nc and "period" in nc
    qo = ftp_h[ftp_h.index("#define VISTAF_FRAME_QUEUE_OVERFLOW"):]
    qo = qo[:qo.index("*/")]
    assert "unwrap" in qo and "whole-frame" in qo
    # constants the reference would not compute the same way are refused at create, and the header says so next to the field
    for field, limit in (("n_fft_peaks", "1..64"), ("irls_iters", ">= 1")):
        line = next(ln for ln in ftp_h.splitlines() if re.search(r"\b%s;" % field, ln))
        assert limit in line and "refuse" in line, line
    temp_h = _read(ROOT, "include", "vistaf_temp.h")
    assert "multiple of 16" in temp_h and "any H, W >= 1" in temp_h
    ts = _read(PKG_DIR, "csrc", "tempseg.hip")
    create = ts[ts.index("int vistaf_tempseg_create("):]
    create = create[:create.index("\n}\n")]
    assert "% 16" not in create and "H < 64" not in create               # the limit lives in vistaf_tempseg_segment only
    seg = ts[ts.index("int vistaf_tempseg_segment("):]
    assert "H % 16" in seg[:seg.index("\n}\n")]
    # the pair-mode status kernel refuses only a missing carrier or a non-positive period
    tables = _read(PKG_DIR, "csrc", "k_dft_tables.hip")
    ps = tables[tables.index("void k_pair_status("):]
    ps = ps[:ps.index("\n}\n")]
    assert "g.ph" not in ps and "g.pw" not in ps


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU


@pytest.fixture(scope="module")
def cal(pkg):
    model, neg = pkg.load_calibration(os.path.join(G, "calibration_phase_to_height.json"))
    fm = pkg.load_force_calibration(os.path.join(G, "calibration_height_to_force.json"))["best_model"]
    _FORCE_MODEL[0] = fm
    return model, neg, fm


def _sensor(pkg, cal, n, cfg, max_batch, ref=None, **kw):
    ref = pkg.synth.reference_frame(n, **kw) if ref is None else ref
    return ref, pkg.FtpSensor(ref, pkg.synth.roi_circle(n), cfg, cal[0], cal[1], cal[2], max_batch=max_batch)


def _check_frame(out, b, o, n, check_argmin=True):
    """compare GPU outputs of frame b against oracle result dict o.  RTOL (1e-4) is relative to the map's PEAK (a depth map is zero over
    most of the ROI, a per-pixel relative bar is meaningless there): every pixel within 1e-4 * max|map|; scalars within 1e-4 relative."""
    hm = out["height_map_mm"][b].cpu().numpy()
    ref = o["height_map_mm_crop"]
    assert int(out["status"][b]) == 0
    assert np.array_equal(np.isnan(hm), np.isnan(ref))
    peak = max(float(np.nanmax(np.abs(ref))), 1e-6)
    diff = np.abs(hm - ref)
    assert float(np.nanmax(diff)) <= RTOL * peak
    rel = out["output_reliable"][b].cpu().numpy().astype(bool)
    mism = int((rel != o["output_reliable_crop"]).sum())
    assert mism == 0
    s = out["scalars"][b].cpu().numpy()
    assert int(s[4]) == o["argmax_depth_index"]                       # arg-max depth index: bit-exact
    v, (ax, ay) = o["argmin_unitless"]
    if check_argmin:
        assert int(s[8]) == ay * n + ax                              # arg-min unitless index: bit-exact
    assert abs(s[7] - v) <= RTOL * max(abs(v), 1e-6)
    for i, key in ((0, "volume_cm3"), (1, "contact_area_mm2"), (2, "max_depth_mm")):
        assert abs(s[i] - o[key]) <= RTOL * max(abs(o[key]), 1e-9), key
    # The force is a FUNCTION of the volume (force_sensor.py:149-167; shipped: growth a(e^{bV} - 1)): a volume inside the bar maps to a force
    # inside the bar times the curve's condition number |V f'(V) / f(V)| (1.8 at V = 0.14 cm^3), so that is the force's bar.
    V, F = o["volume_cm3"], o["force_N"]
    if V > 0 and abs(F) > 0 and _FORCE_MODEL[0] is not None:
        dV = 1e-6 * V
        kappa = abs((O.predict_force_from_volume(_FORCE_MODEL[0], V + dV) - O.predict_force_from_volume(_FORCE_MODEL[0], V - dV)) / (2 * dV) * V / F)
    else:
        kappa = 1.0
    # the widening is capped (a genuine force-tail error must not hide behind a large condition number), and the curve
    # evaluation itself is checked tightly on the GPU's OWN volume, so that only the volume carries the 1e-4 bar.
    assert abs(s[3] - F) <= RTOL * min(4.0, max(1.0, kappa)) * max(abs(F), 1e-9), "force_N"
    if _FORCE_MODEL[0] is not None:
        assert abs(s[3] - O.predict_force_from_volume(_FORCE_MODEL[0], float(s[0]))) <= 1e-12 * max(1.0, abs(s[3])), "force curve on the GPU's own volume"
    # the carrier peak is refined in float32 from spectrum magnitudes: equal to ~1 ulp of the peak position
    assert abs(s[5] - o["estimated_grating_period_px"]) <= 1e-5 * s[5] and abs(s[6] - o["mm_per_px"]) <= 1e-5 * s[6]
    assert int(s[9]) == int(o["reliable"].sum())


def _fringe(pkg, n, seed, kx, ky, wf, deform):
    """A (possibly tilted) fringe frame whose carrier sits at (kx, ky) bins of a wf x wf spectrum; synth.py's illumination and noise model,
    plus a Gaussian phase dent for the deformed frame."""
    rng = np.random.default_rng(seed)
    cx, cy, r = pkg.synth.roi_circle(n)
    yy, xx = np.mgrid[0:n, 0:n].astype(np.float64)
    phi = 0.0
    if deform:
        amp = rng.uniform(0.4, 1.2)
        x0, y0 = cx + rng.uniform(-0.3, 0.3) * r, cy + rng.uniform(-0.3, 0.3) * r
        sig = rng.uniform(0.1, 0.2) * n
        phi = -amp * np.exp(-((xx - x0) ** 2 + (yy - y0) ** 2) / (2.0 * sig * sig))
    s = 1.0 + 0.15 * np.cos(np.pi * np.sqrt((xx - cx) ** 2 + (yy - cy) ** 2) / r)
    img = 128.0 * s * (0.55 + 0.35 * np.cos(2.0 * np.pi * (kx * xx + ky * yy) / wf + phi)) + rng.normal(0.0, 2.0, size=(n, n))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def _same_bits(torch, a, b):
    return torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))


@pytest.mark.gpu
def test_pair_mode_processes_clipped_carrier_patches(pkg, cal):
    """A 221 x 221 patch (patch_half_width_bins 110) around the carrier of a 12.5 px-class fringe reaches past the right border of the
    260-bin spectrum; tilted carriers clip it at the top or the bottom instead.  Mixed with unclipped samples in one pair batch, every sample
    has status 0 and matches the oracle; a clipped one gives the bits of a session on its own reference, an unclipped one the bits of a
    batch without the clipped ones."""
    import torch
    n = 224
    cfg = pkg.FtpConfig.scaled(n)
    bw = 110
    cfg.patch_half_width_bins = bw
    pm = 2 * bw + 1
    wf = n + 2 * cfg.fft_pad_px
    carriers = [(23.0, 0.0), (16.2, 0.0), (18.3, 22.4), (14.7, 9.3), (17.4, -21.6)]     # clipped right, -, bottom, -, top
    nb = len(carriers)
    refs = np.stack([_fringe(pkg, n, 100 + 2 * b, kx, ky, wf, False) for b, (kx, ky) in enumerate(carriers)])
    defs = np.stack([_fringe(pkg, n, 101 + 2 * b, kx, ky, wf, True) for b, (kx, ky) in enumerate(carriers)])
    sensor = pkg.FtpSensor(None, pkg.synth.roi_circle(n), cfg, cal[0], cal[1], cal[2], max_batch=nb, frame_shape=(n, n))
    out = sensor.predict_pairs(refs, defs)
    torch.cuda.synchronize()
    info = sensor.pair_info(nb)
    clipped = []
    for b in range(nb):
        hf, wfi = info[b]["fft_shape"]
        assert wfi == wf
        px, py = (int(np.rint(v)) for v in info[b]["peak_refined"])
        pw = min(wfi, px + bw + 1) - max(0, px - bw)
        ph = min(hf, py + bw + 1) - max(0, py - bw)
        clipped.append(ph < pm or pw < pm)
    assert clipped == [True, False, True, False, True]
    assert out["status"].cpu().numpy().tolist() == [0] * nb
    for b in range(nb):
        rs = O.make_reference_state(refs[b], *pkg.synth.roi_circle(n), cfg)
        assert np.allclose(info[b]["peak_refined"], rs["demod"]["peak_refined"], rtol=0, atol=1e-9), b
        o = O.process_frame(defs[b], rs, cfg, *cal)
        assert int(o["reliable"].sum()) > 0
        _check_frame(out, b, o, n)
    # clipped samples: the bits of a session built on the sample's own reference
    for b in (i for i in range(nb) if clipped[i]):
        _, s1 = _sensor(pkg, cal, n, cfg, 1, ref=refs[b])
        o1 = s1.predict_batch(defs[b][None])
        torch.cuda.synchronize()
        assert int(o1["status"][0]) == 0
        assert _same_bits(torch, o1["height_map_mm"][0], out["height_map_mm"][b]), b
        assert torch.equal(o1["scalars"][0], out["scalars"][b]) and torch.equal(o1["output_reliable"][0], out["output_reliable"][b]), b
    # unclipped samples: the bits of the same pairs run without the clipped ones
    keep = [b for b in range(nb) if not clipped[b]]
    o2 = sensor.predict_pairs(refs[keep], defs[keep])
    torch.cuda.synchronize()
    for i, b in enumerate(keep):
        assert int(o2["status"][i]) == 0
        assert _same_bits(torch, o2["height_map_mm"][i], out["height_map_mm"][b]), b
        assert torch.equal(o2["scalars"][i], out["scalars"][b]) and torch.equal(o2["output_reliable"][i], out["output_reliable"][b]), b


@pytest.mark.gpu
def test_big_cluster_queue_overflow_falls_back_to_the_whole_frame_kernel(pkg, cal):
    """Native 1182 x 1182 crops, constants as shipped.  With every big cluster's queue in global memory (`big_queue_lds` 0) and a 64-entry
    capacity (`big_gq_cap`), the march overflows: without the fallback (`big_fallback` 0) a frame reports status 2; with it every frame has
    status 0 and the same height map, reliable mask and scalars as the default settings and as the whole-frame kernel alone (`inpaint_tier` 1)."""
    import torch
    n, nb = 1182, 2
    cfg = pkg.FtpConfig.as_shipped()
    ref, sensor = _sensor(pkg, cal, n, cfg, nb, config=7)
    frames = np.stack([pkg.synth.deformed_frame(n, i, config=7) for i in range(nb)])
    base = sensor.predict_batch(frames)
    torch.cuda.synchronize()
    assert (base["status"].cpu().numpy() == 0).all()
    hm0, rel0, sc0 = base["height_map_mm"].clone(), base["output_reliable"].clone(), base["scalars"].clone()
    img0 = sensor.intermediate("img", nb).cpu().numpy().copy()
    sensor._test_set("big_queue_lds", 0)
    sensor._test_set("big_gq_cap", 64)
    sensor._test_set("big_fallback", 0)
    ov = sensor.predict_batch(frames)
    torch.cuda.synchronize()
    assert (ov["status"].cpu().numpy() == 2).any(), "the 64-entry queue did not overflow"
    sensor._test_set("big_fallback", 1)
    fb = sensor.predict_batch(frames)
    torch.cuda.synchronize()
    assert (fb["status"].cpu().numpy() == 0).all()
    assert np.array_equal(sensor.intermediate("img", nb).cpu().numpy(), img0)
    assert _same_bits(torch, fb["height_map_mm"], hm0)
    assert torch.equal(fb["output_reliable"], rel0) and torch.equal(fb["scalars"], sc0)
    sensor._test_set("big_queue_lds", 1)
    sensor._test_set("big_gq_cap", 0)
    sensor._test_set("inpaint_tier", 1)
    wf = sensor.predict_batch(frames)
    torch.cuda.synchronize()
    assert (wf["status"].cpu().numpy() == 0).all()
    assert _same_bits(torch, wf["height_map_mm"], hm0)
    assert torch.equal(wf["output_reliable"], rel0) and torch.equal(wf["scalars"], sc0)
    for bad in ("big_gq_cap",):
        with pytest.raises(ValueError):
            sensor._test_set(bad, 100)                                     # not a power of two


def _synthetic_maps(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    roi = ((yy - h / 2) ** 2 + (xx - w / 2) ** 2) < (0.45 * min(h, w)) ** 2
    roi |= (np.abs(yy - h / 2) < 0.3 * h) & (np.abs(xx - w / 2) < 0.45 * w)
    wide = (30.0 + 6.0 * np.sin(xx / 17.0) * np.cos(yy / 23.0) + 0.3 * rng.standard_normal((h, w))).astype(np.float32)
    wide[rng.random((h, w)) < 0.04] = np.nan
    wide[int(0.3 * h):int(0.3 * h) + 6, int(0.4 * w):int(0.4 * w) + 9] = np.nan
    support = roi & (((yy - 0.55 * h) ** 2 + (xx - 0.45 * w) ** 2) < (0.25 * min(h, w)) ** 2)
    color = (27.0 + 8.0 * np.cos(yy / 13.0) + 0.5 * rng.standard_normal((h, w))).astype(np.float32)
    color[~support] = np.nan
    color[support & (rng.random((h, w)) < 0.05)] = np.nan
    return roi, wide, support, color


def _map_stages_against_oracle(api, roi, wide, support, color):
    assert np.array_equal(api.clamp_map(wide, roi, 25.0, 40.0), T.clamp_map(wide, roi, 25.0, 40.0), equal_nan=True)
    for m, r, rad in ((wide, roi, 7), (color, support, 5)):
        assert np.array_equal(api.inpaint_temperature_map(m, r, rad), T.inpaint_temperature_map(m, r, rad), equal_nan=True), rad
    wide_o = T.clamp_map(T.inpaint_temperature_map(wide, roi, 7), roi, T.FINAL_T_MIN, T.FINAL_T_MAX)
    color_o = T.clamp_map(T.inpaint_temperature_map(color, support, 5), support, T.COLOR_T_MIN - 5.0, T.COLOR_T_MAX + 5.0)
    f_o, src_o, dbg_o = T.fuse_maps_per_pixel(roi, wide_o, color_o)
    f_g, src_g, dbg_g = api.fuse_maps_per_pixel(roi, wide_o, color_o)
    assert np.array_equal(f_g, f_o, equal_nan=True) and np.array_equal(src_g, src_o) and dbg_g == dbg_o
    for angle in (0.0, 0.31, -1.2):
        o = T.oriented_gaussian_blur_float(f_o, roi, angle, T.FINAL_SMOOTH_SIGMA_ACROSS, T.FINAL_SMOOTH_SIGMA_ALONG)
        g = api.oriented_gaussian_blur_float(f_o, roi, angle, T.FINAL_SMOOTH_SIGMA_ACROSS, T.FINAL_SMOOTH_SIGMA_ALONG)
        assert np.array_equal(np.isnan(g), np.isnan(o)), angle
        fin = np.isfinite(o)
        if fin.any():
            assert np.abs(g[fin] - o[fin]).max() <= 1e-5 * np.abs(o[fin]).max(), angle


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,seed", [(151, 203, 11), (33, 47, 12), (300, 17, 13)])
def test_map_stages_at_any_frame_size(pkg, h, w, seed):
    """clamp / inpaint / fusion exactly, the oriented smoothing within 1e-5 relative, against the oracle restatement at sizes the
    segmentation cannot take -- through a TempSegmenter and through the module-level drop-ins."""
    roi, wide, support, color = _synthetic_maps(h, w, seed)
    seg = pkg.tempseg.TempSegmenter(h, w)
    _map_stages_against_oracle(seg, roi, wide, support, color)
    _map_stages_against_oracle(pkg.tempseg, roi, wide, support, color)
    # inpainting a constant map (holes included) gives that constant at every ROI pixel
    const = np.where(np.isfinite(wide), np.float32(31.25), np.float32(np.nan)).astype(np.float32)
    for api in (seg, pkg.tempseg):
        c = api.inpaint_temperature_map(const, roi, 7)
        assert np.all(c[roi] == np.float32(31.25)) and np.isnan(c[~roi]).all()
    seg.close()


@pytest.mark.gpu
def test_segmentation_keeps_its_size_limit_and_smoothing_is_transpose_symmetric(pkg):
    """vistaf_tempseg_segment still needs H % 16 == 0 and sides >= 64 (matrix-core strips of its band-pass DFT) and says so; the map stages
    of the same session work.  Angle 0 with equal sigmas smooths a transposition-symmetric map (odd, non-16 square) into a transposition-
    symmetric one."""
    h, w = 151, 203
    seg = pkg.tempseg.TempSegmenter(h, w)
    img = np.zeros((h, w, 3), np.uint8)
    roi = np.ones((h, w), np.uint8)
    with pytest.raises(ValueError, match="multiple of 16"):
        seg.segment(img, roi)
    roi_b, wide, _, _ = _synthetic_maps(h, w, 3)
    assert np.array_equal(seg.clamp_map(wide, roi_b, 25.0, 40.0), T.clamp_map(wide, roi_b, 25.0, 40.0), equal_nan=True)
    seg.close()
    n = 61
    yy, xx = np.mgrid[0:n, 0:n].astype(np.float64)
    m = (30.0 + 4.0 * np.cos(xx / 7.0) * np.cos(yy / 7.0) + np.cos((xx - yy) / 3.0) + 0.01 * (xx * yy)).astype(np.float32)
    m[5, 9] = m[9, 5] = np.float32(np.nan)
    r = ((yy - n // 2) ** 2 + (xx - n // 2) ** 2) <= (n // 2 - 2) ** 2
    assert np.array_equal(m, m.T, equal_nan=True) and np.array_equal(r, r.T)
    s = pkg.tempseg.TempSegmenter(n, n)
    g = s.oriented_gaussian_blur_float(m, r, 0.0, 2.5, 2.5)
    s.close()
    assert np.array_equal(np.isnan(g), np.isnan(g.T))
    fin = np.isfinite(g)
    assert fin.any() and np.abs(g[fin] - g.T[fin]).max() <= 1e-6 * np.abs(g[fin]).max()
