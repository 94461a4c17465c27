#!/usr/bin/env python
"""Timing of the input conversion (launch_to_gray) for every input format: the "gray+badpix" stage of predict_batch's own HIP-event stage
timing on a session with bad_pixel_enable = 0, where that stage is the conversion kernel and the 4 * B byte memset behind it and nothing
else.  Warm, median of the calls with min and max, at batch 256 of 224 x 224 frames and at batch 8 of 1182 x 1182 frames, every format in
the same run with BGR_U8 -- the route a camera user has today, after a conversion of their own -- measured first and again last as the
yardstick: the distance between its two medians and its min..max are the run's own repeat-to-repeat spread.  Bytes moved per pixel
(read + the 4 written) and the rate they amount to are printed beside each time.
python tests/diag/bench_formats.py [calls]"""
import importlib, json, os, statistics, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("vistaf-roboskin-vision-integrated-multimodal-sensor_amd")
CALLS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
G = os.path.join(ROOT, "tests", "golden")
STAGE = "gray+badpix"
READ_BYTES = {"gray": 1, "bgr": 3, "gray_f16": 2, "bgr_f16": 6, "rgb": 3, "bgra": 4, "rgba": 4, "yuyv": 2, "uyvy": 2, "nv12": 1}      # per pixel; a mosaic: 1


def encode(g, fmt):
    """[B,n,n] uint8 gray scenes as frames in `fmt` (gray in every channel and site, chroma 128, alpha 255: the content does not matter here)"""
    B, h, w = g.shape
    if fmt in ("gray", "gray_f16") or fmt.startswith("bayer_"):
        f = g
    elif fmt in ("bgr", "bgr_f16", "rgb"):
        f = np.repeat(g[..., None], 3, axis=-1)
    elif fmt in ("bgra", "rgba"):
        f = np.concatenate([np.repeat(g[..., None], 3, axis=-1), np.full((B, h, w, 1), 255, np.uint8)], axis=-1)
    elif fmt in ("yuyv", "uyvy"):
        f = np.full((B, h, w // 2, 4), 128, np.uint8)
        f[..., [0, 2] if fmt == "yuyv" else [1, 3]] = g.reshape(B, h, w // 2, 2)
    else:
        f = np.concatenate([g, np.full((B, h // 2, w), 128, np.uint8)], axis=1)
    t = torch.from_numpy(np.ascontiguousarray(f)).cuda()
    return t.to(torch.float16) if fmt.endswith("_f16") else t


def run(batch, n, distinct):
    cal, neg = pkg.load_calibration(os.path.join(G, "calibration_phase_to_height.json"))
    fm = pkg.load_force_calibration(os.path.join(G, "calibration_height_to_force.json"))["best_model"]
    cfg = pkg.FtpConfig.scaled(n)
    cfg.bad_pixel_enable = 0
    sensor = pkg.FtpSensor(pkg.synth.reference_frame(n), pkg.synth.roi_circle(n), cfg, cal, neg, fm, max_batch=batch)
    sensor.enable_stage_timing(True)
    g = np.tile(pkg.synth.deformed_batch(n, 0, distinct), (batch // distinct, 1, 1))
    out = sensor._new_out(batch)

    def timed(fmt):
        frames = encode(g, fmt)
        ms = []
        for i in range(3 + CALLS):                  # three warm calls: code objects loaded, the workspace touched
            sensor.predict_batch(frames, out=out, format=fmt)
            torch.cuda.synchronize()
            if i >= 3:
                ms.append(sensor.stage_times_ms()[STAGE])
        return {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}
    rows = [("bgr (first)", "bgr", timed("bgr"))] + [(fmt, fmt, timed(fmt)) for fmt in pkg._lib.FORMATS if fmt != "bgr"] + [("bgr (last)", "bgr", timed("bgr"))]
    bgr = [r[2] for r in rows if r[1] == "bgr"]
    yard = min(b["median"] for b in bgr)
    spread = max(b["max"] for b in bgr) - min(b["min"] for b in bgr)
    for label, fmt, t in rows:
        per_px = READ_BYTES.get(fmt, 1) + 4
        print(json.dumps({"frame": n, "batch": batch, "calls": CALLS, "format": label, "us_median": 1e3 * t["median"], "us_min": 1e3 * t["min"],
                          "us_max": 1e3 * t["max"], "bytes_per_px": per_px, "GB_per_s": per_px * batch * n * n / (t["median"] * 1e-3) / 1e9,
                          "ratio_to_bgr": t["median"] / yard, "beyond_bgr_spread": bool(t["median"] - yard > spread)}), flush=True)
    print(json.dumps({"frame": n, "batch": batch, "bgr_us_median": 1e3 * yard, "bgr_spread_us": 1e3 * spread}), flush=True)
    sensor.close()


run(256, 224, 8)
run(8, 1182, 2)
