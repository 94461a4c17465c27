"""Time temperature_sensor.main() on FINAL_E (3840 x 2160): (a) TempSensor.predict, one session, NumPy photograph in and maps out, and with
the photograph already on the device; (b) the stage-by-stage sequence of the public calls with their host round trips (tests/test_tempsensor.py
_stages, one persistent TempSegmenter); the two inpaint steps and the statistics alone on device buffers.  Device-synchronised medians after
warm-up; prints a JSON line after each measurement, the last one holds them all.

    python tests/diag/bench_tempsensor.py [--iters 20] [--warmup 3] [--parts a,a_dev,b,stages]
For the kernel times:  rocprofv3 --kernel-trace --stats -d <dir> -- python tests/diag/bench_tempsensor.py --iters 1 --warmup 0 --parts a_dev,stages
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("vistaf-roboskin-vision-integrated-multimodal-sensor_amd")
from oracle import align_oracle as A          # noqa: E402
import test_tempsensor as TT                  # noqa: E402


def _median_ms(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parts", default="a,a_dev,b,stages", help="comma list of a (NumPy in / out), a_dev (device photograph), b (stages), "
                    "stages (inpaint steps and statistics alone)")
    a = ap.parse_args()
    parts = set(a.parts.split(","))
    wide_m, col_m = TT._models(pkg)
    img = A.imread_bgr(os.path.join(ROOT, "tests", "golden", "FINAL_E_deformed.jpg"))
    H, W = img.shape[:2]
    roi = pkg.tempseg.roi_mask_from_circle(H, W, *pkg.tempseg.OUTER_CIRCLE)
    sensor = pkg.TempSensor(wide_m, col_m, (H, W))
    img_d = torch.from_numpy(img).cuda()
    out = {"frame": [H, W]}
    lib, seg = pkg._lib.load(), pkg.TempSegmenter(H, W)
    if "a" in parts:
        out["a_predict_numpy_ms"] = _median_ms(lambda: sensor.predict(img), a.iters, a.warmup)
        print(json.dumps(out), flush=True)
    if "a_dev" in parts:
        out["a_predict_device_ms"] = _median_ms(lambda: sensor.predict(img_d), a.iters, a.warmup)
        print(json.dumps(out), flush=True)
    if "b" in parts:
        out["b_stages_ms"] = _median_ms(lambda: TT._stages(pkg, img, roi, wide_m, col_m, seg), a.iters, a.warmup)
        print(json.dumps(out), flush=True)
    if "stages" not in parts:
        return
    res = sensor.predict(img_d)
    # the two inpaint steps and the statistics alone, device buffers in and out
    dres = TT._stages(pkg, img, roi, wide_m, col_m, seg)
    st = int(torch.cuda.current_stream().cuda_stream)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    wr, cr = dev(dres["wide_raw"]), dev(dres["color_raw"])
    r8, s8 = dev(roi.astype(np.uint8)), dev(dres["color_support"].astype(np.uint8))
    o = torch.empty_like(wr)
    out["inpaint_wide_ms"] = _median_ms(lambda: lib.vistaf_temp_inpaint_map(seg._h, wr.data_ptr(), r8.data_ptr(), 7, o.data_ptr(), st), a.iters, a.warmup)
    out["inpaint_color_ms"] = _median_ms(lambda: lib.vistaf_temp_inpaint_map(seg._h, cr.data_ptr(), s8.data_ptr(), 5, o.data_ptr(), st), a.iters, a.warmup)
    fin = res["temperature_map_C"]
    out["statistics_ms"] = _median_ms(lambda: pkg.map_statistics(fin), a.iters, a.warmup)
    out["valid_pixels"] = res["statistics"]["valid_pixels"]
    out["color_support_pixels"] = int(dres["color_support"].sum())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
