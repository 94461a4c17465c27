"""Time the two-model regressor pass (predict_maps) on a 3840 x 2160 frame: the black model (L, a, b, gray; degree 3, 35 terms) over the
ROI and the colour model (L, a, b; degree 2 + isotonic calibrator) over a colour-support-like mask.  Prints one JSON line.

    python tests/diag/bench_tempmodel.py [--iters 200]
For the kernel-only time:  rocprofv3 --kernel-trace --stats -d <dir> -- python tests/diag/bench_tempmodel.py
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("vistaf-roboskin-vision-integrated-multimodal-sensor_amd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--h", type=int, default=2160)
    ap.add_argument("--w", type=int, default=3840)
    a = ap.parse_args()
    H, W = a.h, a.w
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    planes = {k: (torch.rand((H, W), generator=g, device=dev) * 255).round() for k in ("L", "a", "b", "gray")}
    yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    roi = ((yy - H / 2) ** 2 + (xx - W / 2) ** 2) < (0.48 * min(H, W)) ** 2
    cmask = roi & (torch.rand((H, W), generator=g, device=dev) < 0.4)
    rng = np.random.default_rng(0)
    F = pkg.tempmodel.polynomial_powers
    black = pkg.TempModel(("L", "a", "b", "gray"), [120, 128, 128, 110], [60, 20, 20, 55], True, True, F(4, 3), rng.normal(0, 1, 35), 18.0)
    xt = np.sort(rng.uniform(10, 40, 70))
    colour = pkg.TempModel(("L", "a", "b"), [120, 128, 128], [60, 20, 20], True, True, F(3, 2), rng.normal(0, 1, 10), 13.0,
                           dict(x_thresholds=xt, y_thresholds=np.sort(rng.uniform(20, 33, 70)), x_min=xt[0], x_max=xt[-1], out_of_bounds="clip"))
    for _ in range(5):
        pkg.predict_maps(planes, (black, roi), (colour, cmask))
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        pkg.predict_maps(planes, (black, roi), (colour, cmask))
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.iters
    P = H * W
    nbytes = P * (4 * 4 + 2 + 2 * 4)       # four planes, two masks, two maps
    print(json.dumps({"frame": [H, W], "iters": a.iters, "ms_per_pass_incl_host": round(ms, 4), "bytes_per_pass": nbytes,
                      "GBps_incl_host": round(nbytes / (ms * 1e-3) / 1e9, 1)}))


if __name__ == "__main__":
    main()
