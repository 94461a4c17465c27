#!/usr/bin/env python
"""Timing of the point-cloud read-out (CloudReadout.measure): HIP-event time of measure() alone, warm, median of the calls with min and max, at
stride 1 and stride 2 and with a label plane, next to a device-to-device copy of the same depth batch in the same run -- the read-out reads
the batch twice (count, emit) and the copy once, so the copy is the yardstick.  Batch 256 of 224 x 224 planes and batch 8 of 1182 x 1182
planes: a noisy floor below depth_eps_mm, NaN outside the ROI disc, three bumps per frame (23 % of the pixels are surface pixels, far more
than in a real frame), made on the device from a seed.  max_points holds every point, so every record is written.  Bytes: the batch
read twice, 9 neighbour floats per surface pixel (from cache), 36 bytes (37 with labels) written per point.
python tests/diag/bench_cloud.py [calls] [small|native|both]"""
import importlib, json, math, os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("vistaf-roboskin-vision-integrated-multimodal-sensor_amd")
CALLS = int(sys.argv[1]) if len(sys.argv) > 1 else 30
WHICH = sys.argv[2] if len(sys.argv) > 2 else "both"
EPS = 0.01


def timed(fn):
    for _ in range(3):
        fn()                                   # warm: code objects loaded, the handle's buffer allocated, output tensors' allocator blocks cached
    torch.cuda.synchronize()
    ms = []
    for _ in range(CALLS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}


def planes(n, batch):
    g = torch.Generator(device="cuda").manual_seed(n + batch)
    yy, xx = torch.meshgrid(torch.arange(n, device="cuda", dtype=torch.float32), torch.arange(n, device="cuda", dtype=torch.float32), indexing="ij")
    t = torch.arange(batch, device="cuda", dtype=torch.float32)[:, None, None] / max(batch - 1, 1)
    d = 0.009 * torch.rand((batch, n, n), generator=g, device="cuda")
    for k in range(3):
        cx, cy = n * (0.3 + 0.2 * k) + 0.1 * n * t, n * (0.35 + 0.15 * k) - 0.05 * n * t
        d += 0.8 * (1.0 + 0.3 * k) * torch.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2.0 * (0.05 * n) ** 2))
    d[:, (xx - n // 2) ** 2 + (yy - n // 2) ** 2 > (n // 2 - 1) ** 2] = float("nan")
    return d.contiguous()


def run(n, batch):
    depth = planes(n, batch)
    mpp = torch.full((batch,), 0.05, dtype=torch.float64, device="cuda")
    index = torch.zeros((batch, n, n), dtype=torch.int8, device="cuda")
    cap = batch * n * n
    rd1, rd2 = pkg.CloudReadout(n, n, batch, cap, 1), pkg.CloudReadout(n, n, batch, cap, 2)
    out = {"points": torch.empty((cap, 8), dtype=torch.float32, device="cuda"), "pixel": torch.empty((cap,), dtype=torch.int32, device="cuda"),
           "label": torch.empty((cap,), dtype=torch.int8, device="cuda")}
    dst = torch.empty_like(depth)
    t_copy = timed(lambda: dst.copy_(depth))
    t_s1 = timed(lambda: rd1.measure(depth, mpp, EPS, out=out))
    t_s1l = timed(lambda: rd1.measure(depth, mpp, EPS, contact_index=index, out=out))
    t_s2 = timed(lambda: rd2.measure(depth, mpp, EPS, out=out))
    t_copy2 = timed(lambda: dst.copy_(depth))
    r1 = rd1.measure(depth, mpp, EPS, out=out)
    frame = r1["frame"].cpu().numpy()
    n1 = int(r1["offsets"][-1].item())
    n2 = int(rd2.measure(depth, mpp, EPS, out=out)["offsets"][-1].item())
    P = n * n
    in_bytes = batch * P * 4
    surf = float(frame[:, 0].sum())
    by = lambda pts, per: 2 * in_bytes + int(surf) * 36 + pts * per
    copy_ms = min(t_copy["median"], t_copy2["median"])
    print(json.dumps({"frame": n, "batch": batch, "calls": CALLS, "vector_path": P % 4 == 0,
                      "measure_ms_median": t_s1["median"], "measure_ms_min": t_s1["min"], "measure_ms_max": t_s1["max"],
                      "measure_labels_ms_median": t_s1l["median"], "measure_labels_ms_min": t_s1l["min"], "measure_labels_ms_max": t_s1l["max"],
                      "measure_stride2_ms_median": t_s2["median"], "measure_stride2_ms_min": t_s2["min"], "measure_stride2_ms_max": t_s2["max"],
                      "copy_ms_median_before": t_copy["median"], "copy_ms_median_after": t_copy2["median"], "copy_ms_min": min(t_copy["min"], t_copy2["min"]),
                      "ratio_measure_to_copy": t_s1["median"] / copy_ms, "ratio_labels_to_copy": t_s1l["median"] / copy_ms,
                      "ratio_stride2_to_copy": t_s2["median"] / copy_ms,
                      "measure_bytes": by(n1, 36), "copy_bytes": 2 * in_bytes,
                      "measure_GBps": by(n1, 36) / t_s1["median"] / 1e6, "copy_GBps": 2 * in_bytes / copy_ms / 1e6,
                      "points": n1, "points_stride2": n2, "surface_fraction": surf / (batch * P)}), flush=True)
    rd1.close()
    rd2.close()


if WHICH in ("small", "both"):
    run(224, 256)
if WHICH in ("native", "both"):
    run(1182, 8)
