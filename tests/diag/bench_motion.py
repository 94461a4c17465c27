#!/usr/bin/env python
"""Timing of the contact motion read-out (ContactMotion.update): HIP-event time of update() alone, warm, median of the calls with min and max, at
batch 256 of 224 x 224 planes with 1, 4 and 8 contacts per frame, next to the shape read-out (ContactShapes.measure) on the same planes and
tables in the same run, as context: both launch one workgroup per (frame, row) that walks the row's box.  Every contact is an elliptical
Gaussian bump 0.8 mm deep, sigma 9 and 5.4 px (a footprint about 40 x 25 px, some 800 template pixels), that drifts less than a pixel per frame, so every pair
of frames 1.. registers with status ok; the planes, tables and tracker rows are made on the host from the geometry.  Work per update: B * K
pairs, each iterations + 3 sweeps of its box.
python tests/diag/bench_motion.py [calls] [batch]"""
import importlib, json, os, statistics, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import shapes_helpers as SH
pkg = importlib.import_module("vistaf-roboskin-vision-integrated-multimodal-sensor_amd")
CALLS = int(sys.argv[1]) if len(sys.argv) > 1 else 30
BATCH = int(sys.argv[2]) if len(sys.argv) > 2 else 256
N, EPS, SIGMA, AMP, LEVEL, S_MM = 224, 0.01, 9.0, 0.8, 0.05, 0.05
SPOTS = [(56, 56), (168, 56), (56, 168), (168, 168), (112, 112), (112, 28), (28, 112), (196, 112)]


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


def scene(batch, k):
    """depth [B,N,N] f32, index [B,N,N] i8, table [B,8,16], count [B], tracks [B,8,16] for k drifting bumps per frame"""
    yy, xx = np.mgrid[0:N, 0:N].astype(np.float64)
    depth, index = np.zeros((batch, N, N), np.float32), np.full((batch, N, N), -1, np.int8)
    centres = np.zeros((batch, k, 2))
    for t in range(batch):
        for j, (x0, y0) in enumerate(SPOTS[:k]):
            cx, cy = x0 + 5.0 * np.sin(0.1 * t + j), y0 + 5.0 * np.cos(0.13 * t + 2 * j)
            centres[t, j] = cx, cy
            win = (slice(max(int(cy) - 40, 0), min(int(cy) + 41, N)), slice(max(int(cx) - 40, 0), min(int(cx) + 41, N)))
            a = 0.4 * j
            u, v = np.cos(a) * (xx[win] - cx) + np.sin(a) * (yy[win] - cy), -np.sin(a) * (xx[win] - cx) + np.cos(a) * (yy[win] - cy)
            d = AMP * (1.0 - 0.05 * j) * np.exp(-(u * u / (2.0 * SIGMA * SIGMA) + v * v / (2.0 * 0.6 * SIGMA * 0.6 * SIGMA)))
            depth[t][win] = np.maximum(depth[t][win], d.astype(np.float32))
            index[t][win][d > LEVEL] = j
    tab, cnt = SH.table_from_planes(depth, index, 8, EPS)
    tracks = np.full((batch, 8, 16), np.nan)
    for t in range(batch):
        for j in range(k):
            tracks[t, j, :5] = [j, t, j if t else -1, 0 if t else 1, 0]
            if t:
                tracks[t, j, 5:7] = centres[t, j] - centres[t - 1, j]
    return depth, index, tab, cnt, tracks


def run(k):
    depth, index, tab, cnt, tracks = (torch.as_tensor(a).cuda() for a in scene(BATCH, k))
    mpp = torch.full((BATCH,), S_MM, dtype=torch.float64, device="cuda")
    mo, sh = pkg.ContactMotion(N, N, BATCH, 8), pkg.ContactShapes(N, N, BATCH, 8)
    t_sh = timed(lambda: sh.measure(depth, index, tab, cnt, mpp, EPS))
    t_mo = timed(lambda: mo.update(depth, index, tab, cnt, tracks, mpp, EPS))
    t_sh2 = timed(lambda: sh.measure(depth, index, tab, cnt, mpp, EPS))
    mo.reset()
    out = mo.update(depth, index, tab, cnt, tracks, mpp, EPS)
    m = out["motion"].cpu().numpy()
    st = m[..., 2]
    tpl = m[..., 1][st == 0]
    err = np.abs(m[1:, :k, 4:6] - tracks.cpu().numpy()[1:, :k, 5:7])
    print(json.dumps({"frame": N, "batch": BATCH, "contacts_per_frame": k, "calls": CALLS, "iterations": mo.iterations,
                      "update_ms_median": t_mo["median"], "update_ms_min": t_mo["min"], "update_ms_max": t_mo["max"],
                      "shapes_ms_median_before": t_sh["median"], "shapes_ms_median_after": t_sh2["median"], "shapes_ms_min": min(t_sh["min"], t_sh2["min"]),
                      "ratio_update_to_shapes": t_mo["median"] / min(t_sh["median"], t_sh2["median"]),
                      "pairs": int((st == 0).sum() + (st == 1).sum()), "status_ok": int((st == 0).sum()), "status_not_converged": int((st == 1).sum()),
                      "template_pixels_mean": float(tpl.mean()) if tpl.size else 0.0, "us_per_pair": 1e3 * t_mo["median"] / max(int((st <= 1).sum()), 1),
                      "max_error_against_the_drift_px": float(np.nanmax(err))}), flush=True)
    mo.close()
    sh.close()


for k in (1, 4, 8):
    run(k)
