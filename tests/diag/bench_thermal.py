#!/usr/bin/env python
"""Timing of the thermal read-out (ThermalReadout.register and .measure, K = 8, margin 8): HIP-event time of each call alone and of the two
together, warm, median of the calls with min and max, next to `FtpSensor.contacts(8, index_plane=True)` of the same run -- the call that
produces what measure reads.  Batch 256 of 224 x 224 multi-contact frames (scaled constants) and batch 8 of native 1182 x 1182 crops
(constants as shipped), the frames' real contacts.  The temperature maps are made up (a smooth field with float32 noise) in a photograph
frame 1.3 times the crop each way, the records a small rotation about the crop centre plus a sub-pixel shift per frame, as an aligner
writes them; the work of register is one gather of four floats per crop pixel whatever the map holds.  A new path: there is no parent
figure to compare with.
python tests/diag/bench_thermal.py [calls] [small|native|both]"""
import importlib, json, math, os, statistics, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("vistaf-roboskin-vision-integrated-multimodal-sensor_amd")
import contacts_helpers as H
G = os.path.join(ROOT, "tests", "golden")
CALLS = int(sys.argv[1]) if len(sys.argv) > 1 else 30
WHICH = sys.argv[2] if len(sys.argv) > 2 else "both"
K, MARGIN = 8, 8
cal, neg = pkg.load_calibration(os.path.join(G, "calibration_phase_to_height.json"))
fm = pkg.load_force_calibration(os.path.join(G, "calibration_height_to_force.json"))["best_model"]


def timed(fn):
    for _ in range(3):
        fn()                                   # warm: code objects loaded, output tensors' allocator blocks cached
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


def run(n, batch, cfg, distinct):
    ref = pkg.synth.reference_frame(n)
    base = H.multi_contact_batch(pkg, n, 0, distinct)
    frames = torch.from_numpy(np.concatenate([base] * (batch // distinct))).cuda()
    sensor = pkg.FtpSensor(ref, pkg.synth.roi_circle(n), cfg, cal, neg, fm, max_batch=batch)
    o = sensor.predict_batch(frames)
    tab = sensor.contacts(K, index_plane=True)
    PH, PW = int(1.3 * n) | 1, int(1.3 * n) + 2
    x1, y1 = (PW - n) // 2, (PH - n) // 2
    g = torch.Generator(device="cuda").manual_seed(5)
    yy, xx = torch.meshgrid(torch.arange(PH, device="cuda", dtype=torch.float32), torch.arange(PW, device="cuda", dtype=torch.float32), indexing="ij")
    one = 31.0 + 4.0 * torch.sin(xx / (0.04 * n)) * torch.cos(yy / (0.03 * n))
    maps = (one[None] + torch.rand((batch, PH, PW), device="cuda", generator=g) - 0.5).contiguous()
    info = np.zeros((batch, 12))
    for b in range(batch):
        th, c = 0.004 * ((b % 7) - 3), n / 2.0
        cs, sn = math.cos(th), math.sin(th)
        info[b, :2] = (0.37 * (b % 5) - 0.8, 0.21 * (b % 3) - 0.3)
        info[b, 3:9] = (cs, -sn, c - cs * c + sn * c, sn, cs, c - sn * c - cs * c)
    info = torch.from_numpy(info).cuda()
    reader = pkg.ThermalReadout(n, n, PH, PW, (x1, y1), True, batch, K, MARGIN)
    crop = reader.register(maps, info)
    args = (crop, o["height_map_mm"], tab["contact_index"], tab["contacts"], tab["count"], cfg.depth_eps_mm)
    t_contacts = timed(lambda: sensor.contacts(K, index_plane=True))
    t_register = timed(lambda: reader.register(maps, info))
    t_measure = timed(lambda: reader.measure(*args, status=o["status"]))
    t_both = timed(lambda: reader.measure(reader.register(maps, info), *args[1:], status=o["status"]))
    t_session = timed(lambda: sensor.thermal(crop, K, MARGIN))
    r = reader.measure(*args, status=o["status"])
    rows, fr, tb = r["thermal"].cpu().numpy(), r["frame"].cpu().numpy(), tab["contacts"].cpu().numpy()
    used = ~np.isnan(rows[..., 0])
    box = (tb[..., 11] - tb[..., 9] + 1) * (tb[..., 12] - tb[..., 10] + 1)
    out = {"frame": n, "photograph": [PH, PW], "batch": batch, "max_contacts": K, "surround_margin_px": MARGIN, "calls": CALLS}
    for name, t in (("register", t_register), ("measure", t_measure), ("register_measure", t_both), ("contacts", t_contacts), ("session_thermal", t_session)):
        out.update({f"{name}_ms_median": t["median"], f"{name}_ms_min": t["min"], f"{name}_ms_max": t["max"]})
    out.update({"contacts_per_frame_mean": float(tab["count"].float().mean()), "rows_measured": int(used.sum()), "box_px_max": float(box[used].max()),
                "box_px_mean": float(box[used].mean()), "registered_share": float(fr[:, 0].mean() / (n * n)),
                "contrast_C_mean": float(np.nanmean(rows[..., 11])), "register_bytes": int(batch * n * n * 4 * 2), "measure_frame_bytes": int(batch * n * n * 9)})
    print(json.dumps(out), flush=True)


if WHICH in ("small", "both"):
    run(224, 256, pkg.FtpConfig.scaled(224), 16)
if WHICH in ("native", "both"):
    run(1182, 8, pkg.FtpConfig.as_shipped(), 4)
