#!/usr/bin/env python
"""Timing of the lobe read-out (lobes.contact_lobes, K = 8, max_lobes = 4): HIP-event time of the call alone, warm, median of the calls with
min and max, with and without the split table and the lobe plane, next to `FtpSensor.contacts(8, index_plane=True)` and `predict_batch` of the
same run.  Batch 256 of 224 x 224 multi-contact frames (scaled constants), the frames' real contacts -- the scene of bench_centrelines.py --
at the default prominences and at tau = 0 (every raw maximum a peak), and a variant with one two-bump contact of 100 x 60 pixels per frame on
a hand-made plane, a box that leaves LDS.  The largest RAW_MAXIMA and PEAKS of each scene are printed beside the times: the serial replay is
RAW_MAXIMA - 1 steps.
python tests/diag/bench_lobes.py [calls]"""
import importlib, json, os, statistics, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("vistaf-roboskin-vision-integrated-multimodal-sensor_amd")
import contacts_helpers as H
import lobes_helpers as LH
G = os.path.join(ROOT, "tests", "golden")
CALLS = int(sys.argv[1]) if len(sys.argv) > 1 else 30
K, L = 8, 4
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


def spread(prefix, t):
    return {prefix + "_ms_median": t["median"], prefix + "_ms_min": t["min"], prefix + "_ms_max": t["max"]}


def report(scene, n, batch, args, depth, ws, eps, extra, **tau):
    t_records = timed(lambda: pkg.contact_lobes(*args, depth, L, depth_eps_mm=eps, split=False, lobe_index=False, workspace=ws, **tau))
    t_measure = timed(lambda: pkg.contact_lobes(*args, depth, L, depth_eps_mm=eps, workspace=ws, **tau))
    rows = pkg.contact_lobes(*args, depth, L, depth_eps_mm=eps, workspace=ws, **tau)["lobe_rows"].cpu().numpy()
    used = ~np.isnan(rows[..., 0])
    row = {"scene": scene, "frame": n, "batch": batch, "max_contacts": K, "max_lobes": L, "calls": CALLS}
    row.update(tau)
    row.update(spread("measure", t_measure))
    row.update(spread("records_only", t_records))
    row.update(extra)
    row.update({"workspace_bytes_per_frame": ws.nbytes // batch, "rows_measured": int(used.sum()),
                "raw_maxima_max": float(rows[..., LH.RF["raw_maxima"]][used].max()), "raw_maxima_mean": float(rows[..., LH.RF["raw_maxima"]][used].mean()),
                "peaks_max": float(rows[..., LH.RF["peaks"]][used].max()), "pixels_max": float(rows[..., 0][used].max()),
                "truncated_rows": int((rows[..., LH.RF["status"]][used].astype(int) & LH.TRUNCATED != 0).sum())})
    print(json.dumps(row), flush=True)


def run(n, batch, cfg, distinct):
    ref = pkg.synth.reference_frame(n)
    base = H.multi_contact_batch(pkg, n, 0, distinct)
    frames = torch.from_numpy(np.concatenate([base] * (batch // distinct))).cuda()
    sensor = pkg.FtpSensor(ref, pkg.synth.roi_circle(n), cfg, cal, neg, fm, max_batch=batch)
    o = sensor.predict_batch(frames)
    tab = sensor.contacts(K, index_plane=True)
    mpp = o["scalars"][:, 6].contiguous()
    depth = o["height_map_mm"]
    eps = sensor.config.depth_eps_mm
    ws = pkg.lobes.LobesWorkspace(n, n, batch, K)
    args = (tab["contact_index"], tab["contacts"], tab["count"], mpp)
    extra = {}
    extra.update(spread("predict_batch", timed(lambda: sensor.predict_batch(frames))))
    sensor.predict_batch(frames)
    extra.update(spread("contacts", timed(lambda: sensor.contacts(K, index_plane=True))))
    extra.update(spread("session_lobes", timed(lambda: sensor.lobes(K, L))))
    report("contacts of the multi-contact frames, default prominences", n, batch, args, depth, ws, eps, extra)
    report("the same, every raw maximum a peak", n, batch, args, depth, ws, eps, {}, min_prominence_mm=0.0, min_prominence_frac=0.0)
    # one merged two-bump contact per frame, 16 distinct separations, on a hand-made plane and table: a 100 x 60 box, which leaves LDS
    scenes, depths = [], []
    for i in range(distinct):
        d = LH.bumps(n, n, [(1.0, 80, 110), (0.7 + 0.01 * i, 120 + i, 108)], 900.0)
        scenes.append(LH.Scene(n, n, K).paint(0, LH.rect(n, n, 50, 80, 149, 139) & (d > 0.2)))
        depths.append(d)
    c = LH.pack(scenes * (batch // distinct), 0.05)
    c["tab"][:, 0, LH.C_FORCE] = 2.0
    cargs = tuple(torch.as_tensor(c[k]).cuda() for k in ("index", "tab", "count", "mpp"))
    cdepth = torch.as_tensor(np.stack(depths * (batch // distinct))).cuda()
    report("one merged two-bump contact of about 100 x 60 per frame (workspace tier)", n, batch, cargs, cdepth, ws, eps, {})


run(224, 256, pkg.FtpConfig.scaled(224), 16)
