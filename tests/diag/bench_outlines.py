#!/usr/bin/env python
"""Timing of the contact outline read-out (outline.contact_outlines, K = 8): HIP-event time of the call alone, warm, median of the calls with
min and max, with and without polylines, next to `FtpSensor.contacts(8, index_plane=True)` of the same run -- the call that produces what the
read-out reads.  Batch 256 of 224 x 224 multi-contact frames (scaled constants), the frames' real contacts; the longest and the mean
principal loop of the run and the workspace bytes per frame are printed beside the times, since the ranking's work is proportional to the
edges.  python tests/diag/bench_outlines.py [calls]"""
import importlib, json, os, statistics, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("vistaf-roboskin-vision-integrated-multimodal-sensor_amd")
import contacts_helpers as H
G = os.path.join(ROOT, "tests", "golden")
CALLS = int(sys.argv[1]) if len(sys.argv) > 1 else 30
K = 8
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
    mpp = o["scalars"][:, 6].contiguous()
    ws = pkg.outline.OutlineWorkspace(n, n, batch, K)
    args = (tab["contact_index"], tab["contacts"], tab["count"], mpp)
    t_contacts = timed(lambda: sensor.contacts(K, index_plane=True))
    t_records = timed(lambda: pkg.contact_outlines(*args, max_vertices=0, workspace=ws))
    t_measure = timed(lambda: pkg.contact_outlines(*args, workspace=ws))
    t_session = timed(lambda: sensor.outlines(K))
    out = pkg.contact_outlines(*args, workspace=ws)["outlines"].cpu().numpy()
    used = ~np.isnan(out[..., 0])
    print(json.dumps({"frame": n, "batch": batch, "max_contacts": K, "calls": CALLS,
                      "measure_ms_median": t_measure["median"], "measure_ms_min": t_measure["min"], "measure_ms_max": t_measure["max"],
                      "records_only_ms_median": t_records["median"], "records_only_ms_min": t_records["min"], "records_only_ms_max": t_records["max"],
                      "contacts_ms_median": t_contacts["median"], "contacts_ms_min": t_contacts["min"], "contacts_ms_max": t_contacts["max"],
                      "session_outlines_ms_median": t_session["median"], "session_outlines_ms_min": t_session["min"],
                      "session_outlines_ms_max": t_session["max"], "workspace_bytes_per_frame": ws.nbytes // batch,
                      "rows_measured": int(used.sum()), "edges_max": float(out[..., 3][used].max()), "edges_mean": float(out[..., 3][used].mean()),
                      "pixels_max": float(out[..., 0][used].max()), "hull_vertices_max": float(out[..., 9][used].max()),
                      "overflow_rows": int((out[..., 8][used] < out[..., 7][used]).sum())}), flush=True)


run(224, 256, pkg.FtpConfig.scaled(224), 16)
