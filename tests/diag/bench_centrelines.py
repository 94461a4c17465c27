#!/usr/bin/env python
"""Timing of the centreline read-out (centreline.contact_centrelines, K = 8): HIP-event time of the call alone, warm, median of the calls with
min and max, with and without polylines and skeleton plane, next to the outline read-out, `FtpSensor.contacts(8, index_plane=True)` and
`predict_batch` of the same run.  Batch 256 of 224 x 224 multi-contact frames (scaled constants), the frames' real contacts -- the scene of
bench_outlines.py -- and a variant with one long cable per frame on a hand-made plane, because thinning passes grow with half the width and
walk levels with the length.  The largest THINNING_PASSES and STATIONS of each scene are printed beside the times.
python tests/diag/bench_centrelines.py [calls]"""
import importlib, json, os, statistics, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("vistaf-roboskin-vision-integrated-multimodal-sensor_amd")
import centreline_helpers as CL
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


def spread(prefix, t):
    return {prefix + "_ms_median": t["median"], prefix + "_ms_min": t["min"], prefix + "_ms_max": t["max"]}


def report(scene, n, batch, args, depth, ws, extra):
    t_records = timed(lambda: pkg.contact_centrelines(*args, depth, max_stations=0, skeleton=False, workspace=ws))
    t_measure = timed(lambda: pkg.contact_centrelines(*args, depth, workspace=ws))
    out = pkg.contact_centrelines(*args, depth, workspace=ws)["centrelines"].cpu().numpy()
    used = ~np.isnan(out[..., 0])
    row = {"scene": scene, "frame": n, "batch": batch, "max_contacts": K, "calls": CALLS}
    row.update(spread("measure", t_measure))
    row.update(spread("records_only", t_records))
    row.update(extra)
    row.update({"workspace_bytes_per_frame": ws.nbytes // batch, "rows_measured": int(used.sum()),
                "thinning_passes_max": float(out[..., CL.F["thinning_passes"]][used].max()), "stations_max": float(out[..., CL.F["stations"]][used].max()),
                "stations_mean": float(out[..., CL.F["stations"]][used].mean()), "pixels_max": float(out[..., 0][used].max()),
                "branched_rows": int((out[..., CL.F["status"]][used].astype(int) & CL.BRANCHED != 0).sum()),
                "overflow_rows": int((out[..., CL.F["stations_written"]][used] < out[..., CL.F["stations"]][used]).sum())})
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
    ws = pkg.centreline.CentrelineWorkspace(n, n, batch, K)
    ows = pkg.outline.OutlineWorkspace(n, n, batch, K)
    args = (tab["contact_index"], tab["contacts"], tab["count"], mpp)
    extra = {}
    extra.update(spread("predict_batch", timed(lambda: sensor.predict_batch(frames))))
    sensor.predict_batch(frames)
    extra.update(spread("contacts", timed(lambda: sensor.contacts(K, index_plane=True))))
    extra.update(spread("outlines", timed(lambda: pkg.contact_outlines(*args, workspace=ows))))
    extra.update(spread("session_centrelines", timed(lambda: sensor.centrelines(K))))
    report("contacts of the multi-contact frames", n, batch, args, depth, ws, extra)
    # one long cable per frame: a sine of 16 distinct amplitudes and thicknesses across the whole frame, on a hand-made plane and table
    scenes = [CL.Scene(n, n, K).paint(0, CL.sine_cable(n, n, 20 + 4 * (i % 4), 90 + 10 * (i // 4), 5 + 2 * (i % 3))) for i in range(distinct)]
    c = CL.pack(scenes * (batch // distinct), 0.05)
    cargs = tuple(torch.as_tensor(c[k]).cuda() for k in ("index", "tab", "count", "mpp"))
    report("one cable across each frame", n, batch, cargs, depth, ws,
           spread("outlines", timed(lambda: pkg.contact_outlines(*cargs, workspace=ows))))


run(224, 256, pkg.FtpConfig.scaled(224), 16)
