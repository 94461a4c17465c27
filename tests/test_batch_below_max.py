"""A session carves its scratch buffers at the call's batch inside buffers sized for `max_batch` (the *_scratch() layouts of kernels.hpp).
Batches below `max_batch` must give, byte for byte, what a session created for exactly that batch gives -- on every path that carves:
the three inpaint tiers, the consistency check and the floods behind it, the k_big.hip chains.  No oracle: session against session."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def cal(pkg):
    model, neg = pkg.load_calibration(os.path.join(G, "calibration_phase_to_height.json"))
    fm = pkg.load_force_calibration(os.path.join(G, "calibration_height_to_force.json"))["best_model"]
    return model, neg, fm


def _session(pkg, cal, n, ref, max_batch, hooks):
    cfg = pkg.FtpConfig.scaled(n)
    sensor = pkg.FtpSensor(ref, pkg.synth.roi_circle(n), cfg, cal[0], cal[1], cal[2], max_batch=max_batch)
    for name, value in hooks.items():
        sensor._test_set(name, value)
    return sensor


def _outputs(pkg, sensor, frames, flood):
    """One predict and what it returned.  flood: the check is off, so the flood must have run in THIS predict.  Its by-product, the parent plane,
    is the evidence: a pixel has a parent exactly where this predict's unwrapped plane is a number.  Every predict of a session gets other
    frames, hence another reliable mask, so a plane left over from the predict before (or never written: all zeros) does not match."""
    nb = len(frames)
    out = sensor.predict_batch(frames)
    torch.cuda.synchronize()
    got = {key: out[key].cpu().numpy().copy() for key in ("height_map_mm", "output_reliable", "scalars", "status")}
    got["unwrapped"] = sensor.intermediate("unwrapped", nb).cpu().numpy().copy()
    assert (got["status"] == 0).all() and (got["scalars"][:, pkg.SCALAR_NAMES.index("bad_pixels")] > 0).all(), (nb, got["status"])
    if flood:
        got["parent"] = sensor.intermediate("parent", nb, torch.int32).cpu().numpy().copy()
        reached = got["parent"].reshape(nb, -1) >= 0
        assert reached.any(axis=1).all() and np.array_equal(reached, ~np.isnan(got["unwrapped"].reshape(nb, -1))), nb
    return got


@pytest.mark.parametrize("n,max_batch,batches,hooks", [
    (64, 5, (2, 5, 1), {}),
    (64, 5, (2, 5, 1), {"inpaint_tier": 0, "unwrap_fast": 0}),       # cluster front end + big-cluster march; batched flood in LDS
    (64, 5, (2, 5, 1), {"inpaint_tier": 1, "unwrap_fast": 0}),       # whole-frame march
    (256, 3, (2,), {"unwrap_fast": 0}),                              # 66 564 padded pixels: 32-bit ranks and the bitmap flood
    (512, 2, (1,), {}),                                              # the k_big.hip chains
], ids=["64-defaults", "64-clusters-flood", "64-wholeframe-flood", "256-bitmap-flood", "512-chains"])
def test_batches_below_max_batch_equal_a_session_of_that_batch(pkg, cal, n, max_batch, batches, hooks):
    """The synthetic 64 x 64 frames do have bad pixels (about a hundred per frame after the dilation), so the inpaint stage runs at that size."""
    flood = hooks.get("unwrap_fast") == 0
    ref = pkg.synth.reference_frame(n)
    wide = _session(pkg, cal, n, ref, max_batch, hooks)
    for k, nb in enumerate(batches):
        frames = pkg.synth.deformed_batch(n, 20 * k, nb)
        got = _outputs(pkg, wide, frames, flood)
        fresh = _session(pkg, cal, n, ref, nb, hooks)
        want = _outputs(pkg, fresh, frames, flood)
        if flood:       # never written: the check was off from the fresh session's first predict on
            assert (fresh.intermediate("unwrap_need", nb, torch.int32).cpu().numpy() == -1).all()
        for key in want:
            assert got[key].tobytes() == want[key].tobytes(), (nb, key)
