"""The element-wise passes around a short Gaussian blur (at most 15 taps) run inside the blur's LDS tile (k_blurchain.hip) instead of as
streaming kernels of their own: illumination normalise -> pre-blur -> apodise; masked values and mask -> reliable-only smoothing -> division;
frontier taper -> unreliable-region blur -> clamp -> mm curve.  The fused kernels call the same per-pixel expressions (pixel_ops.hpp) and run
the same taps in the same order, so a session with the hook "fused_chains" at 1 (default) must equal one with it at 0 (the kernel sequence)
bit for bit: outputs and the planes the chains leave behind.  No tolerance applies."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
PLANES = (("iw", torch.float32), ("hmap", torch.float32), ("unitless", torch.float32), ("kept", torch.uint8))


@pytest.fixture(scope="module")
def cal(pkg):
    model, neg = pkg.load_calibration(os.path.join(G, "calibration_phase_to_height.json"))
    fm = pkg.load_force_calibration(os.path.join(G, "calibration_height_to_force.json"))["best_model"]
    return model, neg, fm


def _bits(t):
    """the tensor's bytes: equal bytes is equal bits, NaN payloads and signed zeros included"""
    return t.detach().cpu().contiguous().numpy().view(np.uint8)


def _run(pkg, cal, cfg, n, frames, fused, refs=None):
    nb = len(frames)
    if refs is not None:      # room for both frame sets in the workspace
        sensor = pkg.FtpSensor(None, pkg.synth.roi_circle(n), cfg, cal[0], cal[1], cal[2], max_batch=2 * nb, frame_shape=(n, n))
    else:
        sensor = pkg.FtpSensor(pkg.synth.reference_frame(n, config=3), pkg.synth.roi_circle(n), cfg, cal[0], cal[1], cal[2], max_batch=nb)
    sensor._test_set("fused_chains", fused)
    out = sensor.predict_pairs(refs, frames) if refs is not None else sensor.predict_batch(frames)
    torch.cuda.synchronize()
    got = {k: _bits(out[k]) for k in ("height_map_mm", "output_reliable", "scalars", "status")}
    got["nan"] = np.isnan(out["height_map_mm"].cpu().numpy())
    for name, dt in PLANES:
        got["plane:" + name] = _bits(sensor.intermediate(name, nb, dt))
    sensor.close()
    return got


def _compare(pkg, cal, cfg, n, frames, refs=None):
    a = _run(pkg, cal, cfg, n, frames, 1, refs)
    b = _run(pkg, cal, cfg, n, frames, 0, refs)
    assert a["nan"].any() and not a["nan"].all()          # a real map: NaN outside the ROI, values inside
    for k in a:
        assert a[k].shape == b[k].shape, k
        ndiff = int(np.count_nonzero(a[k] != b[k]))
        print("%-18s %9d bytes, %d differ" % (k, a[k].size, ndiff))
        assert ndiff == 0, (k, ndiff)


def test_scaled_224_all_three_chains(pkg, cal):
    """The bench's constants: 3, 5 and 15 taps, all three chains fuse."""
    n = 224
    _compare(pkg, cal, pkg.FtpConfig.scaled(n), n, pkg.synth.deformed_batch(n, 900, 8, config=3))


def test_side_not_a_multiple_of_the_tile(pkg, cal):
    """200 x 200: partial tiles at the right and bottom edges, the reflected border inside a tile's halo."""
    n = 200
    _compare(pkg, cal, pkg.FtpConfig.scaled(n), n, pkg.synth.deformed_batch(n, 901, 8, config=3))


def test_as_shipped_224_only_the_pre_blur_fuses(pkg, cal):
    """The shipped constants at 224 x 224 have 13, 21, 49 and 73 taps: only illumination normalise -> pre-blur -> apodise fuses, the other
    chains stay on the kernel sequence with either setting."""
    n = 224
    _compare(pkg, cal, pkg.FtpConfig.as_shipped(), n, pkg.synth.deformed_batch(n, 902, 8, config=3))


def test_predict_pairs(pkg, cal):
    """Pair mode: both frame sets go through the preprocessing chain in the same launches."""
    n, nb = 224, 4
    refs = np.stack([pkg.synth.reference_frame(n, config=3)] * nb)
    _compare(pkg, cal, pkg.FtpConfig.scaled(n), n, pkg.synth.deformed_batch(n, 903, nb, config=3), refs=refs)
