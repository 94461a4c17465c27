"""The 16-wave window march (k_inpaint_mw.hip) runs its two FMM passes -- outside the hole and the ordering pass over it -- at the same time
on two halves of the workgroup when the scratch of both, sized from the window's ring, band and hole cell counts, fits in LDS, and one after
the other on all 16 waves when it does not.  Both layouts must give the single-wave tiers' plane bit for bit, and so must the frames that
the 16-wave tier hands back."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")

# k_inpaint_mw.hip: window cells, generation entries, pass scratch (region A + the image plane) in bytes
MW_CELLS, GP_GEN, MW_SCRATCH = 10752, 2048, 4096 * 8 + 10752 * 4


@pytest.fixture(scope="module")
def cal(pkg):
    model, neg = pkg.load_calibration(os.path.join(G, "calibration_phase_to_height.json"))
    fm = pkg.load_force_calibration(os.path.join(G, "calibration_height_to_force.json"))["best_model"]
    return model, neg, fm


def _dilate(m, dy_max, dx_max, cross=False):
    out = m.copy()
    H, W = m.shape
    for dy in range(-dy_max, dy_max + 1):
        for dx in range(-dx_max, dx_max + 1):
            if cross and abs(dy) + abs(dx) != 1:
                continue
            s = np.zeros_like(m)
            s[max(0, dy):H + min(0, dy), max(0, dx):W + min(0, dx)] = m[max(0, -dy):H + min(0, -dy), max(0, -dx):W + min(0, -dx)]
            out |= s
    return out


def _layout(bad, rng):
    """Which path the 16-wave kernel takes for a frame's hole mask: its decision restated from the cell counts."""
    ys, xs = np.where(bad)
    if not len(ys):
        return "empty"
    m = rng + 1
    if (ys.max() - ys.min() + 1 + 2 * m) * (xs.max() - xs.min() + 1 + 2 * m) > MW_CELLS:
        return "window"
    band = _dilate(bad, 1, 1, cross=True) & ~bad
    ring = _dilate(bad, rng, rng) & ~bad & ~band
    nhole, nband, nring = int(bad.sum()), int(band.sum()), int(ring.sum())
    if nband > GP_GEN:
        return "generation"
    go, gh = min(GP_GEN, max(nband, nring)), min(GP_GEN, max(nband, nhole))
    need = 8 * (nring + nhole + go + gh) + 4 * (go + gh) + GP_GEN * 4 // 8
    return "concurrent" if need <= MW_SCRATCH else "sequential"


def test_concurrent_and_sequential_passes_match_the_single_wave_tiers(pkg, cal):
    n, nb = 224, 8
    cfg = pkg.FtpConfig.scaled(n)
    ref = pkg.synth.reference_frame(n, config=3)
    sensor = pkg.FtpSensor(ref, pkg.synth.roi_circle(n), cfg, cal[0], cal[1], cal[2], max_batch=nb)
    frames = pkg.synth.deformed_batch(n, 900, nb, config=3).copy()
    # lattices of saturated dots (each becomes a 5 x 5 hole blob): more dots, more ring and band cells per window
    for b, (side, step) in {1: (5, 12), 2: (6, 12), 3: (7, 12), 4: (8, 11), 5: (7, 11), 6: (11, 8)}.items():
        o = 112 - (side - 1) * step // 2
        for i in range(side):
            for j in range(side):
                frames[b][o + i * step, o + j * step] = 255
    yy, xx = np.mgrid[0:n, 0:n]
    frames[7][(yy - 110) ** 2 + (xx - 115) ** 2 <= 24 ** 2] = 255          # one large hole: many fills, few ring cells
    out = sensor.predict_batch(frames)
    torch.cuda.synchronize()
    img1 = sensor.intermediate("img", nb).cpu().numpy().reshape(nb, n, n).copy()
    bad = sensor.intermediate("bad1", nb, torch.uint8).cpu().numpy().reshape(nb, n, n) != 0
    st1 = out["status"].cpu().numpy().copy()
    kinds = [_layout(bad[b], int(round(cfg.bad_inpaint_radius))) for b in range(nb)]
    assert "concurrent" in kinds and "sequential" in kinds, kinds
    sensor._test_set("telea_mw", 0)
    out0 = sensor.predict_batch(frames)
    torch.cuda.synchronize()
    img0 = sensor.intermediate("img", nb).cpu().numpy().reshape(nb, n, n)
    assert np.array_equal(st1, out0["status"].cpu().numpy())
    for b in range(nb):
        assert np.array_equal(img1[b], img0[b]), (b, kinds[b])


def test_concurrent_passes_on_a_full_batch(pkg, cal):
    """The bench's batch (256 frames of 224 x 224, scaled constants): every frame that takes the concurrent layout equals the single-wave
    tiers bit for bit."""
    n, nb = 224, 256
    cfg = pkg.FtpConfig.scaled(n)
    ref = pkg.synth.reference_frame(n, config=3)
    sensor = pkg.FtpSensor(ref, pkg.synth.roi_circle(n), cfg, cal[0], cal[1], cal[2], max_batch=nb)
    frames = np.concatenate([pkg.synth.deformed_batch(n, 3000, nb // 2, config=3), pkg.synth.deformed_batch(n, 4000, nb // 2, config=3, amp_scale=1.6)])
    sensor.predict_batch(frames)
    torch.cuda.synchronize()
    img1 = sensor.intermediate("img", nb).cpu().numpy().reshape(nb, n, n).copy()
    bad = sensor.intermediate("bad1", nb, torch.uint8).cpu().numpy().reshape(nb, n, n) != 0
    kinds = [_layout(bad[b], int(round(cfg.bad_inpaint_radius))) for b in range(nb)]
    assert kinds.count("concurrent") >= nb // 2, kinds
    sensor._test_set("telea_mw", 0)
    sensor.predict_batch(frames)
    torch.cuda.synchronize()
    assert np.array_equal(img1, sensor.intermediate("img", nb).cpu().numpy().reshape(nb, n, n))
