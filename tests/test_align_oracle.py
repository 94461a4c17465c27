"""The alignment oracle (oracle/align_oracle.py) against known answers, on the CPU: the GPU alignment tests compare the kernels
with this oracle, so it is pinned here by something other than its sibling kernel.

A smooth analytic texture is rendered in float64 at exactly rotated and translated coordinates (tests/align_scenes.py) and rounded to
uint8 (300 x 300: on a 200 x 200 crop the texture's own bias reaches 2.5e-4 rad); with the global shift off, ECC (euclidean) must recover the rotation within 1e-4 rad and the translation within 5e-2 px.
"""
import numpy as np
import pytest

from align_scenes import smooth_frame
from oracle import align_oracle as A

ECC_CASES = [(2e-3, 1.5, -2.0), (-6e-3, -3.0, 2.5), (1e-2, 2.0, 3.0)]


@pytest.mark.parametrize("theta,tx,ty", ECC_CASES)
def test_oracle_ecc_recovers_a_known_rigid_motion(theta, tx, ty):
    ref = smooth_frame(300, 300)
    mov = smooth_frame(300, 300, theta, tx, ty)
    rg, dg, circle, info = A.aligned_crops_arrays(ref, mov, (150, 150, 150), apply_global_shift=False)
    assert circle == (150, 150, 149) and rg.shape == (300, 300) and np.array_equal(rg, ref[..., 0])
    assert not info["ecc_failed"] and 2 <= info["ecc_iters"] < 300
    w = info["warp"].astype(np.float64)
    assert abs(np.arcsin(w[1, 0]) - theta) <= 1e-4, (np.arcsin(w[1, 0]), theta)
    assert abs(w[0, 2] - tx) <= 5e-2 and abs(w[1, 2] - ty) <= 5e-2, (w[:, 2], tx, ty)
    # the aligned crop is the template again, away from the border the motion brings in
    d = np.abs(dg.astype(np.int16) - rg.astype(np.int16))[10:-10, 10:-10]
    assert d.max() <= 2, int(d.max())


def test_oracle_record_without_ecc_and_on_failure():
    """ECC off: identity warp, rho -1, 0 iterations, as vistaf_align_batch records; a blank frame: NaN rho, failed on iteration 1"""
    ref = smooth_frame(64, 64)
    _, dg, _, info = A.aligned_crops_arrays(ref, smooth_frame(64, 64, 0, 1.0, 0), (32, 32, 30), apply_global_shift=False, use_ecc=False)
    assert info["rho"] == -1.0 and info["ecc_iters"] == 0 and not info["ecc_failed"] and np.array_equal(info["warp"], np.eye(2, 3))
    blank = np.full_like(ref, 90)
    _, dg, _, info = A.aligned_crops_arrays(ref, blank, (32, 32, 30), apply_global_shift=False)
    assert info["ecc_failed"] and np.isnan(info["rho"]) and info["ecc_iters"] == 1 and (dg == 90).all()
