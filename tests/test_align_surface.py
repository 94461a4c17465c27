"""The GPU alignment (csrc/align.hip through FtpAligner) against its CPU restatement (oracle/align_oracle.py) away from the one geometry
of test_align_gpu.py: frame sizes that need a zero-padded (and odd) FFT, ROI circles clipped by the frame, correlation peaks at the
border of the fftshifted plane, every config branch, ECC iteration by iteration, batches and handle reuse, every BGR triple, refusals.

All frames are synthetic uint8 BGR scenes built here (tests/align_scenes.py); each case runs the GPU and the oracle on the same arrays.

The phase correlation is checked against the oracle, not against the truth (the reference's estimator is not truth-recovering on
synthetic scenes), in two steps, as in test_align_gpu.py:
(a) shift: within 2e-2 px of the oracle's and the same multiple of 1/32 px, on scenes where that is well posed, which is asserted:
    the oracle's surface has a clear single maximum (the top value exceeds the best one outside its 5x5 box by MARGIN), and the
    shift is stable under float32 rounding.  The whitening gives every bin of the cross-power spectrum unit weight, also the bins
    past the blur's passband that hold nothing but rounding noise, so two float32 FFTs of the same frames can put the centroid
    0.03 .. 0.3 px apart (measured: a float32 CPU FFT against the float64 oracle, on corner peaks at sigma 3 and 7).  A scene is used
    only when a second float32 transform (align_scenes.float32_shift) lands within F32_SPREAD of the oracle and the oracle's shift
    lies at least twice that far from a 1/32 px rounding tie; F32_SPREAD is a quarter of the bar;
(b) crop: warping the frame with the GPU's own float32 shift through the oracle's warpAffine and cropping gives the GPU crop bit for bit.
"""
import ctypes

import numpy as np
import pytest
import torch

from align_scenes import dark_scene, float32_shift, gauss_ksize, peak_margin, rolled, smooth_frame
from oracle import align_oracle as A

pytestmark = pytest.mark.gpu

MARGIN = 1.3
F32_SPREAD = 5e-3
GEN = {0: 4, 1: 3}          # gray_coeffs -> oracle BGR2GRAY generation


def _oracle(ref, dfr, circle, apply_global_shift=True, use_ecc=True, ecc_iters=300, ecc_eps=1e-7, ecc_gauss_sigma=5.0, gray_coeffs=0,
            shift_blur_sigma=7.0):
    return A.aligned_crops_arrays(ref, dfr, circle, apply_global_shift, use_ecc, ecc_iters, ecc_eps, ecc_gauss_sigma, GEN[gray_coeffs],
                                  shift_blur_sigma)


def _check_geometry(al, ref, circle, gray_coeffs=0):
    (x1, x2, y1, y2), local = A.crop_geometry(ref.shape[0], ref.shape[1], circle)
    assert al.crop_box == (x1, y1, x2, y2) and al.crop_shape == (y2 - y1, x2 - x1)
    assert al.circle_crop == local
    assert np.array_equal(al.reference_gray_crop.cpu().numpy(), A.bgr2gray_u8(ref[y1:y2, x1:x2], GEN[gray_coeffs]))


def _check_shift(out, b, info_o, ref, dfr, sigma=7.0, gray_coeffs=0):
    """bar (a); returns the oracle surface's peak (py, px) and size (M, N)"""
    m, peak, shape = peak_margin(ref, dfr, sigma, GEN[gray_coeffs])
    assert m > MARGIN, ("ill-posed scene", m)
    g = np.asarray(out["shift"][b], np.float64)
    o = np.asarray(info_o["shift"], np.float64)
    spread = np.abs(np.asarray(float32_shift(ref, dfr, sigma, GEN[gray_coeffs])) - o).max()
    tie = np.abs((o * 32) % 1 - 0.5).min() / 32
    assert spread <= F32_SPREAD and tie >= 2 * max(spread, 2e-3), ("shift not stable under float32 rounding", spread, tie)
    # float32 FFTs of a whitened cross-power spectrum: the centroid moves by up to ~1e-2 px (test_align_gpu.py)
    assert np.abs(g - o).max() <= 2e-2, (g, o)
    assert np.array_equal(np.rint(g * 32), np.rint(o * 32)), (g, o)
    assert abs(out["response"][b] - info_o["response"]) <= 2e-2 * abs(info_o["response"]), (out["response"][b], info_o["response"])
    return peak, shape


def _shifted_crop(al, dfr, out, b, gray_coeffs=0):
    """bar (b): the oracle's warpAffine of the frame with the GPU's float32 shift, cropped and converted"""
    M = np.array([[1, 0, np.float32(out["shift"][b, 0])], [0, 1, np.float32(out["shift"][b, 1])]], np.float32)
    x1, y1, x2, y2 = al.crop_box
    return A.bgr2gray_u8(A.warp_affine(dfr, M, False, border="reflect")[y1:y2, x1:x2], GEN[gray_coeffs])


def _check_ecc_off_record(out, b):
    assert out["rho"][b] == -1.0 and out["ecc_iters"][b] == 0 and not out["ecc_failed"][b]
    assert np.array_equal(out["warp"][b], np.eye(2, 3))


def _check_ecc(out, b, info_o, exact_iters=True):
    assert bool(out["ecc_failed"][b]) == bool(info_o["ecc_failed"])
    if exact_iters:
        assert out["ecc_iters"][b] == info_o["ecc_iters"], (out["ecc_iters"][b], info_o["ecc_iters"])
    if info_o["ecc_failed"]:
        assert np.isnan(out["rho"][b]) and np.array_equal(out["warp"][b], np.eye(2, 3))
        return
    wg, wo = out["warp"][b], info_o["warp"].astype(np.float64)
    assert abs(np.arcsin(wg[1, 0]) - np.arcsin(wo[1, 0])) <= 2e-6, (wg, wo)                 # rad, as test_align_gpu.py
    assert abs(wg[0, 2] - wo[0, 2]) <= 2e-3 and abs(wg[1, 2] - wo[1, 2]) <= 2e-3, (wg, wo)   # px
    assert abs(out["rho"][b] - info_o["rho"]) <= 1e-5, (out["rho"][b], info_o["rho"])


def _check_crop_close(got, exp):
    # two bilinear uint8 warps with 1/32-pixel coordinate quantisation (test_align_gpu.py)
    d = np.abs(got.astype(np.int16) - exp.astype(np.int16))
    assert d.max() <= 3 and (d > 0).mean() <= 0.10 and (d > 1).mean() <= 2e-3, (int(d.max()), float((d > 0).mean()), float((d > 1).mean()))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. frame sizes: padded FFT (M != H or N != W), odd optimal sizes, a frame smaller than the blur radius.
# Blur sigma 3 (SHIFT_SIGMA) except on the small frame: at sigma 7 a second float32 FFT already moves the shift of these hard-edged
# frames by 0.004 .. 0.016 px, and on one frame that passed that check the GPU landed 0.0208 px from the oracle (measured); at
# sigma 3 the second transform stays within 2.5e-3 px.  The default sigma runs on the smooth pair of the config matrix (6).
SHIFT_SIGMA = 3.0
SIZES = [  # H, W, seed, roll (dy, dx), circle
    (480, 640, 2, (-23, 17), (320, 240, 180)),
    (433, 601, 3, (-23, 17), (300, 216, 180)),          # padded to 450 x 625
    (675, 1125, 1, (-12, -15), (562, 337, 180)),        # 675 = 3^3 5^2, 1125 = 3^2 5^3: odd M and N, no padding
    (17, 19, 1, (-12, -15), (9, 8, 6)),                 # padded to 18 x 20; blur radius 28 exceeds the frame
]


@pytest.mark.parametrize("H,W,seed,roll,circle", SIZES, ids=[f"{s[0]}x{s[1]}" for s in SIZES])
def test_frame_sizes_padded_and_odd_fft(pkg, H, W, seed, roll, circle):
    ref = dark_scene(H, W, seed)
    dfr = rolled(ref, *roll)
    if H < 32:
        assert gauss_ksize(7.0) // 2 > max(H, W)
    sigma = SHIFT_SIGMA if H >= 32 else 7.0
    al = pkg.FtpAligner(ref, circle=circle, use_ecc=False, shift_blur_sigma=sigma)
    _check_geometry(al, ref, circle)
    out = al.align(dfr)
    _, _, _, info_o = _oracle(ref, dfr, circle, use_ecc=False, shift_blur_sigma=sigma)
    _, shape = _check_shift(out, 0, info_o, ref, dfr, sigma)
    assert shape == (A._optimal_dft_size(H), A._optimal_dft_size(W))
    if H >= 32:             # the oracle finds the roll; the 17 x 19 frame, blurred past its size, keeps the window's zero-lag lobe
        assert np.abs(np.asarray(info_o["shift"]) - roll[::-1]).max() <= 1.0, info_o["shift"]
    assert np.array_equal(out["aligned_gray"][0].cpu().numpy(), _shifted_crop(al, dfr, out, 0))
    _check_ecc_off_record(out, 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. ROI circles clipped by the frame, with a shift whose warp reads outside the frame (BORDER_REFLECT in k_warp_u8); sigma 3 as in 1
BORDERS = [  # roll, circle, expected local circle
    ((17, 12), (60, 50, 120), (60, 50, 50)),            # clipped at the left and top, shift (+12, +17): reads x, y < 0
    ((-13, -16), (600, 440, 110), (110, 110, 39)),      # clipped at the right and bottom, shift (-16, -13): reads x >= W, y >= H
    ((17, 12), (320, 95, 100), (100, 95, 95)),          # clipped at the top only
]


@pytest.mark.parametrize("roll,circle,local", BORDERS, ids=["left-top", "right-bottom", "top"])
def test_roi_clipped_by_the_frame(pkg, roll, circle, local):
    ref = dark_scene(480, 640, 8)
    dfr = rolled(ref, *roll)
    al = pkg.FtpAligner(ref, circle=circle, use_ecc=False, shift_blur_sigma=SHIFT_SIGMA)
    _check_geometry(al, ref, circle)
    assert al.circle_crop == local
    out = al.align(dfr)
    _, _, lc, info_o = _oracle(ref, dfr, circle, use_ecc=False, shift_blur_sigma=SHIFT_SIGMA)
    assert lc == local
    _check_shift(out, 0, info_o, ref, dfr, SHIFT_SIGMA)
    assert np.abs(np.asarray(info_o["shift"]) - roll[::-1]).max() <= 1.0, info_o["shift"]
    x1, y1, x2, y2 = al.crop_box
    sx, sy = float(out["shift"][0, 0]), float(out["shift"][0, 1])
    assert x1 - sx < 0 or y1 - sy < 0 or x2 - 1 - sx > 639 or y2 - 1 - sy > 479       # the warp reads outside the frame
    assert np.array_equal(out["aligned_gray"][0].cpu().numpy(), _shifted_crop(al, dfr, out, 0))


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. correlation peak within 2 px of the border of the fftshifted plane: the 5x5 centroid window clamped at the top and the right, and
# at the bottom and the left.  Rolls by about half of a hard-edged frame put the peak there.  Blur sigma 2: at sigma 3 and 7 the
# float32 spread of these corner peaks is 0.006 .. 0.3 px (more bins of the whitened spectrum are rounding noise), past F32_SPREAD.
PEAKS = [  # H, W, seed, roll
    (480, 640, 3, (239, 322)),          # peak at (1, 638): clamped at the top and at the right
    (480, 640, 1, (242, 319)),          # peak at (478, 1): clamped at the bottom and at the left
]


@pytest.mark.parametrize("H,W,seed,roll", PEAKS, ids=["top-right", "bottom-left"])
def test_correlation_peak_at_the_plane_border(pkg, H, W, seed, roll):
    ref = dark_scene(H, W, seed)
    dfr = rolled(ref, *roll)
    circle = (W // 2, H // 2, 100)
    al = pkg.FtpAligner(ref, circle=circle, use_ecc=False, shift_blur_sigma=2.0)
    out = al.align(dfr)
    _, _, _, info_o = _oracle(ref, dfr, circle, use_ecc=False, shift_blur_sigma=2.0)
    (py, px), (M, N) = _check_shift(out, 0, info_o, ref, dfr, 2.0)
    assert min(py, M - 1 - py) <= 1 and min(px, N - 1 - px) <= 1, (py, px)      # the window reaches past the plane
    assert np.array_equal(out["aligned_gray"][0].cpu().numpy(), _shifted_crop(al, dfr, out, 0))


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. ECC iteration by iteration: eps = 0 never stops early, so both sides run exactly to the cap (the host polls every 8 iterations)
ECC_FRAME = dict(H=240, W=240, circle=(120, 120, 100), theta=5e-3, tx=2.2, ty=-1.4)


@pytest.fixture(scope="module")
def ecc_frames():
    f = ECC_FRAME
    return smooth_frame(f["H"], f["W"]), smooth_frame(f["H"], f["W"], f["theta"], f["tx"], f["ty"])


@pytest.mark.parametrize("iters", [1, 7, 8, 9, 13])
def test_ecc_capped_iterations(pkg, ecc_frames, iters):
    ref, dfr = ecc_frames
    circle = ECC_FRAME["circle"]
    al = pkg.FtpAligner(ref, circle=circle, apply_global_shift=False, ecc_iters=iters, ecc_eps=0.0)
    out = al.align(dfr)
    _, dg, _, info_o = _oracle(ref, dfr, circle, apply_global_shift=False, ecc_iters=iters, ecc_eps=0.0)
    assert info_o["ecc_iters"] == iters
    _check_ecc(out, 0, info_o)
    _check_crop_close(out["aligned_gray"][0].cpu().numpy(), dg)


def test_ecc_to_convergence(pkg, ecc_frames):
    ref, dfr = ecc_frames
    circle = ECC_FRAME["circle"]
    al = pkg.FtpAligner(ref, circle=circle, apply_global_shift=False)
    out = al.align(dfr)
    _, dg, _, info_o = _oracle(ref, dfr, circle, apply_global_shift=False)
    assert 2 <= info_o["ecc_iters"] < 300
    _check_ecc(out, 0, info_o)
    _check_crop_close(out["aligned_gray"][0].cpu().numpy(), dg)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. ECC known answer, independent of the oracle (the oracle alone: test_align_oracle.py)
@pytest.mark.parametrize("theta,tx,ty", [(2e-3, 1.5, -2.0), (-6e-3, -3.0, 2.5), (1e-2, 2.0, 3.0)])
def test_ecc_recovers_a_known_rigid_motion(pkg, theta, tx, ty):
    ref = smooth_frame(300, 300)
    mov = smooth_frame(300, 300, theta, tx, ty)
    al = pkg.FtpAligner(ref, circle=(150, 150, 150), apply_global_shift=False)
    out = al.align(mov)
    _, _, _, info_o = _oracle(ref, mov, (150, 150, 150), apply_global_shift=False)
    for w in (out["warp"][0], info_o["warp"].astype(np.float64)):
        assert abs(np.arcsin(w[1, 0]) - theta) <= 1e-4, (w, theta)
        assert abs(w[0, 2] - tx) <= 5e-2 and abs(w[1, 2] - ty) <= 5e-2, (w, tx, ty)
    assert not out["ecc_failed"][0] and 2 <= out["ecc_iters"][0] < 300


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. config matrix, each run against the oracle with the same arguments; ECC with ecc_eps = 0 and 8 iterations (past the host's first
# convergence poll), so that the iteration counts are exact.  With the default eps the stop is float-limited on this pair: the
# oracle's |rho - last_rho| is 4.9e-7, 3.0e-7, 9.2e-8 at iterations 21..23 (it stops at 23) and then wobbles between 2e-9 and 6e-8
# around rho = 0.999847 (measured), so a rounding difference of 1e-8 in rho moves the stop (the GPU stopped at 36 on a 480 x 640
# version of this pair).  Stopped at 12 iterations, mid-convergence, the rotations there were 3.0e-6 rad apart (measured).
# ECC runs on the smooth texture (on the sparse hard-edged scene it wanders off to 0.25 rad in the oracle too), at 600 x 800, where
# its phase correlation is stable under float32 rounding at sigma 7 and 30; sigma 3 runs on the hard-edged scene with ECC off.
CONFIGS = [dict(apply_global_shift=s, use_ecc=e) for s in (True, False) for e in (True, False)] + \
          [dict(ecc_gauss_sigma=g) for g in (0.0, 2.5)] + [dict(gray_coeffs=1)] + \
          [dict(shift_blur_sigma=3.0, use_ecc=False), dict(shift_blur_sigma=30.0)]


@pytest.fixture(scope="module")
def matrix_frames():
    hard = dark_scene(480, 640, 1)
    return {"smooth": (smooth_frame(600, 800), smooth_frame(600, 800, 4e-3, 1.7, -1.1)), "hard": (hard, rolled(hard, -9, 13))}


@pytest.mark.parametrize("cfg", CONFIGS, ids=["-".join(f"{k}={v}" for k, v in c.items()) for c in CONFIGS])
def test_config_matrix(pkg, matrix_frames, cfg):
    kw = dict(apply_global_shift=True, use_ecc=True, ecc_iters=8, ecc_eps=0.0, ecc_gauss_sigma=5.0, gray_coeffs=0, shift_blur_sigma=7.0)
    kw.update(cfg)
    ref, dfr = matrix_frames["hard" if kw["shift_blur_sigma"] == 3.0 else "smooth"]
    circle = (ref.shape[1] // 2, ref.shape[0] // 2, 100)
    if kw["shift_blur_sigma"] == 30.0:
        assert gauss_ksize(30.0) > 225                  # past the LDS column kernel (k_gauss_cols)
    al = pkg.FtpAligner(ref, circle=circle, **kw)
    _check_geometry(al, ref, circle, kw["gray_coeffs"])
    out = al.align(dfr)
    _, dg, _, info_o = _oracle(ref, dfr, circle, **kw)
    _check_shift(out, 0, info_o, ref, dfr, kw["shift_blur_sigma"], kw["gray_coeffs"])
    got = out["aligned_gray"][0].cpu().numpy()
    if not kw["use_ecc"]:
        _check_ecc_off_record(out, 0)
        if kw["apply_global_shift"]:
            assert np.array_equal(got, _shifted_crop(al, dfr, out, 0, kw["gray_coeffs"]))
        else:
            x1, y1, x2, y2 = al.crop_box
            assert np.array_equal(got, A.bgr2gray_u8(dfr[y1:y2, x1:x2], GEN[kw["gray_coeffs"]]))      # k_crop_bgr
        return
    assert not info_o["ecc_failed"] and info_o["ecc_iters"] == 8
    _check_ecc(out, 0, info_o)
    _check_crop_close(got, dg)


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. batches and handle reuse: per-frame done / failed flags, B < max_batch, repeated calls
def test_batch_equals_frames_alone_and_repeats(pkg):
    ref = smooth_frame(240, 240)
    frames = np.stack([smooth_frame(240, 240, 5e-3, 2.2, -1.4), smooth_frame(240, 240, -1e-2, -3.0, 1.0), np.full_like(ref, 90), ref.copy(),
                       smooth_frame(240, 240, 2e-3, 0.4, 0.3)])
    circle = (120, 120, 100)
    al = pkg.FtpAligner(ref, circle=circle, max_batch=8)
    o5 = al.align(frames)
    assert list(o5["ecc_failed"]) == [False, False, True, False, False]
    it = [int(v) for j, v in enumerate(o5["ecc_iters"]) if j != 2]
    assert len(set(it)) >= 3, it                         # frames of one batch converge at different iterations
    g5 = o5["aligned_gray"].cpu().numpy()
    again = al.align(frames)
    assert np.array_equal(again["aligned_gray"].cpu().numpy(), g5) and np.array_equal(again["info"], o5["info"], equal_nan=True)
    for b in range(len(frames)):
        one = al.align(frames[b])                        # B = 1 after B = 5 on the same handle
        assert np.array_equal(one["aligned_gray"][0].cpu().numpy(), g5[b]), b
        assert np.array_equal(one["info"][0], o5["info"][b], equal_nan=True), (b, one["info"][0], o5["info"][b])
    # the blank frame against the oracle: failed on iteration 1, the unaligned crop
    _, dg, _, info_o = _oracle(ref, frames[2], circle)
    _check_ecc(o5, 2, info_o)
    assert np.array_equal(g5[2], dg)
    # refusals: B > max_batch (Python and the C entry point), a frame of another size
    with pytest.raises(ValueError):
        al.align(np.concatenate([frames, frames]))
    big = torch.as_tensor(np.concatenate([frames, frames])).cuda()
    out = torch.empty((10,) + al.crop_shape, dtype=torch.uint8, device="cuda")
    info = torch.empty((10, 12), dtype=torch.float64, device="cuda")
    for B in (0, 9):
        rc = al._lib.vistaf_align_batch(al._h, ctypes.c_void_p(big.data_ptr()), B, ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(info.data_ptr()),
                                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc != 0, B
    with pytest.raises(RuntimeError):
        al.align(np.zeros((1, 240, 241, 3), np.uint8))
    # the handle still works after the refusals
    assert np.array_equal(al.align(frames[:2])["aligned_gray"].cpu().numpy(), g5[:2])


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. every BGR triple once: the reference crop is the whole 4096 x 4096 frame
@pytest.mark.parametrize("gray_coeffs", [0, 1])
def test_bgr2gray_every_triple(pkg, gray_coeffs):
    i = np.arange(1 << 24, dtype=np.uint32)
    frame = np.stack([i & 255, (i >> 8) & 255, i >> 16], -1).astype(np.uint8).reshape(4096, 4096, 3)
    al = pkg.FtpAligner(frame, circle=(2048, 2048, 2048), use_ecc=False, gray_coeffs=gray_coeffs)
    assert al.crop_box == (0, 0, 4096, 4096)
    assert np.array_equal(al.reference_gray_crop.cpu().numpy(), A.bgr2gray_u8(frame, GEN[gray_coeffs]))
    al.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 9. refusals of vistaf_align_create (include/vistaf_align.h), and the accepted boundaries
def test_create_refusals_and_boundaries(pkg):
    f = dark_scene(64, 64, 2)
    for frame, circle, kw in [
            (f[:15], (32, 7, 6), {}), (f[:, :15], (7, 32, 6), {}),       # H or W below 16
            (f, (32, 32, 3), {}),                                        # r below 4
            (f, (-2, 32, 9), {}), (f, (32, 70, 13), {}),                 # clipped crop under 8 px (7 wide; 7 high)
            (f, (32, 32, 20), dict(shift_blur_sigma=64.0)),              # 513 taps
            (f, (32, 32, 20), dict(ecc_gauss_sigma=64.0)),
            (f, (32, 32, 20), dict(shift_blur_sigma=0.0)),
            (f, (32, 32, 20), dict(ecc_iters=0)),
            (f, (32, 32, 20), dict(max_batch=0))]:
        with pytest.raises(ValueError):
            pkg.FtpAligner(frame, circle=circle, **kw)
    assert gauss_ksize(64.0) == 513 and gauss_ksize(63.8) == 511
    al = pkg.FtpAligner(f[:16, :16], circle=(8, 8, 4), ecc_iters=1, shift_blur_sigma=63.8, ecc_gauss_sigma=63.8)   # 16 px, r 4, 511 taps
    assert al.crop_shape == (8, 8)
    al2 = pkg.FtpAligner(f, circle=(4, 32, 4))                           # touching the left edge: an 8 x 8 crop
    assert al2.crop_shape == (8, 8) and al2.circle_crop == (4, 4, 3)
    out = al2.align(rolled(f, 1, 1))
    assert out["aligned_gray"].shape == (1, 8, 8)
