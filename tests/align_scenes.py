"""Synthetic frames for the alignment tests (test_align_surface.py, test_align_oracle.py): uint8 BGR scenes built in the test,
so the tests cover any frame size, ROI and shift without data files.

* dark_scene: hard-edged discs and rectangles plus a square-wave fringe patch on a black background.  The black background keeps the
  window's own (shared, unshifted) energy low, so the phase correlation of a rolled copy has a clear peak at the roll.
* smooth_frame: a smooth analytic texture rendered, in float64, at exactly rotated and translated coordinates (the ECC known answer).
"""
import numpy as np

from oracle import align_oracle as A
from oracle import cvlite


def _colour(g, rng):
    c = rng.uniform(0.5, 1.0, 3)
    return np.clip(np.rint(g[..., None] * c), 0, 255).astype(np.uint8)


def dark_scene(H, W, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    g = np.zeros((H, W))
    fr = (yy > H * 0.55) & (xx < W * 0.45)
    g[fr] = np.where(((xx[fr] + yy[fr] // 3) // 4) % 2 == 0, 40.0, 90.0)
    for _ in range(max(10, H * W // 2500)):
        cx, cy, r = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(2, 7)
        g = np.where((xx - cx) ** 2 + (yy - cy) ** 2 <= r * r, rng.uniform(60, 250), g)
        x0, y0 = rng.integers(0, W), rng.integers(0, H)
        g[y0:y0 + rng.integers(2, 12), x0:x0 + rng.integers(2, 12)] = rng.uniform(60, 250)
    return _colour(g, rng)


def rolled(frame, dy, dx):
    return np.ascontiguousarray(np.roll(frame, (dy, dx), axis=(0, 1)))


def _texture(u, v):
    return (128.0 + 50.0 * np.sin(2 * np.pi * u / 41.0 + 0.4) * np.sin(2 * np.pi * v / 37.0)
            + 35.0 * np.cos(2 * np.pi * (0.6 * u - 0.8 * v) / 29.0) + 25.0 * np.sin(2 * np.pi * (0.3 * u + 0.95 * v) / 53.0 + 1.1))


def smooth_frame(H, W, theta=0.0, tx=0.0, ty=0.0):
    """grey texture f as BGR (equal channels, so BGR2GRAY returns it unchanged) at I(p) = f(R(-theta) (p - t)): the ECC warp
    that maps the template (theta = 0, t = 0) into this frame is [[cos, -sin, tx], [sin, cos, ty]]"""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    c, s = np.cos(theta), np.sin(theta)
    px, py = xx - tx, yy - ty
    g = np.clip(np.rint(_texture(c * px + s * py, -s * px + c * py)), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(g[..., None], 3, axis=2))


def gauss_ksize(sigma):
    """cv::GaussianBlur's ksize for a float32 source: cvRound(8 sigma + 1) | 1"""
    return int(np.rint(sigma * 8 + 1)) | 1


def _blurred_pair(ref_bgr, def_bgr, sigma, generation):
    a = cvlite.gaussian_blur(A.bgr2gray_u8(ref_bgr, generation).astype(np.float32), sigma)
    b = cvlite.gaussian_blur(A.bgr2gray_u8(def_bgr, generation).astype(np.float32), sigma)
    return a, b


def float32_shift(ref_bgr, def_bgr, sigma=7.0, generation=4):
    """the oracle's phase correlation with its FFTs in float32 (scipy.fft's pocketfft keeps float32 inputs in float32) instead of
    float64: a second float32 transform, reproducible on any CPU, whose rounding differs from hipFFT's.  The whitening gives every bin
    unit weight, also the bins past the blur's passband that hold only rounding noise, so this shows how far float32 rounding alone
    moves the shift of a scene."""
    import scipy.fft as F
    a, b = _blurred_pair(ref_bgr, def_bgr, sigma, generation)
    h, w = a.shape
    M, N = A._optimal_dft_size(h), A._optimal_dft_size(w)
    win = A.hanning_window(h, w)
    pa = np.zeros((M, N), np.float32)
    pb = np.zeros((M, N), np.float32)
    pa[:h, :w] = a * win
    pb[:h, :w] = b * win
    p = F.rfft2(pa, workers=1) * np.conj(F.rfft2(pb, workers=1))
    assert p.dtype == np.complex64
    mag = np.abs(p)
    c = np.where(mag > 0, p / np.maximum(mag, np.finfo(np.float32).tiny), 0).astype(np.complex64)
    corr = F.irfft2(c, s=(M, N), workers=1) * np.float32(M * N)
    return A.peak_centroid(np.fft.fftshift(corr).astype(np.float32))[0]


def peak_margin(ref_bgr, def_bgr, sigma=7.0, generation=4):
    """(top / best value outside the 5x5 box around it, (py, px), (M, N)) of the oracle's fftshifted correlation surface"""
    a, b = _blurred_pair(ref_bgr, def_bgr, sigma, generation)
    c = A.correlation_surface(a, b, A.hanning_window(*a.shape))
    py, px = np.unravel_index(int(np.argmax(c)), c.shape)
    rest = c.copy()
    rest[max(0, py - 2):py + 3, max(0, px - 2):px + 3] = -np.inf
    return float(c[py, px] / rest.max()), (int(py), int(px)), c.shape
