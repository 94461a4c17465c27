"""Frames, constants and a stage-by-stage reference for the periodic-stripe segmentation of the temperature modality (csrc/tempseg.hip,
vistaf_tempseg_segment).  NumPy float64 on the primitives of oracle/temp_oracle.py and oracle/cvlite.py; no GPU.  The tests that use them are
in tests/test_tempseg_stages.py: a CPU test runs every stage function below on the oracle's own planes and finds the oracle's masks and numbers
again, exactly, so the staged reference IS the oracle; the GPU tests then hold every stage of the device against the stage function applied to
the device's own upstream plane.

Bound on the band-passed field z (bound_z).  The device forms z with four float64 matrix products (k_dft.hip): rows T = a Ex (a = inorm, real;
K = w real steps), columns patch = win (Ey T) (K = 2 h), then Q = patch Gx and z = Gy Q (K = 2 pm each, pm = 2 R + 1), the inverse tables
carrying 1 / (H W).  tests/test_dft_direct.py holds each such product to (K + 3) 2^-53 (|A| . |B|) per component.  Every table entry has
components of modulus at most 1 (times the scale), so with S = sum |a| over the frame and SP = sum over the nb bins of the disc of
|Re F| + |Im F| (F the reference spectrum):
    |T| <= S_row, |patch| <= 2 S per component;  patch error per component <= [2 (2 h + 3) + 2 (w + 3)] u S + table errors 4 u (2 S + 2 S)
    z error <= 2 nb (patch error) / (H W)  +  [2 (2 pm + 3) 2 + table errors 2 * 2 pi * 4 * 5 * 2] u SP / (H W)
(u = 2^-53; a forward table entry is good to 4 u, an inverse one to 2 pi 4 u (1 + |arg|) with |arg| < 4, kernel_refs.table_*_ref).  The float64
reference (np.fft) has its own error, for which 8 log2(H W) u of the same two magnitudes is added: pocketfft's error grows with log2 N and stays
far below that.  The bound is computed per case from the reference's sums; it is not a fixed number."""
import dataclasses
import functools

import numpy as np

from oracle import align_oracle as A
from oracle import cvlite as cv
from oracle import ftp_oracle as O
from oracle import temp_oracle as T

U = 2.0 ** -53


# =======================================================================================================================================
# frames

def roi_ellipse(h, w):
    """an ellipse that the frame cuts on all four sides: ROI rim and frame border both run through the stripes"""
    yy, xx = np.mgrid[0:h, 0:w]
    return ((xx - 0.5 * w) / (0.56 * w)) ** 2 + ((yy - 0.47 * h) / (0.62 * h)) ** 2 <= 1.0


def stripes(h, w, period, tilt=0.0, duty=0.5, seed=1):
    """BGR stripes of `period` px across x (phase advancing by tilt px per row), the bright part `duty` of a period, under a slow illumination
    field, with noise, a saturated disc inside the frame and a saturated half disc on the top border"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    s = 1.0 + 0.2 * np.cos(np.pi * np.hypot(xx - w / 2, yy - h / 2) / (0.7 * max(h, w)))
    bright = np.cos(2 * np.pi * (xx + tilt * yy) / period) > np.cos(np.pi * duty)
    g = 120.0 * s * (0.6 + 0.3 * np.where(bright, 1.0, -1.0)) + rng.normal(0, 3.0, (h, w))
    r = max(4.0, min(h, w) / 9.0)
    g[(xx - 0.6 * w) ** 2 + (yy - 0.45 * h) ** 2 <= r ** 2] = 255.0
    g[(xx - 0.31 * w) ** 2 + yy ** 2 <= (0.6 * r) ** 2] = 255.0
    g = np.clip(g, 0, 255)
    img = np.stack([0.9 * g, g, np.minimum(255.0, 1.05 * g)], axis=-1)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def tie_frame(h=96, w=203):
    """flat gray 100; a 29 x 61 patch at the centre with stripes of period 9 at 255 / 248 (all of it saturated: none of it in roi_eff); the ROI
    leaves out rows 0..3 and columns 0..4"""
    g = np.full((h, w), 100, np.uint8)
    xs = np.arange(w // 2 - 30, w // 2 + 31)
    g[h // 2 - 14:h // 2 + 15, xs] = np.where((xs % 9) < 5, 255, 248).astype(np.uint8)[None, :]
    roi = np.ones((h, w), bool)
    roi[:4] = False
    roi[:, :5] = False
    return np.repeat(g[..., None], 3, axis=2), roi


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    h: int
    w: int
    cfg: tuple                  # ((field, value), ..): the constants that differ from the defaults
    frame: tuple                # ("stripes", period, tilt, duty) or ("tie",)
    chosen: str = "B_is_dark"

    def config(self, cls):
        return cls(**dict(self.cfg))

    def image(self):
        if self.frame[0] == "tie":
            return tie_frame(self.h, self.w)
        _, period, tilt, duty = self.frame
        return stripes(self.h, self.w, period, tilt, duty, seed=self.h + self.w), roi_ellipse(self.h, self.w)


def _c(**kw):
    return tuple(sorted(kw.items()))


_TIE = dict(seg_band_radius=8, seg_dc_exclusion=14, seg_illum_sigma=0, sat_dilate_ksize=1, post_close_ky=9)
CASES = [
    Case("c1_64x64_bits", 64, 64, _c(seg_band_radius=5, seg_dc_exclusion=4, seg_illum_sigma=6, sat_dilate_ksize=5, post_close_ky=9, post_open_ky=5),
         ("stripes", 8.0, 0.0, 0.5)),
    # even sizes: odd_up makes them the constants of c1
    Case("c1_even_sizes", 64, 64, _c(seg_band_radius=5, seg_dc_exclusion=4, seg_illum_sigma=6, sat_dilate_ksize=4, post_close_kx=2, post_close_ky=8,
                                     post_open_kx=2, post_open_ky=4), ("stripes", 8.0, 0.0, 0.5)),
    Case("c2_96x203_tilted", 96, 203, _c(seg_band_radius=8, seg_dc_exclusion=6, seg_illum_sigma=8, sat_dilate_ksize=7, post_close_ky=15),
         ("stripes", 11.3, 0.15, 0.5)),
    Case("c3_256x320_defaults", 256, 320, _c(), ("stripes", 9.7, 0.0, 0.5)),
    Case("c4_272x1009_prefix", 272, 1009, _c(), ("stripes", 20.3, 0.0, 0.5)),
    Case("c5_272x1009_kmorph", 272, 1009, _c(seg_illum_sigma=0, sat_dilate_ksize=5, post_close_ky=3, post_open_ky=3), ("stripes", 20.3, -0.1, 0.5)),
    Case("c6_80x3329_one_peak", 80, 3329, _c(seg_band_radius=10, seg_dc_exclusion=12, n_peaks=1, seg_peak_max_dy_from_center=0.0, post_close_kx=1,
                                             post_close_ky=1, post_open_kx=1, post_open_ky=1), ("stripes", 20.3, 0.0, 0.5)),
    Case("c7_80x3329_wide_band", 80, 3329, _c(seg_band_radius=39, n_peaks=64, post_close_ky=33, post_open_ky=33), ("stripes", 20.3, 0.0, 0.5)),
    Case("c8_tie", 96, 203, _c(**_TIE), ("tie",), "A_is_dark"),
    Case("c8_tie_sigma8", 96, 203, _c(**dict(_TIE, seg_illum_sigma=8)), ("tie",), "A_is_dark"),
    Case("c8_tie_dc6_empty_b", 96, 203, _c(**dict(_TIE, seg_dc_exclusion=6)), ("tie",), "A_is_dark"),
    Case("c9_96x203_narrow_bright", 96, 203, _c(seg_band_radius=8, seg_dc_exclusion=6, seg_illum_sigma=8, sat_dilate_ksize=7, post_close_ky=15),
         ("stripes", 11.3, 0.15, 0.3)),
    Case("c9_96x203_narrow_dark", 96, 203, _c(seg_band_radius=8, seg_dc_exclusion=6, seg_illum_sigma=8, sat_dilate_ksize=7, post_close_ky=15),
         ("stripes", 11.3, 0.15, 0.7)),
    Case("c9_272x1009_narrow_bright", 272, 1009, _c(), ("stripes", 20.3, 0.0, 0.3)),
    Case("c9_272x1009_narrow_dark", 272, 1009, _c(), ("stripes", 20.3, 0.0, 0.7)),
]
BY_NAME = {c.name: c for c in CASES}


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """(image, roi, dark, light, pack) of the oracle on a case: computed once, shared, never written to"""
    c = BY_NAME[name]
    img, roi = c.image()
    dark, light, pack = T.segment_dark_light_gratings_periodic_fft(img, roi, c.config(T.TempSegConfig))
    for a in (img, roi, dark, light):
        a.setflags(write=False)
    return img, roi, dark, light, pack


# =======================================================================================================================================
# the stages, each from its own upstream plane

def ref_gray(img):
    return A.bgr2gray_u8(img)


def ref_sat(gray_u8, roi, cfg):
    """(sat0, sat, roi_eff)"""
    sat0 = (gray_u8 >= int(cfg.sat_thresh_gray)) & roi
    sat = T.make_saturation_mask(gray_u8, roi, cfg)
    return sat0, sat, roi & ~sat


def ref_med(gray_u8, roi_eff):
    return np.float32(np.median(gray_u8.astype(np.float32)[roi_eff]))


def ref_g(gray_u8, roi, med):
    g = gray_u8.astype(np.float32)
    g[~roi] = med
    return g


def ref_norm(g, sigma):
    """(blur or None, norm): norm = g / where(blur < 1e-6, 1, blur) in float32; g itself without the Gaussian"""
    if int(sigma) <= 0:
        return None, g
    blur = cv.gaussian_blur(g, float(sigma))
    return blur, (g / np.where(blur < 1e-6, np.float32(1.0), blur)).astype(np.float32)


def ref_inorm_candidates(norm, roi_eff):
    """norm / mu in float32 for mu = float32(float64 mean of norm[roi_eff]) and its two float32 neighbours (the order of the sum decides the last
    bit of mu, and the reference's own float32 pairwise sum is one more order)"""
    mu = np.float32(np.mean(norm[roi_eff].astype(np.float64)))
    if not abs(mu) > 1e-9:
        mu = np.float32(1.0)
    return [(m, (norm / m).astype(np.float32)) for m in (mu, np.nextafter(mu, np.float32(-np.inf)), np.nextafter(mu, np.float32(np.inf)))]


def ref_spectrum(inorm):
    """fftshift(fft2(float64(inorm)))"""
    return np.fft.fftshift(np.fft.fft2(inorm.astype(np.float64)))


def ref_peaks(mag, cfg):
    return O.find_top_peaks(mag, dc_exclusion=int(cfg.seg_dc_exclusion), n_peaks=cfg.n_peaks)


def ref_carrier(peaks, h, w, cfg):
    """(peak_x, peak_y, angle, period) by the oracle's choice and formulas"""
    px, py = T.choose_carrier_peak(peaks, h, w, cfg.seg_peak_max_dy_from_center)
    dx, dy = float(px - w // 2), float(py - h // 2)
    fmag = float(np.hypot(dx / float(w), dy / float(h)))
    return int(px), int(py), float(np.arctan2(dy, dx)), (1.0 / fmag) if fmag > 1e-9 else float("nan")


def band_disc(h, w, peak, R):
    yy, xx = np.ogrid[:h, :w]
    return (xx - peak[0]) ** 2 + (yy - peak[1]) ** 2 <= float(R) ** 2


def ref_bandpass(F_shift, peak, R):
    h, w = F_shift.shape
    return np.fft.ifft2(np.fft.ifftshift(F_shift * band_disc(h, w, peak, R)))


def bound_z(inorm, F_shift, peak, R):
    """the componentwise bound on the device's z against ref_bandpass (module docstring)"""
    h, w = inorm.shape
    pm = 2 * R + 1
    disc = band_disc(h, w, peak, R)
    nb = int(disc.sum())
    S = float(np.abs(inorm.astype(np.float64)).sum())
    SP = float((np.abs(F_shift.real) + np.abs(F_shift.imag))[disc].sum())
    lg = 8.0 * np.log2(h * w)
    patch_err = (2 * (2 * h + 3) + 2 * (w + 3) + 16 + lg) * U * S
    return (2 * nb * patch_err + (4 * (2 * pm + 3) + 2 * 2 * np.pi * 4 * 5 * 2 + lg) * U * SP) / (h * w)


def ref_phi0(z, inorm, roi_eff):
    """(phi0, c, sum |z m|) of c = sum over roi_eff of z (inorm - 1)"""
    m = (inorm - 1.0).astype(np.float32)
    t = z[roi_eff] * m[roi_eff]
    c = np.sum(t)
    return (float(np.angle(c)) if np.isfinite(c) else 0.0), complex(c), float(np.abs(t).sum())


def ref_signal(z, phi0):
    """Re(z e^{-i phi0}) in float64; the sign mask is float32(.) >= 0 inside roi_eff"""
    return np.real(z * np.exp(-1j * phi0))


def ref_mask_a(z, phi0, roi_eff):
    return (ref_signal(z, phi0).astype(np.float32) >= 0) & roi_eff


def ref_sides(gray_u8, mask_a, roi_eff):
    """((sum, count) of A, (sum, count) of B, mean_a, mean_b, a_is_dark): integer sums, float64 quotients, 1e9 for an empty side"""
    b = roi_eff & ~mask_a
    sa, na, sb, nb = int(gray_u8[mask_a].sum(dtype=np.int64)), int(mask_a.sum()), int(gray_u8[b].sum(dtype=np.int64)), int(b.sum())
    mean_a, mean_b = (sa / na if na else 1e9), (sb / nb if nb else 1e9)
    return (sa, na), (sb, nb), mean_a, mean_b, mean_a <= mean_b


def ref_final(mask_a, a_is_dark, roi_eff, cfg):
    """(raw_dark, dark, light)"""
    raw = mask_a if a_is_dark else roi_eff & ~mask_a
    dark = T.postprocess_mask(raw, roi_eff, cfg) & roi_eff
    return raw, dark, roi_eff & ~dark
