/* vistaf_temp.h -- C ABI of the first two slices of the temperature modality, part of libvistaf_ftp.so.
 *
 * Replaces, on the MI355X, the periodic-stripe segmentation of the reference's temperature module -- the step that splits the
 * thermochromic grating of a full photograph into its dark and its light stripes before any regression runs:
 *
 *   vistaf_tempseg_segment     Code/temperature_sensor.py:437-540 `segment_dark_light_gratings_periodic_fft(image_bgr, roi_full)`
 *                              with its helpers _make_saturation_mask (:378-387), _illum_normalize (:363-375), _find_top_peaks (:316-337),
 *                              _choose_carrier_peak (:339-360) and _postprocess_mask (:390-406)
 *
 * The temperature regressors themselves (TempModel.predict, :236) are in include/vistaf_tempmodel.h, evaluated from exported parameters.
 * All image pointers are HIP device pointers; `stream` is a hipStream_t passed as void*.  Every function returns 0
 * or a negative VISTAF_E_* code (vistaf_ftp.h); vistaf_ftp_last_error() holds the message.  The full-frame spectrum of the carrier search
 * is a plain library transform (hipFFT, float32: only the POSITION of the strongest peaks is read from it); the band-pass around the chosen
 * carrier is the library's own pruned float64 DFT on the matrix cores, everything else hand-written HIP.
 * Known numerical differences from upstream, both without effect on the five stored demo photographs (0 differing mask pixels): the peak
 * search ranks float32 magnitudes where upstream ranks float64 ones (two peaks within float32 rounding of each other could swap), and the
 * mean of the normalised image is a float64 sum rounded once where np.mean accumulates pairwise in float32 (a stripe-edge pixel whose
 * band-passed value is within an ulp of 0 could flip).  Pixel-for-pixel parity is pinned on those photographs only.
 */
#ifndef VISTAF_TEMP_H
#define VISTAF_TEMP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vistaf_tempseg_handle vistaf_tempseg_handle;

typedef struct vistaf_tempseg_config {   /* Code/temperature_sensor.py:67-82, defaults as shipped */
    int32_t seg_band_radius;             /* :67 22  */
    int32_t seg_dc_exclusion;            /* :68 28  */
    int32_t seg_illum_sigma;             /* :72 20 (0 disables the Gaussian illumination normalisation) */
    int32_t sat_thresh_gray;             /* :75 245 */
    int32_t sat_dilate_ksize;            /* :76 13  */
    int32_t post_close_kx, post_close_ky;/* :79-80 3, 31 */
    int32_t post_open_kx, post_open_ky;  /* :81-82 3, 7 */
    int32_t n_peaks;                     /* :457 16 */
    double seg_peak_max_dy_from_center;  /* :71 0.14 */
} vistaf_tempseg_config;

/* record returned by vistaf_tempseg_segment (the `dbg` dict of :513-527), doubles */
#define VISTAF_TEMPSEG_NINFO 16
#define VISTAF_TS_PEAK_X 0
#define VISTAF_TS_PEAK_Y 1
#define VISTAF_TS_PHI0_RAD 2
#define VISTAF_TS_MEAN_GRAY_A 3
#define VISTAF_TS_MEAN_GRAY_B 4
#define VISTAF_TS_A_IS_DARK 5
#define VISTAF_TS_ROI_PIXELS 6
#define VISTAF_TS_ROI_EFF_PIXELS 7
#define VISTAF_TS_SAT_PIXELS 8
#define VISTAF_TS_DARK_PIXELS 9
#define VISTAF_TS_LIGHT_PIXELS 10
#define VISTAF_TS_CARRIER_ANGLE_RAD 11
#define VISTAF_TS_CARRIER_PERIOD_PX 12

int vistaf_tempseg_default_config(vistaf_tempseg_config *cfg);
/* Any frame size H, W >= 1.  The session allocates the segmentation's workspace (hipFFT plan, band-pass tables and planes) on its first
 * vistaf_tempseg_segment call; a session used for the feature planes, the colour support or the map stages only never allocates it. */
int vistaf_tempseg_create(const vistaf_tempseg_config *cfg, int H, int W, vistaf_tempseg_handle **out);
void vistaf_tempseg_destroy(vistaf_tempseg_handle *h);

/* d_bgr [H,W,3] uint8 (cv2.imread order), d_roi [H,W] uint8 0/1 (roi_full).  Outputs [H,W] uint8 0/1, any may be NULL:
 * d_dark / d_light (dark_final, light_final), d_roi_eff, d_sat; info_host[VISTAF_TEMPSEG_NINFO] on the HOST.
 * Errors as upstream: VISTAF_E_STATE when the ROI is empty after the saturation exclusion (:445-446).  Synchronises `stream`.
 * SIZE LIMIT of this function only: H must be a multiple of 16 (the band-pass DFT runs in 16-row matrix-core strips) and both sides >= 64;
 * other sizes return VISTAF_E_INVALID ("segment: frame height must be a multiple of 16 ...").  The functions below have no such limit. */
/* DELIBERATE RESTRICTION: returns VISTAF_E_NOCARRIER ("carrier band leaves the spectrum") when the band-pass disc of radius
 * bandpass_radius_bins around the carrier peak is clipped by the spectrum border; upstream multiplies by the clipped disc and goes on
 * (temperature_sensor.py:463-468).  Such a carrier is within 22 bins of Nyquist (stripe period ~2 px); parity for that edge is unpinned. */
int vistaf_tempseg_segment(vistaf_tempseg_handle *h, const uint8_t *d_bgr, const uint8_t *d_roi, uint8_t *d_dark, uint8_t *d_light,
                           uint8_t *d_roi_eff, uint8_t *d_sat, double *info_host, void *stream);

/* Second slice: the feature planes and the colour-support test the temperature models are evaluated on.
 *
 *   vistaf_temp_feature_planes   Code/temperature_sensor.py:278-293 `compute_feature_planes(image_bgr, blur_ksize)`:
 *                                cv2.GaussianBlur(img, (5, 5), 0) on uint8 (fixed point, one rounding), cv2.cvtColor BGR2LAB on uint8 (integer
 *                                table path) and BGR2GRAY, returned as the float32 planes "L", "a", "b", "gray" ([H,W], any may be NULL).
 *                                blur_ksize: 5 (BLUR_KSIZE as shipped, :52) or <= 1 (no smoothing); other sizes are VISTAF_E_INVALID.
 *   vistaf_temp_color_support    main() :793-799: chroma = sqrt((a - 128)^2 + (b - 128)^2) in float32 and
 *                                color_support = dilate_bool_mask(light, dilate_ksize) & roi_eff & ~sat & (chroma >= chroma_min)
 *                                (dilate_bool_mask :583-590, MORPH_ELLIPSE; defaults COLOR_CHROMA_MIN 10.0 :86, COLOR_SUPPORT_DILATE 3 :87;
 *                                the threshold is compared in float32 like NumPy does for a Python scalar).  d_chroma / d_support may be NULL;
 *                                the masks are only needed for d_support.
 * Both are asynchronous on `stream`; the handle's frame size applies, any H, W >= 1 (tiled per-pixel kernels with clamped borders and the
 * bit-plane / row-span morphology: neither needs the segmentation's size limit). */
int vistaf_temp_feature_planes(vistaf_tempseg_handle *h, const uint8_t *d_bgr, int blur_ksize, float *d_L, float *d_a, float *d_b, float *d_gray,
                               void *stream);
int vistaf_temp_color_support(vistaf_tempseg_handle *h, const float *d_a, const float *d_b, const uint8_t *d_light, const uint8_t *d_roi_eff,
                              const uint8_t *d_sat, double chroma_min, int dilate_ksize, float *d_chroma, uint8_t *d_support, void *stream);

/* Third slice (round 3): the map-domain stages behind the regressors.  PARITY UNPINNED -- the reference tree holds no output of these stages
 * (temperature_map_*.npy were not mounted) and the regressors that feed them only exist as pickles; checked against the restatement of the
 * source text in oracle/temp_oracle.py on synthetic planes.  Maps are float32 [H,W] with NaN = no value, masks uint8 0/1.
 *
 *   vistaf_temp_clamp_map       :538-543 `clamp_map(m, roi, lo, hi)`
 *   vistaf_temp_inpaint_map     :546-580 `inpaint_temperature_map(temp_map, roi_mask, radius)`: 8-bit rescaling over the range of the known
 *                               values, cv2.inpaint(INPAINT_TELEA) of the missing ROI pixels with OpenCV's 8-bit rounding of every estimate,
 *                               EVERY ROI pixel read back from the 8-bit image; the two early returns (nothing missing / known; flat map) included
 *   vistaf_temp_fuse_maps       :594-636 `fuse_maps_per_pixel(roi, wide_map, color_map)`: d_source 0 = wide, 255 = colour, 128 = blend (may be NULL);
 *                               counts_host[4] = roi, wide_ok, color_ok, blend pixels (may be NULL; non-NULL synchronises `stream`)
 *   vistaf_temp_oriented_blur   :705-747 `oriented_gaussian_blur_float(map, roi, angle_rad, sigma_across, sigma_along)`: warpAffine (INTER_LINEAR,
 *                               BORDER_REFLECT; the ROI with INTER_NEAREST) by getRotationMatrix2D, anisotropic GaussianBlur, rotate back.
 *                               Uploads the two tap vectors (synchronises `stream`).
 * All four are per-pixel kernels (and the whole-frame Telea march) with no frame-size limit: any H, W >= 1. */
typedef struct vistaf_temp_fuse_config {     /* Code/temperature_sensor.py:55-64, defaults as shipped */
    double color_t_min, color_t_max;         /* 20, 33 */
    double color_guard_band, switch_margin_c;/* 0.5, 1.0 */
    double final_t_min, final_t_max;         /* 20, 75 */
} vistaf_temp_fuse_config;
int vistaf_temp_clamp_map(vistaf_tempseg_handle *h, const float *d_map, const uint8_t *d_roi, double lo, double hi, float *d_out, void *stream);
int vistaf_temp_inpaint_map(vistaf_tempseg_handle *h, const float *d_map, const uint8_t *d_roi, int radius, float *d_out, void *stream);
int vistaf_temp_fuse_maps(vistaf_tempseg_handle *h, const uint8_t *d_roi, const float *d_wide, const float *d_color, const vistaf_temp_fuse_config *cfg,
                          float *d_final, uint8_t *d_source, int64_t *counts_host, void *stream);
int vistaf_temp_oriented_blur(vistaf_tempseg_handle *h, const float *d_map, const uint8_t *d_roi, double angle_rad, double sigma_across, double sigma_along,
                              float *d_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
