/* vistaf_tempsensor.h -- C ABI of the temperature modality end to end, part of libvistaf_ftp.so.
 *
 * Replaces, on the MI355X, the orchestration of the reference's temperature module and the statistics its summary reports:
 *
 *   vistaf_tsensor_predict          Code/temperature_sensor.py:749-870 `main()`: BGR photograph -> final temperature map, its source map and
 *                                   its statistics, every intermediate plane on the device
 *   vistaf_tsensor_map_statistics   Code/multimodal_sensor.py:558-567: mean / median / std / min / max / count of the final map over its
 *                                   valid pixels (sensor_readings.temperature of multimodal_summary.json), equal to NumPy's to the last bit
 *
 * THE CHAIN (full frame, one stream; every stage is the library's existing public one, include/vistaf_temp.h and vistaf_tempmodel.h):
 *   1. vistaf_tempseg_segment(bgr, roi_full) -> dark, light, roi_eff, sat and the segmentation record (carrier angle included)
 *   2. vistaf_temp_feature_planes(bgr, blur_ksize)                            L, a, b, gray
 *   3. vistaf_temp_color_support(a, b, light, roi_eff, sat, chroma_min, dilate) color_support
 *   4. vistaf_tmodel_predict_maps: wide_raw = wide model over roi_eff, color_raw = colour model over color_support (one pass)
 *   5. wide  = clamp(inpaint(wide_raw, roi_full, wide_inpaint_radius), roi_full, final_t_min, final_t_max)
 *   6. color = clamp(inpaint(color_raw, color_support, color_inpaint_radius), color_support, color_t_min - pad, color_t_max + pad)
 *   7. fused, source, counts = fuse_maps_per_pixel(roi_full, wide, color)
 *   8. final = oriented_gaussian_blur_float(fused, roi_full, carrier_angle_rad, sigma_across, sigma_along)
 *   9. statistics(final, isfinite(final))
 * Where the order, masks and constants come from: the map-stage order and clamp ranges are those recorded for main() :835-855, segmentation
 * and feature planes run on the full frame (the bbox crop of :770 only feeds the saved artefacts).  ONE STEP IS INFERRED: the wide model's
 * mask is roi_eff -- the black model was trained with exclude_saturated_pixels (tests/golden/ref_temp_black_metrics.json) and the inpaint
 * over roi_full in step 5 then fills exactly the saturated pixels.  PARITY UNPINNED as the map stages are: the reference tree holds no
 * temperature map; only the segmentation masks and the number of valid pixels of the stored summary pin the chain.
 *
 * Every function returns 0 or a negative VISTAF_E_* code (vistaf_ftp.h); vistaf_ftp_last_error() holds the message.  Device pointers are
 * HIP device pointers on the device current at create time, `stream` a hipStream_t passed as void*.
 */
#ifndef VISTAF_TEMPSENSOR_H
#define VISTAF_TEMPSENSOR_H

#include <stdint.h>

#include "vistaf_temp.h"
#include "vistaf_tempmodel.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vistaf_tsensor vistaf_tsensor;
typedef struct vistaf_tstats vistaf_tstats;

typedef struct vistaf_tsensor_config {     /* Code/temperature_sensor.py, defaults as shipped */
    vistaf_tempseg_config seg;              /* :67-82 */
    vistaf_temp_fuse_config fuse;           /* :55-64; final_t_min / final_t_max also clamp the wide map (step 5) */
    int32_t blur_ksize;                     /* :52 5 (5 or <= 1) */
    int32_t color_support_dilate;           /* :87 3 */
    int32_t wide_inpaint_radius;            /* 7 (step 5) */
    int32_t color_inpaint_radius;           /* 5 (step 6) */
    double color_chroma_min;                /* :86 10 */
    double color_clamp_pad;                 /* 5: the colour map is clamped to [color_t_min - pad, color_t_max + pad] */
    double smooth_sigma_across;             /* :95 6 */
    double smooth_sigma_along;              /* :96 1 */
} vistaf_tsensor_config;

/* info_host of vistaf_tsensor_predict: the segmentation record (VISTAF_TS_* of vistaf_temp.h) then the four fusion counts */
#define VISTAF_TSENSOR_NINFO (VISTAF_TEMPSEG_NINFO + 4)
#define VISTAF_TSENSOR_ROI_PIXELS (VISTAF_TEMPSEG_NINFO + 0)
#define VISTAF_TSENSOR_WIDE_OK_PIXELS (VISTAF_TEMPSEG_NINFO + 1)
#define VISTAF_TSENSOR_COLOR_OK_PIXELS (VISTAF_TEMPSEG_NINFO + 2)
#define VISTAF_TSENSOR_BLEND_PIXELS (VISTAF_TEMPSEG_NINFO + 3)
/* planes of d_masks, uint8 0/1 [5, H, W] */
#define VISTAF_TSENSOR_MASK_ROI_EFF 0
#define VISTAF_TSENSOR_MASK_SAT 1
#define VISTAF_TSENSOR_MASK_DARK 2
#define VISTAF_TSENSOR_MASK_LIGHT 3
#define VISTAF_TSENSOR_MASK_COLOR_SUPPORT 4
#define VISTAF_TSENSOR_NMASKS 5
/* d_stats / stats_host: mean_C, median_C, std_C, min_C, max_C, valid_pixels (the key order of writers.temperature_statistics) */
#define VISTAF_TSENSOR_NSTATS 6

int vistaf_tsensor_default_config(vistaf_tsensor_config *cfg);

/* One session for H x W photographs.  Both models are required (the library keeps the pointers: they must outlive the session).  The frame
 * must suit the segmentation: H a multiple of 16, both sides >= 64, else VISTAF_E_INVALID.  Every buffer and workspace of the chain and of the
 * statistics is allocated here, and the smoothing taps are uploaded (the sigmas are fixed per session).  Synchronous. */
int vistaf_tsensor_create(const vistaf_tsensor_config *cfg, int H, int W, const vistaf_tmodel *wide_model, const vistaf_tmodel *color_model,
                          vistaf_tsensor **out);
void vistaf_tsensor_destroy(vistaf_tsensor *h);

/* d_bgr [H, W, 3] uint8 (cv2.imread order), d_roi [H, W] uint8 0/1 (roi_full), d_final float32 [H, W] (required).  Optional (NULL: not
 * written): d_source uint8 [H, W] (0 wide, 255 colour, 128 blend), d_wide / d_color float32 [H, W] (the clamped maps of steps 5 and 6),
 * d_masks uint8 [5, H, W] (VISTAF_TSENSOR_MASK_*), info_host double[VISTAF_TSENSOR_NINFO] (host), d_stats double[6] (device), stats_host
 * double[6] (host).  Errors of the segmentation as vistaf_tempseg_segment.  SYNCHRONISES `stream`: the segmentation's own synchronisations
 * (carrier search, phase), the fusion counts when info_host is given, the host copy of the statistics when stats_host is given; the other
 * steps are asynchronous. */
int vistaf_tsensor_predict(vistaf_tsensor *h, const uint8_t *d_bgr, const uint8_t *d_roi, float *d_final, uint8_t *d_source, float *d_wide,
                           float *d_color, uint8_t *d_masks, double *info_host, double *d_stats, double *stats_host, void *stream);

/* Statistics workspace for H x W maps, any H, W >= 1 (allocated here, synchronous). */
int vistaf_tsensor_stats_create(int H, int W, vistaf_tstats **out);
void vistaf_tsensor_stats_destroy(vistaf_tstats *s);

/* writers.temperature_statistics(map, valid) of a float32 [H, W] map over a uint8 [H, W] mask (nonzero = valid), or over isfinite(map)
 * when d_valid is NULL: the float32 results of np.mean / np.median / np.std / np.min / np.max of map[valid] widened to double, and the
 * count; NaN statistics and count 0 when no pixel is valid; NaN ones (count unchanged) when a valid pixel is NaN.  Equal to NumPy 2.x to the
 * last bit (pairwise summation tree of np.add.reduce, np.var's two passes, exact order statistics), with two stated exceptions: with an
 * explicit mask holding +-inf the median is taken over the finite values only, and a zero min / max may carry either sign when +0 and -0
 * tie.  At least one of d_stats (device, double[6]) and stats_host (host, double[6]) is required.  Asynchronous on `stream` unless
 * stats_host is given (then it synchronises); no allocation. */
int vistaf_tsensor_map_statistics(vistaf_tstats *s, const float *d_map, const uint8_t *d_valid, double *d_stats, double *stats_host, void *stream);

#ifdef __cplusplus
}
#endif
#endif
