/* Test-only entry points of libvistaf_ftp.so for the back end of a predict: everything post_demod (api.hip) runs after the core medians -- the
 * reliable-only smoothing, the sign flip, the hole stage's glue, the frontier taper / composition / mm curve, the blob filter, the force tail and
 * the copy to the caller's planes (k_post.hip, k_holes.hip, k_blurchain.hip, k_backend.hip).  NOT part of the drop-in boundary
 * (include/vistaf_ftp.h), like everything in test_hooks.h.  Their ctypes signatures are `_lib.POST_SIGNATURES`; tests/test_post_direct.py holds
 * that table against these prototypes and runs the hooks against the NumPy references of tests/post_cases.py.
 *
 * Conventions (those of test_hooks.h): planes are device planes of the caller, [B, h, w] or [B, P] unless a parameter says otherwise; every call
 * runs on `stream`, waits for it, and returns the tier it launched (>= 0) or a negative VISTAF_E_* code (text in vistaf_ftp_last_error).  A NULL
 * plane (the ones marked optional apart), a size below 1, an unknown variant and a variant the shape or blur does not take are refused with
 * VISTAF_E_INVALID before anything is allocated or launched.  Scratch planes are allocated and freed by the call.  Blurs take the taps a
 * session builds for their sigma (gauss_taps of host_util.hpp) and the session's default blur tiers.  The hooks are in api_hooks.hip; the three
 * with tiers of their own (_smooth_reliable, _height_finish, _backend) call the functions post_demod calls (smooth_stage, height_finish_stage,
 * backend_stage of stages.hpp), variant 0 with the default of the tier's flag, and may allocate the scratch of the separate kernels whichever
 * tier runs. */
#ifndef VISTAF_TEST_HOOKS_POST_H
#define VISTAF_TEST_HOOKS_POST_H
#include "../../include/vistaf_ftp.h"
#ifdef __cplusplus
extern "C" {
#endif
/* hmap = masked smoothing of (detr - bg_med[b]) over reliable & finite, sigma > 0:
 *   variant 1  launch_sub_scalar_mask, two launch_gauss_blur, launch_div_planes (returns 1),
 *   variant 2  launch_smooth_reliable, the tile-fused kernel (returns 2); refused when sigma gives more than GF_MAXK = 15 taps,
 *   variant 0  what a session with default tiers runs: 2 up to 15 taps, else 1.
 * sigma == 0: launch_zeroed_keep_nan, hmap = detr - bg_med[b] on reliable and the quiet NaN off it (returns 3; variants 0 and 1 only).
 * bg_med: [B].  Refused: a negative or non-finite sigma, one beyond 511 taps. */
int vistaf_ftp_test_smooth_reliable(const float *detr, const float *bg_med, const uint8_t *reliable, double sigma, float *hmap, int B, int h, int w,
                                    int variant, void *stream);

/* launch_core_flip: frames whose core_med[b] is finite and > 0 are multiplied by -1 in place; flipped[b] = 1 for those, else 0.  Returns 0. */
int vistaf_ftp_test_core_flip(float *hmap_inout, const float *core_med, int32_t *flipped, int B, int P, void *stream);

/* launch_hole_candidates: cand = reliable & !finite(hmap) & known / (container + 1e-6) >= frac_thr & dist >= min_dist, the two counts over the
 * ksize x ksize window (BORDER_REFLECT_101, folded as often as the window needs; ksize odd, 3..511) and the quotient in float32.  Returns 0. */
int vistaf_ftp_test_hole_candidates(const float *hmap, const uint8_t *reliable, const float *dist, int ksize, float frac_thr, float min_dist, uint8_t *cand,
                                    int B, int h, int w, void *stream);

/* The glue of the hole stage, one launcher each; med and fill are [B] arrays of the caller (the medians a session selects).  Each returns 0.
 * _hole_tmp:   tmp = hmap where finite, else med[b] (0 when that is not finite), on reliable & !cand; the quiet NaN elsewhere.
 * _hole_zin:   tmp_zin = itself where finite, else fill[b] (0 when that is not finite).
 * _hole_merge: hmap = zin on cand, itself elsewhere, the quiet NaN off reliable; out_rel = reliable & finite(hmap). */
int vistaf_ftp_test_hole_tmp(const float *hmap, const uint8_t *reliable, const uint8_t *cand, const float *med, float *tmp, int B, int P, void *stream);
int vistaf_ftp_test_hole_zin(float *tmp_zin, const float *fill, int B, int P, void *stream);
int vistaf_ftp_test_hole_merge(float *hmap_inout, const uint8_t *reliable, const uint8_t *cand, const float *zin, uint8_t *out_rel, int B, int P,
                               void *stream);

/* Frontier taper, composition, unreliable-region smoothing, clamp and the mm curve, as post_demod calls them: the taper band is `band` with
 * use_band, else 1 (a session then passes a plane of huge distances, bytes 0x7f, as dist_in and dist_out is not read).
 *   variant 1  launch_frontier_compose, launch_gauss_blur (sigma_unrel > 0), launch_finalize_unitless, launch_to_mm (returns 1),
 *   variant 2  launch_compose_finalize_mm (returns 2); refused unless sigma_unrel gives 1..15 taps,
 *   variant 0  what a session with default tiers runs.
 * roi, roi_den: one [h, w] plane for the batch (roi_den = blur(roi) + 1e-6 in a session; read on unreliable ROI pixels only).  gmax: [B] float32,
 * the largest candidate depth's bits, 0 without a candidate.  curve: type 0..5 of Curve (common.hpp) with a, b, c.
 * Refused: use_band other than 0 / 1, use_band with band <= 0, a curve type outside 0..5, a negative or non-finite sigma_unrel. */
int vistaf_ftp_test_height_finish(const float *hmap, const uint8_t *reliable, const uint8_t *roi, const float *dist_in, const float *dist_out,
                                  const float *roi_den, float band, int use_band, double sigma_unrel, int curve_type, double curve_a, double curve_b,
                                  double curve_c, int use_neg, float *unitless, float *depth, uint8_t *cand, float *gmax, int B, int h, int w, int variant,
                                  void *stream);

/* launch_to_mm alone, on a unitless plane of the caller's: depth = float32(curve(max(use_neg ? -u : u, 0))) (NaN stays NaN), cand = roi & finite(depth) &
 * depth > 0, gmax[b] = the largest candidate depth's bits (0 without one).  roi: one [P] plane.  This is the only way to hand the mm curve finite
 * values off the ROI: the composition above writes NaN there in both variants, so k_compose_finalize_mm cannot be fed such a plane.  Returns 0. */
int vistaf_ftp_test_to_mm(const float *unitless, const uint8_t *roi, int curve_type, double curve_a, double curve_b, double curve_c, int use_neg, float *depth,
                          uint8_t *cand, float *gmax, int B, int P, void *stream);

/* launch_tail: scalars[b * nscal + 0..8] = volume_cm3, area_mm2, max depth, force, arg-max of height over roi_static & finite (-1: none), period_px,
 * mm_per_px, the minimum of unitless over roi_static & finite (NaN: none, or no unitless plane) and its index (-1); out3[b * 3 + 0..2] = the first
 * three.  The rest of a scalar record is not touched.
 *   variant 1  k_tail, one workgroup per frame (returns 1),
 *   variant 2  k_tail_part + k_tail_final at any P (returns 2),
 *   variant 0  launch_tail's own dispatch with the chain scratch a session of frames of this size holds.
 * Optional: roi_frame ([B, P]; NULL: isfinite(height)), unitless ([B, P]), scalars, out3 (not both NULL); roi_static ([P]) may be NULL without
 * scalars.  Refused: nscal < 9 with scalars, a force curve type outside 0..5. */
int vistaf_ftp_test_tail(const float *height, const uint8_t *roi_frame, const float *unitless, const uint8_t *roi_static, double mm_per_px,
                         double depth_eps_mm, double period_px, int force_type, double force_a, double force_b, double force_c, double *scalars, int nscal,
                         double *out3, int B, int P, int variant, void *stream);

/* The back end from the candidates on: labels, blob filter (depth_inout zeroed at the candidates not kept), force tail and arg-extrema, copy to
 * out_h / out_r (the quiet NaN / 0 for frames of status 1 or 3).
 *   variant 1  launch_cc_label, launch_blob_filter, launch_tail (with the chain scratch a session of this frame size holds), launch_copy_out
 *              (returns 1),
 *   variant 2  launch_backend_fused (returns 2); refused where backend_fused_fits(h, w) is false,
 *   variant 0  what a session with default tiers runs.
 * gmax: [B] float32 as vistaf_ftp_test_height_finish leaves it; roi_static: [h, w]; status: [B].  labels [B, P] int32, peak_bits [B, P] uint32
 * (valid at component roots only: the fused kernel writes no other entry).  Optional: unitless, kept, out_h, out_r.  nscal >= 9. */
int vistaf_ftp_test_backend(float *depth_inout, const uint8_t *cand, const float *gmax, const float *unitless, const uint8_t *roi_static,
                            const uint8_t *reliable, const int32_t *status, double min_peak_mm, double rel_frac, double mm_per_px, double depth_eps_mm,
                            double period_px, int force_type, double force_a, double force_b, double force_c, int32_t *labels, uint32_t *peak_bits,
                            uint8_t *kept, double *scalars, int nscal, float *out_h, uint8_t *out_r, int B, int h, int w, int variant, void *stream);

/* backend_fused_fits(h, w): 1 / 0.  Launches nothing. */
int vistaf_ftp_test_backend_fits(int h, int w);

/* launch_fill_scalars (scalars[b * nscal + 9..15] = rel_count, flipped, amp_thr, contact_thr, bg_med, bad_count, 0; a NULL source gives 0) and
 * launch_mark_empty (status[b] = 1 where rel_count[b] == 0 and status[b] was 0).  rel_count is required, status and scalars (nscal >= 16) optional but
 * not both NULL.  Returns 0. */
int vistaf_ftp_test_frame_records(const int *rel_count, const int *flipped, const float *amp_thr, const float *contact_thr, const float *bg_med,
                                  const int *bad_count, double *scalars, int nscal, int32_t *status, int B, void *stream);
#ifdef __cplusplus
}
#endif
#endif
