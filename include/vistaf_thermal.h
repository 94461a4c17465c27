/* vistaf_thermal.h -- C ABI of the thermal read-out, part of libvistaf_ftp.so.
 *
 * An extension with no counterpart in the reference: the force chain ends in a depth map and the tables read out of it (contacts, tracks,
 * shapes, taxels), all in the ALIGNED ROI CROP -- after the global shift, the crop and the inverse ECC warp of vistaf_align.h; the temperature
 * chain (vistaf_tempsensor.h) ends in a temperature map in the PHOTOGRAPH'S FRAME.  This brings the second into the frame of the first with
 * the record the aligner wrote, and reduces it over the rows of the contacts table: how warm the thing touching the skin is, how warm the
 * skin around it, the contrast of the two.  It is an object of its own: it touches no other handle and reads only what it is handed.
 * The temperature chain itself is parity-unpinned (no stored reference output pins its maps); the read-out inherits that and adds nothing
 * to it: it is an exact, documented function of the map it is given.
 *
 * THE DEFINITION.  All arithmetic is float64 unless said otherwise, evaluated left to right, no fused multiply-add anywhere.
 *
 * REGISTRATION, frame b, crop pixel (x, y), photograph H x W, crop origin (crop_x1, crop_y1) in the photograph (vistaf_align_geometry):
 *   0. info = row b of d_align_info.  (sx, sy) = (info[VISTAF_AI_SHIFT_X], info[VISTAF_AI_SHIFT_Y]) when apply_global_shift is set, else
 *      (0, 0) and the two entries are not read into the formula; M = the 2 x 3 matrix info[VISTAF_AI_WARP ..], row-major.  A NULL
 *      d_align_info means (sx, sy) = (0, 0) and M = identity.
 *   1. u = ((M00*x + M01*y) + M02) + crop_x1 - sx
 *      v = ((M10*x + M11*y) + M12) + crop_y1 - sy
 *      This is the composition the aligner applies to the photograph, in order: warpAffine by [[1,0,sx],[0,1,sy]] without the inverse flag
 *      (destination (X, Y) reads source (X - sx, Y - sy)), the crop at (crop_x1, crop_y1), warpAffine(WARP_INVERSE_MAP) by the ECC warp
 *      (destination (x, y) reads source M (x, y, 1)).
 *   2. The sample is NaN unless u and v are finite, 0 <= u <= W-1 and 0 <= v <= H-1.  There is no border reflection: a crop pixel whose
 *      source lies outside the photograph has no temperature.  Otherwise
 *        x0 = min(floor(u), W-2), fx = u - x0,  y0 = min(floor(v), H-2), fy = v - y0,
 *        t  = (1-fy)*((1-fx)*T00 + fx*T01) + fy*((1-fx)*T10 + fx*T11),   Tij = map[y0+i][x0+j] widened to float64,
 *      and NaN if any of the four map values is not finite (also one of weight 0).  t is stored once, as float32.  Non-finite info
 *      entries make u or v non-finite for every pixel: the frame is all NaN by the formula alone.
 *
 * CONTACT ROW, frame b, row k of a table of K = max_contacts rows; eps = depth_eps_mm, m = surround_margin_px, t = the registered plane:
 *   0. kk = min(max(count[b], 0), K).  A row k >= kk is all NaN.  When d_status is given and status[b] != 0, every row of the frame and
 *      its frame row are NaN and nothing of the frame is interpreted.  A NaN depth counts as 0.
 *   1. The table's box (BBOX_X0..Y1) is read as in vistaf_shape.h: values that are not finite, beyond +-1e9 or inverted (x1 < x0, y1 < y0)
 *      give a box without pixels, and then a grown box without pixels.  The BOX is the table's clipped to the frame; the GROWN BOX is the
 *      table's enlarged by m on every side, then clipped to the frame.
 *   2. The CONTACT PIXELS of k are the pixels of the box with index == k and depth > float32(eps) (vistaf_shape.h step 1); n = their number.
 *      The VALID PIXELS are those whose t is finite; nv = their number; d = their depth, widened.
 *   3. The SURROUND PIXELS of k are the pixels of the grown box whose index-plane value is outside 0..kk-1 -- the skin that belongs to no
 *      contact, so a touching neighbour is excluded -- and whose t is finite; ns = their number.
 *   4. The row, VISTAF_NTHERMAL doubles:
 *        CONTACT_PIXELS    n
 *        VALID_PIXELS      nv
 *        COVERAGE          nv/n; NaN when n == 0
 *        MEAN_C            (sum t)/nv; NaN when nv == 0
 *        WEIGHTED_MEAN_C   (sum d*t)/(sum d) over the valid pixels (d and t are float32: each product is exact): where the contact presses
 *                          hardest the thermal coupling is best; NaN when nv == 0
 *        MIN_C, MAX_C      over the valid pixels, a selection (the stored float32, widened; -0 orders below +0); NaN when nv == 0
 *        STD_C             sqrt((sum (t - MEAN_C)*(t - MEAN_C))/nv), a second sweep with the finished mean; NaN when nv == 0
 *        PEAK_TEMP_C       t at the table's ARGMAX_INDEX pixel (row-major y*w + x); NaN when that index is not finite or outside
 *                          0..h*w-1, or t there is not finite
 *        SURROUND_PIXELS   ns
 *        SURROUND_MEAN_C   (sum t)/ns over the surround pixels; NaN when ns == 0
 *        CONTRAST_C        MEAN_C - SURROUND_MEAN_C: positive when the object is warmer than the skin around it
 *        12..15            reserved, NaN
 *
 * FRAME ROW, VISTAF_NTHERMALFRAME doubles, over the whole frame (no box):
 *        REGISTERED_PIXELS number of pixels with finite t
 *        SKIN_MEAN_C       mean of t over the finite pixels with index outside 0..kk-1; NaN when there is none
 *        CONTACT_PIXELS    number of finite pixels with index in 0..kk-1 and depth > float32(eps)
 *        CONTACT_MEAN_C    mean of t over those; NaN when there is none
 *        CONTRAST_C        CONTACT_MEAN_C - SKIN_MEAN_C
 *        HOTTEST_CONTACT   the row k < kk with the largest MEAN_C, ties to the lowest k; NaN when no row has a MEAN_C
 *        COLDEST_CONTACT   likewise for the smallest MEAN_C
 *        7                 reserved, NaN
 *
 * Every float64 sum is formed in an order fixed by the box (or the frame) and the launch geometry alone (pixel -> lane -> wave ->
 * workgroup), without float atomics: two calls on the same inputs give the same bits, whatever the batch a frame is part of.
 *
 * What is NOT measured: no emissivity, contact conductance or time constant enters -- the numbers are statistics of the map, not the
 * temperature of the object; no temperature per taxel and none over time (the registered plane is the input both would need).
 *
 * Every function returns 0 or a negative VISTAF_E_* code (vistaf_ftp.h); vistaf_ftp_last_error() holds the message.
 */
#ifndef VISTAF_THERMAL_H
#define VISTAF_THERMAL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* per-contact record written by vistaf_thermal_measure: d_thermal[(b*max_contacts + k)*VISTAF_NTHERMAL + i] (double), row k = row k of frame
 * b's contacts table.  Unused rows and fields are NaN, as in the contacts table. */
#define VISTAF_NTHERMAL 16
#define VISTAF_THERMAL_CONTACT_PIXELS 0
#define VISTAF_THERMAL_VALID_PIXELS 1
#define VISTAF_THERMAL_COVERAGE 2
#define VISTAF_THERMAL_MEAN_C 3
#define VISTAF_THERMAL_WEIGHTED_MEAN_C 4
#define VISTAF_THERMAL_MIN_C 5
#define VISTAF_THERMAL_MAX_C 6
#define VISTAF_THERMAL_STD_C 7
#define VISTAF_THERMAL_PEAK_TEMP_C 8
#define VISTAF_THERMAL_SURROUND_PIXELS 9
#define VISTAF_THERMAL_SURROUND_MEAN_C 10
#define VISTAF_THERMAL_CONTRAST_C 11
                                             /* 12..15 reserved (NaN) */

/* per-frame record: d_frame[b*VISTAF_NTHERMALFRAME + i] (double) */
#define VISTAF_NTHERMALFRAME 8
#define VISTAF_THERMALFRAME_REGISTERED_PIXELS 0
#define VISTAF_THERMALFRAME_SKIN_MEAN_C 1
#define VISTAF_THERMALFRAME_CONTACT_PIXELS 2
#define VISTAF_THERMALFRAME_CONTACT_MEAN_C 3
#define VISTAF_THERMALFRAME_CONTRAST_C 4
#define VISTAF_THERMALFRAME_HOTTEST_CONTACT 5
#define VISTAF_THERMALFRAME_COLDEST_CONTACT 6
                                             /* 7 reserved (NaN) */

typedef struct vistaf_thermal_handle vistaf_thermal_handle;

/* A thermal read-out for h x w crops (1..65536 each way, h*w below 2^31) of H x W photographs (each >= 2, H*W below 2^31) cropped at
 * (crop_x1, crop_y1) (each at most 2^20 in magnitude), the aligner's apply_global_shift flag, at most max_batch (1..65535) frames per call,
 * tables of max_contacts rows (1..VISTAF_MAX_CONTACTS = 64), surround_margin_px in 0..4096.  No HIP call is made and no call needs a
 * workspace on the device.  VISTAF_E_INVALID for a NULL `out` or arguments outside these ranges. */
int vistaf_thermal_create(int h, int w, int H, int W, int crop_x1, int crop_y1, int apply_global_shift, int max_batch, int max_contacts,
                          int surround_margin_px, vistaf_thermal_handle **out);

/* Register `batch` temperature maps.  Inputs (device): d_temp_map [B,H,W] float32 (the map of vistaf_tsensor_predict, NaN where it has no
 * value), d_align_info [B, VISTAF_ALIGN_NINFO] double as vistaf_align_batch wrote it for the same photographs, or NULL.  Output (device):
 * d_temp_crop [B,h,w] float32.  Asynchronous on `stream`; one launch, allocates nothing, no memset.  Every argument is checked before the
 * first HIP call: VISTAF_E_INVALID for a NULL handle, map or output (the message names it) or `batch` outside 1..max_batch; VISTAF_E_HIP
 * for a runtime failure. */
int vistaf_thermal_register(vistaf_thermal_handle *th, const float *d_temp_map, const double *d_align_info, int batch, float *d_temp_crop,
                            void *stream);

/* Measure every contact of `batch` frames.  Inputs (device): d_temp_crop [B,h,w] float32 (vistaf_thermal_register's output), d_depth_mm
 * [B,h,w] float32 (the height map of a predict), d_contact_index [B,h,w] int8, d_contacts [B, max_contacts, VISTAF_NCONTACT] double and
 * d_count [B] int32 as vistaf_ftp_contacts wrote them with the same max_contacts, d_status [B] int32 or NULL (every frame OK).  Outputs
 * (device): d_thermal [B, max_contacts, VISTAF_NTHERMAL] and d_frame [B, VISTAF_NTHERMALFRAME] double.  Asynchronous on `stream`; two
 * launches, allocates nothing, no memset.  Every argument is checked before the first HIP call: VISTAF_E_INVALID for a NULL argument
 * other than d_status (the message names it), `batch` outside 1..max_batch or a depth_eps_mm that is not finite; VISTAF_E_HIP for a runtime
 * failure. */
int vistaf_thermal_measure(vistaf_thermal_handle *th, const float *d_temp_crop, const float *d_depth_mm, const int8_t *d_contact_index,
                           const double *d_contacts, const int32_t *d_count, const int32_t *d_status, float depth_eps_mm, int batch,
                           double *d_thermal, double *d_frame, void *stream);

void vistaf_thermal_destroy(vistaf_thermal_handle *th);

#ifdef __cplusplus
}
#endif
#endif /* VISTAF_THERMAL_H */
