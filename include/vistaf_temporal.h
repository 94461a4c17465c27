/* vistaf_temporal.h -- C ABI of the temporal read-out, part of libvistaf_ftp.so.
 *
 * An extension with no counterpart in the reference: every other read-out but the tracker describes one frame in isolation, and the tracker
 * links table rows, not pixels.  The temporal read-out follows every pixel of a stream of float32 planes (the height maps of consecutive
 * predicts) through time on the device: a filtered depth without frame-to-frame flicker, its rate, a touch bit with hysteresis, how long the
 * bit has held, the largest raw depth of the running touch, and per frame the counts, extremes and events a controller asks of a skin.
 * It is an object of its own: it never touches a vistaf_ftp_handle and reads only what it is handed.
 *
 * PARAMETERS (create): alpha in (0, 1], on_mm > off_mm >= 0, all finite, each a double rounded ONCE to float32 (alpha, on, off below are
 * those float32 values); frame_period_s finite and > 0, kept as a double (period below).
 *
 * STATE on the device, carried from update to update.  Per pixel: filt f32 (filtered depth), rate f32 (mm/s), touch u8 (0 or 1), dwell i32
 * (accepted frames since the pixel's touch bit last changed), hold f32 (largest raw depth since the pixel's touch began, 0 while not
 * touching).  Per stream: primed (an accepted frame has been seen), gap (skipped frames since the last accepted one), prev_touch_pixels and
 * prev_volume (TOUCH_PIXELS and FILTERED_VOLUME_CM3 of the last accepted frame).  After create or reset every plane is 0, primed = 0, gap = 0.
 *
 * ONE UPDATE takes `batch` frames, consecutive in time; frame 0 follows the last frame of the previous update.  Frames are taken in order.
 *
 * A SKIPPED frame is one whose status is not 0 (VISTAF_FRAME_OK).  No plane of it is read, the per-pixel state is unchanged, its row is NaN
 * except GAP_FRAMES, its per-frame output planes (when asked for) hold the held state (filt and touch as they stand), and then gap += 1.
 *
 * AN ACCEPTED frame, per pixel p, every operation in float32 unless a type is written, no fused multiply-add, in this order:
 *    d      = depth[p] if it is finite, else 0
 *    fp     = primed ? filt : d
 *    f      = fp + alpha * (d - fp)                                  one subtraction, one product, one sum
 *    rate   = float32( double(f - fp) / (double(gap + 1) * period) ) the subtraction in float32, product and quotient in float64
 *    touch' = touch ? (f > off) : (f >= on)                          the Schmitt trigger
 *    dwell' = (touch' == touch) ? dwell + 1 : 0
 *    hold'  = touch' ? larger(touch ? hold : 0, d) : 0               larger(a, d) = (d > a) ? d : a
 *    filt   = f
 * and after the frame primed = 1, gap = 0.  Should the filter overflow float32 the operations still run as written, the non-finite values
 * propagate as IEEE 754 has it, and the maxima and minima of the frame row are then unspecified.
 *
 * THE FRAME ROW of an accepted frame (fields below), over the pixels with touch' = 1 ("touching"):
 *    TOUCH_PIXELS their number; ONSET_PIXELS pixels with touch = 0, touch' = 1; RELEASE_PIXELS pixels with touch = 1, touch' = 0;
 *    LOADING_PIXELS touching with f > fp; UNLOADING_PIXELS touching with f < fp;
 *    FILTERED_VOLUME_CM3 = S * (s * s) / 1000, S the float64 sum of double(f) over the touching pixels, s = mm_per_px of the frame;
 *    DVOLUME_CM3_PER_S = (volume - prev_volume) / (double(gap + 1) * period), NaN on the first accepted frame since create or reset;
 *    MAX_FILTERED_MM / ARGMAX_INDEX the largest f and the first pixel (lowest y * w + x) that attains it;
 *    MAX_RATE_MM_PER_S / MAX_RATE_INDEX and MIN_RATE_MM_PER_S / MIN_RATE_INDEX the same for the largest and the smallest rate;
 *    LONGEST_DWELL_FRAMES the largest dwell';
 *    EVENTS: VISTAF_TEMPEV_TOUCH_BEGAN when prev_touch_pixels == 0 and TOUCH_PIXELS > 0, VISTAF_TEMPEV_TOUCH_ENDED when
 *    prev_touch_pixels > 0 and TOUCH_PIXELS == 0 (prev_touch_pixels is 0 before the first accepted frame);
 *    GAP_FRAMES the value of gap at the head of the frame, for accepted and skipped frames alike.
 * A frame without touching pixels has volume 0 and NaN in fields 7..13.
 * The sum S is formed in an order fixed by h * w alone (pixel -> lane -> wave -> chunk), so a row depends neither on `batch` nor on how a
 * stream is cut into updates, and two handles fed the same stream give the same bits.
 *
 * NOT PART OF IT: per-frame timestamps (the period is fixed); a debounce count (the hysteresis band is the only guard against chatter);
 * bridging the tracker's gaps; filtering the temperature plane -- the object takes any float32 plane stream, but only depth is wired into
 * FtpSensor and tested.
 *
 * Every function returns 0 or a negative VISTAF_E_* code (vistaf_ftp.h); vistaf_ftp_last_error() holds the message.  Arguments are checked
 * before any HIP call.  Updates of one handle must be ordered (one stream, or the caller's own events).
 */
#ifndef VISTAF_TEMPORAL_H
#define VISTAF_TEMPORAL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* frame row written by vistaf_temporal_update: d_rows[b*VISTAF_NTEMPORAL + i] (double) */
#define VISTAF_NTEMPORAL 16
#define VISTAF_TEMPORAL_TOUCH_PIXELS 0
#define VISTAF_TEMPORAL_ONSET_PIXELS 1
#define VISTAF_TEMPORAL_RELEASE_PIXELS 2
#define VISTAF_TEMPORAL_LOADING_PIXELS 3
#define VISTAF_TEMPORAL_UNLOADING_PIXELS 4
#define VISTAF_TEMPORAL_FILTERED_VOLUME_CM3 5
#define VISTAF_TEMPORAL_DVOLUME_CM3_PER_S 6
#define VISTAF_TEMPORAL_MAX_FILTERED_MM 7
#define VISTAF_TEMPORAL_ARGMAX_INDEX 8
#define VISTAF_TEMPORAL_MAX_RATE_MM_PER_S 9
#define VISTAF_TEMPORAL_MAX_RATE_INDEX 10
#define VISTAF_TEMPORAL_MIN_RATE_MM_PER_S 11
#define VISTAF_TEMPORAL_MIN_RATE_INDEX 12
#define VISTAF_TEMPORAL_LONGEST_DWELL_FRAMES 13
#define VISTAF_TEMPORAL_EVENTS 14           /* bitmask of VISTAF_TEMPEV_* */
#define VISTAF_TEMPORAL_GAP_FRAMES 15

#define VISTAF_TEMPEV_TOUCH_BEGAN 1         /* the touch pixels went from 0 to more than 0 */
#define VISTAF_TEMPEV_TOUCH_ENDED 2         /* the touch pixels went from more than 0 to 0 */

typedef struct vistaf_temporal_handle vistaf_temporal_handle;

/* A read-out for h x w planes (each 1..65536, below 2^31 pixels), at most max_batch (1..65535) frames per update.  Makes no HIP call: the
 * one device buffer (five state planes, the stream scalars, the partial records of max_batch frames) is allocated on the current device by
 * the first update, and nothing after it.  VISTAF_E_INVALID, with the argument's name in the message, for a NULL `out`, a size or max_batch
 * outside these ranges, a non-finite alpha, on_mm, off_mm or frame_period_s, alpha outside (0, 1], off_mm < 0, off_mm >= on_mm, or
 * frame_period_s <= 0. */
int vistaf_temporal_create(int h, int w, int max_batch, double alpha, double on_mm, double off_mm, double frame_period_s,
                           vistaf_temporal_handle **out);

/* Take `batch` frames.  Inputs (device): d_depth [B,h,w] float32, d_mm_per_px [B] double, d_status [B] int32 or NULL (every frame OK).
 * Outputs (device): d_rows [B, VISTAF_NTEMPORAL] double; d_filtered [B,h,w] float32 and d_touch [B,h,w] uint8, the state after every frame,
 * each written only when its pointer is not NULL.  When h * w is a multiple of 4 the planes are moved 16 bytes at a time: d_depth and
 * d_filtered must then be 16-byte aligned and d_touch 4-byte aligned.  Asynchronous on `stream`; three launches, no memset, no atomics.
 * VISTAF_E_INVALID for a NULL handle, d_depth, d_mm_per_px or d_rows, `batch` outside 1..max_batch, or a misaligned plane;
 * VISTAF_E_HIP for a runtime failure. */
int vistaf_temporal_update(vistaf_temporal_handle *tp, const float *d_depth, const double *d_mm_per_px, const int32_t *d_status, int batch,
                           double *d_rows, float *d_filtered, uint8_t *d_touch, void *stream);

/* Copy the five state planes out, device to device, asynchronously on `stream`: d_filt, d_rate, d_hold [h,w] float32, d_touch [h,w] uint8,
 * d_dwell [h,w] int32; a NULL pointer skips its plane.  After create or reset, before the next update, the planes are 0. */
int vistaf_temporal_state(vistaf_temporal_handle *tp, float *d_filt, float *d_rate, uint8_t *d_touch, int32_t *d_dwell, float *d_hold,
                          void *stream);

/* Forget the stream: takes effect at the head of the next update, on that update's stream. */
int vistaf_temporal_reset(vistaf_temporal_handle *tp);

void vistaf_temporal_destroy(vistaf_temporal_handle *tp);

#ifdef __cplusplus
}
#endif
#endif /* VISTAF_TEMPORAL_H */
