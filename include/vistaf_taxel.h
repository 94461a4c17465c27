/* vistaf_taxel.h -- C ABI of the taxel read-out, part of libvistaf_ftp.so.
 *
 * An extension with no counterpart in the reference: the contacts table (vistaf_ftp.h), the tracker (vistaf_track.h) and the shape read-out
 * (vistaf_shape.h) describe individual touches, rows that move from frame to frame.  This reduces a depth plane to a fixed array of TAXELS
 * -- the same cells every frame, a grid, rings and sectors of the ROI disc, or any patches the integrator drew -- with depth, volume and a
 * share of the frame's force per cell, and to the frame's wrench: normal force, centre of pressure, tilting moments.  It is an object of its
 * own: it never touches a vistaf_ftp_handle and reads only what it is handed, the depth plane, mm_per_px, force and status a predict wrote.
 *
 * THE LAYOUT is a host plane layout[y*w + x] of uint16: the taxel of the pixel, 0..n_taxels-1, or VISTAF_TAXEL_NONE for a pixel of no taxel.
 * Taxels need not be connected or rectangular; a taxel without a pixel is legal.  T = n_taxels, L_t = number of layout pixels of taxel t.
 *
 * THE DEFINITION for frame b, taxel t; s = mm_per_px[b], eps = depth_eps_mm, F = frame_force_N[b]:
 *   0. If d_status is given and status[b] != 0, every taxel row and the frame row of b are NaN; nothing of that frame's depth plane, scale
 *      or force is interpreted.
 *   1. Depth d is the plane's value, a NaN counting as 0 (and -0 as +0).  The CONTACT PIXELS of t are its layout pixels with
 *      d > float32(eps), a float32 compare as the tail's, the contacts table's and vistaf_shape.h step 1.  n = their number.
 *   2. In float64, over the contact pixels: S = sum d, Sx = sum x*d, Sy = sum y*d (x, y < 65536 and d a float32: every product is exact;
 *      no fused multiply-add anywhere).
 *   3. The taxel row, VISTAF_NTAXEL doubles:
 *        CONTACT_PIXELS    n
 *        CONTACT_AREA_MM2  n*(s*s)
 *        VOLUME_CM3        S*(s*s)/1000
 *        MEAN_DEPTH_MM     S/L_t, the taxel's average indentation; NaN when L_t == 0
 *        MAX_DEPTH_MM      maximum of d over the contact pixels; 0 when n == 0
 *        ARGMAX_INDEX      row-major index y*w + x of the first pixel that attains it; NaN when n == 0
 *        CENTROID_X, _Y    Sx/S, Sy/S; NaN when n == 0
 *        FORCE_N           the taxel's share of the frame's force, F*(S/S_frame), S_frame = the sum of S over the taxels in taxel order
 *                          0..T-1; 0 when S_frame == 0; NaN when d_frame_force_N is NULL
 *        PRESSURE_KPA      1000*FORCE_N/(L_t*(s*s)), the share over the whole area of the cell; NaN when L_t == 0
 *      FORCE_N is an APPORTIONING, not a measurement: the share a Winkler foundation (pressure proportional to indentation) gives the
 *      cell.  It is chosen because the shares add up to the frame's force.  The contacts table's per-contact force_N instead runs the
 *      non-linear volume-to-force curve on partial volumes, so its rows do not add up; the two are different quantities.
 *   4. The frame row, VISTAF_NTAXELFRAME doubles:
 *        ACTIVE_TAXELS     number of taxels with n > 0
 *        VOLUME_CM3        S_frame*(s*s)/1000
 *        FORCE_N           F, or NaN when d_frame_force_N is NULL
 *        COP_X, COP_Y      (sum_t Sx)/S_frame, (sum_t Sy)/S_frame, the sums in taxel order as S_frame; NaN when S_frame == 0
 *        MOMENT_X_NMM      F*(COP_Y - origin_y)*s, evaluated left to right
 *        MOMENT_Y_NMM      -(F*(COP_X - origin_x)*s): the moment about the origin of a force F along -z at the centre of pressure
 *        PEAK_TAXEL        the taxel with the largest MAX_DEPTH_MM among those with n > 0, ties to the lowest t; NaN with no active taxel
 *   5. Every float64 sum is formed in an order fixed by the layout and the launch geometry alone (pixel -> lane -> wave; taxel by taxel
 *      for the frame sums), without float atomics: two calls on the same inputs give the same bits, whatever the batch a frame is part of.
 *
 * Every function returns 0 or a negative VISTAF_E_* code (vistaf_ftp.h); vistaf_ftp_last_error() holds the message.
 */
#ifndef VISTAF_TAXEL_H
#define VISTAF_TAXEL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VISTAF_TAXEL_NONE 0xFFFF             /* layout value of a pixel that belongs to no taxel */

/* per-taxel record written by vistaf_taxel_measure: d_taxels[(b*n_taxels + t)*VISTAF_NTAXEL + i] (double) */
#define VISTAF_NTAXEL 12
#define VISTAF_TAXEL_CONTACT_PIXELS 0
#define VISTAF_TAXEL_CONTACT_AREA_MM2 1
#define VISTAF_TAXEL_VOLUME_CM3 2
#define VISTAF_TAXEL_MEAN_DEPTH_MM 3
#define VISTAF_TAXEL_MAX_DEPTH_MM 4
#define VISTAF_TAXEL_ARGMAX_INDEX 5
#define VISTAF_TAXEL_CENTROID_X 6
#define VISTAF_TAXEL_CENTROID_Y 7
#define VISTAF_TAXEL_FORCE_N 8
#define VISTAF_TAXEL_PRESSURE_KPA 9
                                             /* 10, 11 reserved (NaN) */

/* per-frame record: d_frame[b*VISTAF_NTAXELFRAME + i] (double) */
#define VISTAF_NTAXELFRAME 8
#define VISTAF_TAXELFRAME_ACTIVE_TAXELS 0
#define VISTAF_TAXELFRAME_VOLUME_CM3 1
#define VISTAF_TAXELFRAME_FORCE_N 2
#define VISTAF_TAXELFRAME_COP_X 3
#define VISTAF_TAXELFRAME_COP_Y 4
#define VISTAF_TAXELFRAME_MOMENT_X_NMM 5
#define VISTAF_TAXELFRAME_MOMENT_Y_NMM 6
#define VISTAF_TAXELFRAME_PEAK_TAXEL 7

typedef struct vistaf_taxel_handle vistaf_taxel_handle;

/* A taxel read-out for h x w planes (1..65536 each way, h*w below 2^31), at most max_batch (1..65535) frames per call, `layout` (host,
 * [h,w]) with n_taxels in 1..65535 taxels, the moments taken about (origin_x, origin_y) in crop pixels.  The layout is copied and inverted here, on the host: the
 * pixel indices sorted by (taxel, index) and where each taxel's run starts.  No HIP call is made: the lists go to the device current at the
 * first vistaf_taxel_measure.  VISTAF_E_INVALID for a NULL `layout` or `out`, sizes outside these ranges, origins that are not finite, or
 * a layout value >= n_taxels other than VISTAF_TAXEL_NONE. */
int vistaf_taxel_create(int h, int w, int max_batch, const uint16_t *layout, int n_taxels, double origin_x, double origin_y,
                        vistaf_taxel_handle **out);

/* Measure `batch` frames.  Inputs (device): d_depth_mm [B,h,w] float32 (the height map of a predict), d_mm_per_px [B] double,
 * d_frame_force_N [B] double or NULL, d_status [B] int32 or NULL (every frame OK).  Outputs (device): d_taxels [B, n_taxels, VISTAF_NTAXEL]
 * and d_frame [B, VISTAF_NTAXELFRAME] double.  Asynchronous on `stream`, two launches, no memset; the first call of a handle uploads the
 * lists (synchronously), later calls allocate nothing.  Every argument is checked before the first HIP call: VISTAF_E_INVALID for a NULL
 * handle, depth, scale or output, `batch` outside 1..max_batch or a depth_eps_mm that is not finite; VISTAF_E_HIP for a runtime failure. */
int vistaf_taxel_measure(vistaf_taxel_handle *tx, const float *d_depth_mm, const double *d_mm_per_px, const double *d_frame_force_N,
                         const int32_t *d_status, float depth_eps_mm, int batch, double *d_taxels, double *d_frame, void *stream);

/* The layout as the handle holds it (host, no HIP call): info[t*4 + 0] = L_t, 1 and 2 = the mean x and the mean y of the taxel's pixels
 * (NaN when L_t == 0), 3 reserved (NaN). */
int vistaf_taxel_layout_info(vistaf_taxel_handle *tx, double *info);

void vistaf_taxel_destroy(vistaf_taxel_handle *tx);

#ifdef __cplusplus
}
#endif
#endif /* VISTAF_TAXEL_H */
