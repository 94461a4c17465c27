/* vistaf_cloud.h -- C ABI of the point-cloud read-out, part of libvistaf_ftp.so.
 *
 * An extension with no counterpart in the reference: every other read-out summarises the float32 depth plane (rows per contact, cells, time
 * series); none hands a consumer the touched surface itself.  The point-cloud read-out turns the planes of a batch, on the device, into what
 * a grasp planner, a registration or pose estimator or a point-cloud publisher consumes: the surface pixels as metric points in millimetres,
 * each with its unit normal, mean and Gaussian curvature, compacted in a fixed order, and one row per frame with the areas, the mean
 * normal and the steepest slope.  It is an object of its own: it never touches a vistaf_ftp_handle and reads only what it is handed.
 *
 * DEFINITION, for frame b; s = mm_per_px[b] (a double), eps = depth_eps_mm (a float32).  Every operation is in float64 unless a type is
 * written, there is no fused multiply-add, and the order of the operations is exactly as written.
 *
 * 1. DEPTH.  d(x, y) is the float32 depth, or 0 where the depth is not finite (d32); it is then widened to float64.  A neighbour outside
 *    the frame takes the value of the nearest pixel inside it (coordinates are clamped).
 * 2. A SURFACE PIXEL has d32 > eps, a float32 compare.  A POINT is a surface pixel with x % stride == 0 and y % stride == 0.  The points
 *    of a frame are ordered by pixel index y * w + x, frames by b.
 * 3. DERIVATIVES, with the neighbours l, r (x - 1, x + 1), u, dn (y - 1, y + 1), the centre c and the diagonals ul, ur, bl, br
 *    (u / b: y - 1 / y + 1):
 *       dx  = (r - l) / (2 * s)                     dy  = (dn - u) / (2 * s)
 *       dxx = ((r - c) - (c - l)) / (s * s)         dyy = ((dn - c) - (c - u)) / (s * s)
 *       dxy = ((br - bl) - (ur - ul)) / (4 * (s * s))
 * 4. NORMAL AND CURVATURE.
 *       g  = (1 + dx * dx) + dy * dy                rt = sqrt(g)
 *       nx = dx / rt        ny = dy / rt            nz = 1 / rt
 *       Hc = (((1 + dy * dy) * dxx - (2 * (dx * dy)) * dxy) + (1 + dx * dx) * dyy) / (2 * (g * rt))         mean curvature
 *       Kc = (dxx * dyy - dxy * dxy) / (g * g)                                                              Gaussian curvature
 *    Hc is negative on a cap (a ball pressed into the skin), as the curvatures of the per-contact quadric fit are.
 * 5. THE POINT RECORD is 8 float32 (32 bytes), every field rounded once from float64:
 *       X = (x - origin_x) * s     Y = (y - origin_y) * s     Z = -d     nx  ny  nz  Hc  Kc
 *    The frame is the right-handed camera-optical one: x right, y down, z away from the camera.  A press moves the skin towards the camera,
 *    so Z <= 0, and the normal points at the object.
 * 6. SIDE ARRAYS.  pixel (int32) holds y * w + x of every point; label (int8) the value of the contact index plane at the pixel, written
 *    only when both the plane and the output are given.
 * 7. OFFSETS [batch + 1] int64: the points of frame b are those numbered offsets[b] .. offsets[b + 1] - 1.  They are never capped.
 * 8. CAPACITY.  A point whose number is >= max_points is not written; nothing at or beyond max_points, and nothing between the last
 *    written point and max_points, is touched.  Overflow is reported through the offsets and the frame row; it is not an error.
 * 9. THE FRAME ROW, over the SURFACE PIXELS (the stride is ignored), n their number:
 *       SURFACE_PIXELS n; POINTS the points of the frame; POINTS_WRITTEN those of them that were written;
 *       PROJECTED_AREA_MM2 = n * (s * s); SURFACE_AREA_MM2 = (sum of rt) * (s * s);
 *       MEAN_NORMAL_X / _Y / _Z = (Sx, Sy, Sz) / sqrt((Sx * Sx + Sy * Sy) + Sz * Sz), S the sums of nx, ny, nz: the direction the object
 *       presses from; TILT_DEG = degrees(atan2(hypot(MEAN_NORMAL_X, MEAN_NORMAL_Y), MEAN_NORMAL_Z));
 *       MAX_SLOPE_DEG = degrees(atan(sqrt(q))), q the largest dx * dx + dy * dy (compared in float64);
 *       MAX_SLOPE_INDEX the first pixel (lowest y * w + x) that attains q; field 11 is reserved and NaN.
 *    With n == 0 the counts and areas are 0 and fields 5..10 are NaN.  The sum of rt and the three sums of the normal are float64 and are formed in an order fixed by h * w
 *    and the launch geometry alone (pixel -> lane -> wave -> chunk -> lane of the row kernel), without float atomics: the same inputs give
 *    the same bits whatever the batch a frame is part of, and a frame's points do not depend on the frames before it except through
 *    their position.  atan, atan2 and hypot are the device library's; every other operation is a correctly rounded + - * / or sqrt.
 * 10. A SKIPPED frame is one whose status is not 0 (VISTAF_FRAME_OK).  It has no points (offsets[b + 1] == offsets[b]), its row is all
 *    NaN and no plane of it is read.
 * With mm_per_px that is 0 or not finite, or a depth whose derivatives overflow, the operations still run as written, the non-finite
 * values propagate as IEEE 754 has it, and MAX_SLOPE_DEG / MAX_SLOPE_INDEX are then unspecified.
 *
 * NOT PART OF IT: smoothing of the depth before it is differentiated (the plane is already the reference's sigma-filtered one); meshing;
 * camera intrinsics (the points are orthographic, the pixel grid scaled by mm_per_px); a margin of untouched skin around a contact.
 *
 * Every function returns 0 or a negative VISTAF_E_* code (vistaf_ftp.h); vistaf_ftp_last_error() holds the message.  Arguments are checked
 * before any HIP call.  Calls on one handle must be ordered (one stream, or the caller's own events).
 */
#ifndef VISTAF_CLOUD_H
#define VISTAF_CLOUD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* point record written by vistaf_cloud_measure: d_points[k*VISTAF_NCLOUD_POINT + i] (float) */
#define VISTAF_NCLOUD_POINT 8
#define VISTAF_CLOUD_X 0
#define VISTAF_CLOUD_Y 1
#define VISTAF_CLOUD_Z 2
#define VISTAF_CLOUD_NX 3
#define VISTAF_CLOUD_NY 4
#define VISTAF_CLOUD_NZ 5
#define VISTAF_CLOUD_CURVATURE 6            /* Hc, 1/mm */
#define VISTAF_CLOUD_GAUSSIAN_CURVATURE 7   /* Kc, 1/mm^2 */

/* frame row: d_frame[b*VISTAF_NCLOUD_FRAME + i] (double) */
#define VISTAF_NCLOUD_FRAME 12
#define VISTAF_CLOUDFRAME_SURFACE_PIXELS 0
#define VISTAF_CLOUDFRAME_POINTS 1
#define VISTAF_CLOUDFRAME_POINTS_WRITTEN 2
#define VISTAF_CLOUDFRAME_PROJECTED_AREA_MM2 3
#define VISTAF_CLOUDFRAME_SURFACE_AREA_MM2 4
#define VISTAF_CLOUDFRAME_MEAN_NORMAL_X 5
#define VISTAF_CLOUDFRAME_MEAN_NORMAL_Y 6
#define VISTAF_CLOUDFRAME_MEAN_NORMAL_Z 7
#define VISTAF_CLOUDFRAME_TILT_DEG 8
#define VISTAF_CLOUDFRAME_MAX_SLOPE_DEG 9
#define VISTAF_CLOUDFRAME_MAX_SLOPE_INDEX 10
#define VISTAF_CLOUDFRAME_RESERVED 11

/* launch geometry, which fixes the order of the float64 sums: a workgroup of VISTAF_CLOUD_CHUNK_THREADS threads owns a chunk of that many
 * pixels of one frame, four times as many when h * w is a multiple of 4; the scan of the batch * chunks counts takes VISTAF_CLOUD_SCAN_THREADS
 * of them a round; in the row kernel lane l of VISTAF_CLOUD_ROW_LANES adds the records of chunks l, l + VISTAF_CLOUD_ROW_LANES, ... of a frame
 * in ascending order, VISTAF_CLOUD_ROW_UNROLL of them a round of its loop, so a round of the wave takes ROW_LANES * ROW_UNROLL chunks */
#define VISTAF_CLOUD_CHUNK_THREADS 256
#define VISTAF_CLOUD_SCAN_THREADS 1024
#define VISTAF_CLOUD_ROW_LANES 64
#define VISTAF_CLOUD_ROW_UNROLL 4

typedef struct vistaf_cloud_handle vistaf_cloud_handle;

/* A read-out for h x w planes (each 1..65536, below 2^31 pixels), at most max_batch (1..65535) frames per call, at most max_points (>= 1)
 * points written per call, every stride-th (1..64) column and row, the origin of X and Y at pixel (origin_x, origin_y) (finite; the crop
 * centre is ((w - 1) / 2, (h - 1) / 2)).  Makes no HIP call: the one device buffer (the counts and bases of max_batch * chunks chunks and
 * their partial records) is allocated on the current device by the first measure, and nothing after it.  VISTAF_E_INVALID, with the
 * argument's name in the message, for a NULL `out`, an argument outside these ranges, or max_batch times the chunks of a frame (see the
 * launch geometry above) at or above 2^31. */
int vistaf_cloud_create(int h, int w, int max_batch, int64_t max_points, int stride, double origin_x, double origin_y, vistaf_cloud_handle **out);

/* Measure `batch` frames.  Inputs (device): d_depth_mm [B,h,w] float32, d_mm_per_px [B] double, d_status [B] int32 or NULL (every frame
 * OK), d_contact_index [B,h,w] int8 or NULL.  Outputs (device): d_points [max_points, 8] float32, 16-byte aligned; d_pixel [max_points]
 * int32; d_label [max_points] int8 or NULL; d_offsets [B + 1] int64; d_frame [B, VISTAF_NCLOUD_FRAME] double.  When h * w is a multiple of
 * 4 the depth is read 16 bytes at a time and d_depth_mm must be 16-byte aligned.  Asynchronous on `stream`; four launches, no memset, no
 * atomics.  VISTAF_E_INVALID for a NULL handle, d_depth_mm, d_mm_per_px, d_points, d_pixel, d_offsets or d_frame, `batch` outside
 * 1..max_batch, or a misaligned d_points or d_depth_mm; VISTAF_E_HIP for a runtime failure. */
int vistaf_cloud_measure(vistaf_cloud_handle *cl, const float *d_depth_mm, const double *d_mm_per_px, const int32_t *d_status,
                         const int8_t *d_contact_index, float depth_eps_mm, int batch, float *d_points, int32_t *d_pixel, int8_t *d_label,
                         int64_t *d_offsets, double *d_frame, void *stream);

void vistaf_cloud_destroy(vistaf_cloud_handle *cl);

#ifdef __cplusplus
}
#endif
#endif /* VISTAF_CLOUD_H */
