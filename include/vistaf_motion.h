/* vistaf_motion.h -- C ABI of the contact motion read-out, part of libvistaf_ftp.so.
 *
 * An extension with no counterpart in the reference: the tracker (vistaf_track.h) says which touch of the frame before a contact continues
 * and how far its footprint centroid went; this says how the touching object moved against the skin -- slide (tx, ty), twist (theta) and
 * lift or press (beta) -- by registering the depth surface the parent left in frame t-1 onto the depth plane of frame t: a dense
 * registration of depth, not of footprints.  A ball pressed harder without sliding moves its centroid when the footprint grows unevenly
 * and has tx = ty = 0 here; an object that turns in place does not move its centroid and has theta here.  It is an object of its own: it
 * never touches another handle and reads only what it is handed, the depth planes of a predict, the index planes, tables and counts
 * vistaf_ftp_contacts wrote for them and the rows vistaf_track_update wrote for those.
 *
 * THE DEFINITION for frame t, row k of a table of K = max_contacts rows.  Float64 throughout, no fused multiply-add; every expression is
 * evaluated left to right as written.  s = mm_per_px[t], eps = depth_eps_mm.  A depth that is not finite counts as 0.  The frame before t
 * is frame t-1 of the same update, and for t = 0 the frame the handle carried over from the update before (none after create or reset).
 *   0. kk = min(max(count[t], 0), K); m the same of the frame before (0 if there is none).  A row k >= kk is all NaN.
 *      p = PARENT_ROW of d_tracks[t][k].  Status NO_PARENT when p is not finite, p < 0 or p >= m: the row is
 *      [p (or -1 when not finite), 0, NO_PARENT, 0, NaN ...].
 *   1. TEMPLATE PIXELS Omega: the pixels of the parent's box (BBOX_X0..Y1 of row p of the table of the frame before, clipped to the frame; a
 *      box that is not finite or is empty after clipping holds no pixel) with index[t-1] == p and T32 > float32(eps), T32 the float32
 *      depth of frame t-1 with non-finite values replaced by 0.  n = their number.  T = T32 widened to float64, I the same of frame t,
 *      both read at coordinates clamped to the frame.  Centre cx = Sx/n, cy = Sy/n from the exact integer sums of x and y over Omega, each
 *      converted once.  R = 0.5 * sqrt(bw*bw + bh*bh), bw and bh the width and height of the clipped box.  The row starts
 *      [p, n, status, iterations run]; CENTRE_X/Y are written when n > 0.  Status TOO_FEW when n < min_pixels, nothing else is written.
 *   2. Per pixel of Omega, on the integer grid:  Tx = (T(x+1, y) - T(x-1, y)) / 2,  Ty = (T(x, y+1) - T(x, y-1)) / 2,  ux = x - cx,
 *      uy = y - cy,  g = (Tx, Ty, ux*Ty - uy*Tx, 1).  H = sum over Omega of g g^T: the nine sums Tx*Tx, Tx*Ty, Tx*g2, Tx, Ty*Ty, Ty*g2, Ty,
 *      g2*g2, g2, and H33 = n.  Status SINGULAR, nothing else written, unless chol_solve<4> (csrc/chol.hpp) succeeds on H - 2^-32 * diag(H)
 *      and on H: the floor of vistaf_shape.h step 5.
 *   3. State theta = 0, beta = 0, (tx, ty) = (DX, DY) of d_tracks[t][k] when init_from_centroid is set and both are finite, else (0, 0).
 *      The warp about the centre:  c = cos(theta), sn = sin(theta),
 *        wx = ((cx + c*ux) - sn*uy) + tx,   wy = ((cy + sn*ux) + c*uy) + ty.
 *      The sample I(W): qx = wx when 0 <= wx <= w-1, w-1 when wx > w-1, else 0 (a NaN goes to 0); qy likewise; x0 = floor(qx),
 *      x1 = min(x0 + 1, w-1), fx = qx - x0, y0, y1, fy likewise;
 *        top = (1 - fx)*I(x0, y0) + fx*I(x1, y0),  bot = (1 - fx)*I(x0, y1) + fx*I(x1, y1),  I(W) = (1 - fy)*top + fy*bot.
 *   4. A SWEEP over Omega with the current state:  r = (I(W) - beta) - T,  b = sum g*r (four sums),  rss = sum r*r.
 *      Exactly `iterations` steps, each one sweep followed by  d = chol_solve<4>(H, b)  and the inverse-compositional update
 *        theta = theta - d2;  c = cos(theta), sn = sin(theta);  tx = tx - (c*d0 - sn*d1);  ty = ty - (sn*d0 + c*d1);  beta = beta + d3
 *      (W o W(d)^-1 of two rigid maps about the centre).  step = max(|d0|, |d1|, |d2|*R).  rss_before is the rss of the first sweep.
 *      One more sweep with the final state gives rss_after.
 *   5. Status OK when the last step <= tol_px, else NOT_CONVERGED (a NaN step too); the values are written either way.
 *      RMS_BEFORE_MM = sqrt(rss_before/n), RMS_AFTER_MM = sqrt(rss_after/n), TX_MM = tx*s, TY_MM = ty*s.
 *      SE_i = sqrt(z_i * (rss_after / max(n - 4, 1))) for i = tx, ty, theta, z_i component i of chol_solve<4>(H, e_i): the standard error
 *      of the estimate under the residual it leaves.  A round cap's twist is unobservable: its SE_THETA is orders of magnitude above an
 *      anisotropic contact's, and that is where the row says so (it is SINGULAR only when the floor of step 2 says so).
 *      TX_MINUS_DX = tx - DX, TY_MINUS_DY = ty - DY (NaN when the tracker's is): the part of the centroid motion that is footprint change.
 *   6. The frame row, over the rows of the frame with status OK in ascending order: their number; the largest
 *      sqrt(TX_MM*TX_MM + TY_MM*TY_MM) and its row, the largest |theta| and its row (ties to the lowest row); the n-weighted means
 *      (sum n*v) / (sum n) of TX_MM, TY_MM and RMS_AFTER_MM, sums in ascending row order.  Without such a row the number is 0 and the
 *      rest NaN.  A frame with kk == 0 (every frame whose status is not VISTAF_FRAME_OK) has no pair and a row that is all NaN.
 *   Every float64 sum over Omega is formed in an order fixed by the box and the launch geometry alone (pixel -> lane -> wave -> workgroup),
 *   without float atomics: two updates, two handles, or a frame in another position of a batch give the same bits.
 *
 * Every function returns 0 or a negative VISTAF_E_* code (vistaf_ftp.h); vistaf_ftp_last_error() holds the message.  Nothing is ever
 * refused for what the data holds: that is what the status is for.
 */
#ifndef VISTAF_MOTION_H
#define VISTAF_MOTION_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* per-contact record written by vistaf_motion_update: d_motion[(b*max_contacts + k)*VISTAF_NMOTION + i] (double), row k = row k of frame b's
 * contacts table.  Unused rows and fields are NaN, as in the contacts table. */
#define VISTAF_NMOTION 24
#define VISTAF_MOTION_PARENT_ROW 0        /* the tracker's PARENT_ROW; -1 when that is not finite                                     */
#define VISTAF_MOTION_TEMPLATE_PIXELS 1   /* n: the parent's contact pixels; 0 with NO_PARENT                                         */
#define VISTAF_MOTION_STATUS 2            /* VISTAF_MOTIONST_*                                                                        */
#define VISTAF_MOTION_ITERATIONS 3        /* steps run: `iterations` with OK and NOT_CONVERGED, else 0                                */
#define VISTAF_MOTION_TX_PX 4             /* slide of the object against the skin from frame t-1 to t, crop pixels ...                */
#define VISTAF_MOTION_TY_PX 5
#define VISTAF_MOTION_THETA_RAD 6         /* ... its twist about the centre, positive from x towards y ...                            */
#define VISTAF_MOTION_BETA_MM 7           /* ... and the uniform depth change: I(W(x)) ~ T(x) + beta                                  */
#define VISTAF_MOTION_TX_MM 8
#define VISTAF_MOTION_TY_MM 9
#define VISTAF_MOTION_CENTRE_X 10         /* centre of the twist: the parent's unweighted footprint centroid (crop pixels)            */
#define VISTAF_MOTION_CENTRE_Y 11
#define VISTAF_MOTION_RMS_BEFORE_MM 12    /* root mean square residual at the start ...                                               */
#define VISTAF_MOTION_RMS_AFTER_MM 13     /* ... and with the final estimate                                                          */
#define VISTAF_MOTION_LAST_STEP_PX 14     /* max(|d tx|, |d ty|, |d theta| * R) of the last step                                      */
#define VISTAF_MOTION_SE_TX_PX 15         /* standard errors of tx, ty, theta                                                         */
#define VISTAF_MOTION_SE_TY_PX 16
#define VISTAF_MOTION_SE_THETA_RAD 17
#define VISTAF_MOTION_TX_MINUS_DX 18      /* tx - the tracker's DX: centroid motion that is footprint change, not sliding             */
#define VISTAF_MOTION_TY_MINUS_DY 19
                                          /* 20..23 reserved (NaN) */

#define VISTAF_MOTIONST_OK 0              /* registered: the last step is at most tol_px                                              */
#define VISTAF_MOTIONST_NOT_CONVERGED 1   /* the last step is larger; the values are written                                          */
#define VISTAF_MOTIONST_NO_PARENT 2       /* born, or the parent is not a row of the frame before                                     */
#define VISTAF_MOTIONST_TOO_FEW 3         /* fewer than min_pixels template pixels                                                    */
#define VISTAF_MOTIONST_SINGULAR 4        /* the template does not determine the four parameters (a flat, a ridge)                    */

/* per-frame record: d_frame[b*VISTAF_NMOTIONFRAME + i] (double) */
#define VISTAF_NMOTIONFRAME 8
#define VISTAF_MOTIONFRAME_REGISTERED 0       /* rows with status OK                                         */
#define VISTAF_MOTIONFRAME_MAX_SLIDE_MM 1     /* largest sqrt(tx_mm^2 + ty_mm^2) among them ...              */
#define VISTAF_MOTIONFRAME_MAX_SLIDE_ROW 2    /* ... and its row                                             */
#define VISTAF_MOTIONFRAME_MAX_TWIST_RAD 3    /* largest |theta| ...                                         */
#define VISTAF_MOTIONFRAME_MAX_TWIST_ROW 4    /* ... and its row                                             */
#define VISTAF_MOTIONFRAME_MEAN_TX_MM 5       /* n-weighted means                                            */
#define VISTAF_MOTIONFRAME_MEAN_TY_MM 6
#define VISTAF_MOTIONFRAME_MEAN_RMS_AFTER_MM 7

typedef struct vistaf_motion_handle vistaf_motion_handle;

/* A motion read-out for h x w planes, at most max_batch frames per update, tables of max_contacts rows (1..VISTAF_MAX_CONTACTS = 64: the K of
 * the vistaf_ftp_contacts and vistaf_track_update calls that feed it), iterations 1..16, tol_px finite and >= 0, min_pixels >= 1,
 * init_from_centroid 0 or 1.  Makes no call of the runtime: the workspace (the carried frame) is allocated by the first update.
 * VISTAF_E_INVALID for a NULL `out` or arguments outside these ranges. */
int vistaf_motion_create(int h, int w, int max_batch, int max_contacts, int iterations, double tol_px, int min_pixels, int init_from_centroid,
                         vistaf_motion_handle **out);

/* Register every linked contact of `batch` frames, consecutive in time; frame 0 follows the last frame of the update before (the handle
 * keeps that frame's depth plane, index plane, table and count on the device).  Inputs (device): d_depth_mm [B,h,w] float32 (the height
 * map of a predict), d_contact_index [B,h,w] int8, d_contacts [B, max_contacts, VISTAF_NCONTACT] double and d_count [B] int32 as
 * vistaf_ftp_contacts wrote them, d_tracks [B, max_contacts, VISTAF_NTRACK] double as vistaf_track_update wrote it for the same frames
 * (the tracker and this handle must have seen the same sequence), d_mm_per_px [B] double.  Outputs (device): d_motion
 * [B, max_contacts, VISTAF_NMOTION] double, d_frame [B, VISTAF_NMOTIONFRAME] double.  Asynchronous on `stream`; three launches, no memset,
 * no atomics.  VISTAF_E_INVALID for a NULL argument, `batch` outside 1..max_batch, a depth_eps_mm that is not finite or a pointer that is
 * not aligned to its element, VISTAF_E_HIP for a runtime failure. */
int vistaf_motion_update(vistaf_motion_handle *mo, const float *d_depth_mm, const int8_t *d_contact_index, const double *d_contacts,
                         const int32_t *d_count, const double *d_tracks, const double *d_mm_per_px, float depth_eps_mm, int batch,
                         double *d_motion, double *d_frame, void *stream);

/* Forget the carried frame: every row of frame 0 of the next update is NO_PARENT.  Takes effect at the head of that update, on its stream. */
int vistaf_motion_reset(vistaf_motion_handle *mo);

void vistaf_motion_destroy(vistaf_motion_handle *mo);

#ifdef __cplusplus
}
#endif
#endif /* VISTAF_MOTION_H */
