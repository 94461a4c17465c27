/* vistaf_shape.h -- C ABI of the per-contact shape read-out, part of libvistaf_ftp.so.
 *
 * An extension with no counterpart in the reference: vistaf_ftp_contacts (vistaf_ftp.h) says where a touch is, how large, how deep and how
 * strong; this says what it looks like -- the ellipse of its footprint, its boundary, and the curvature of the cap it leaves in the depth
 * map (a ball, an edge, a flat punch).  It is an object of its own: it never touches a vistaf_ftp_handle and reads only what it is handed,
 * the depth plane a predict wrote and the index plane, table and counts vistaf_ftp_contacts wrote for it.
 *
 * THE DEFINITION for frame b, row k of a table of K = max_contacts rows; s = mm_per_px[b], eps = depth_eps_mm, f = fit_min_fraction:
 *   0. kk = min(max(count[b], 0), K).  A row k >= kk is all NaN.  Plane values outside 0..kk-1 count as -1.  A NaN depth counts as 0.
 *   1. The CONTACT PIXELS of k are the pixels with index == k and depth > float32(eps), a float32 compare as the tail's and the table's.
 *      Only the table's box (BBOX_X0..Y1, clipped to the frame) is searched: it must contain every pixel of k, as vistaf_ftp_contacts
 *      writes it.  A box that is not finite or is empty after clipping holds no pixel.  n = their number, (x, y) their crop coordinates.
 *   2. A contact pixel is a BOUNDARY PIXEL when one of its four neighbours (x-1, x+1, y-1, y+1) lies outside the frame or is not a
 *      contact pixel of k.
 *   3. Footprint, from the exact integer sums Sx = sum x, Sy, Sxx = sum x*x, Syy, Sxy, each converted to float64 once; no fused
 *      multiply-add anywhere:  cx = Sx/n, cy = Sy/n, mu20 = Sxx/n - cx*cx, mu02 = Syy/n - cy*cy, mu11 = Sxy/n - cx*cy,
 *      hd = (mu20 - mu02)/2, r = sqrt(hd*hd + mu11*mu11), l1 = max((mu20 + mu02)/2 + r, 0), l2 = max((mu20 + mu02)/2 - r, 0),
 *      major = 4*sqrt(l1)*s, minor = 4*sqrt(l2)*s (the full axes of the ellipse with the same moments),
 *      orientation = HALF(2*mu11, mu20 - mu02) with HALF(p, q) = 0 when p == 0 and q == 0, else 0.5*atan2(p, q), and pi/2 in place
 *      of -pi/2: a direction in (-pi/2, pi/2].  n == 0 leaves fields 2..6 NaN.
 *   4. The FIT PIXELS are the contact pixels with depth >= float32(f * peak), peak = the table's MAX_DEPTH_MM (a NaN threshold admits no
 *      pixel); f == 0 admits every contact pixel.  m = their number.
 *   5. The fit: least squares of d ~ c0 + c1*u + c2*v + c3*u*u + c4*u*v + c5*v*v over the fit pixels by normal equations in float64, in
 *      coordinates centred on the table's (unclipped) box and scaled to [-1, 1]:  u = (x - xc)/hx, xc = (bx0 + bx1)/2,
 *      hx = max((bx1 - bx0)/2, 1), v = (y - yc)/hy likewise.  The matrix A holds the 15 sums of u^a * v^b, a + b <= 4, the right-hand
 *      side the 6 sums of d * u^a * v^b, a + b <= 2; each monomial is a product of float64 factors (u*u, (u*u)*u, (u*u)*(u*u), ...).
 *      status 1 (no fit) when m < 6 or A is not safely positive definite: chol_solve<6> (csrc/chol.hpp) must succeed on
 *      A - 2^-32 * diag(A) and on A; the solution is that of A.  The floor makes the verdict on a rank-deficient set of pixels (a line, two
 *      rows, a conic) independent of the last bit of a pivot: it asks that the smallest singular value of the design matrix with columns
 *      of unit length exceed 2^-16.
 *   6. In millimetres, about the box centre: ax = hx*s, ay = hy*s, q3 = c3/(ax*ax), q4 = c4/(ax*ay), q5 = c5/(ay*ay).  The Hessian is
 *      [[2*q3, q4], [q4, 2*q5]]: mean = q3 + q5, dev = sqrt((q3 - q5)*(q3 - q5) + q4*q4), eigenvalues mean - dev and mean + dev.
 *      curvature_1 is the one of larger magnitude (mean - dev when mean <= 0, else mean + dev), curvature_2 the other;
 *      curvature_axis = HALF(q4, q3 - q5) when curvature_1 = mean + dev, else HALF(-q4, q5 - q3).
 *      status 2 (fitted, not a cap) unless mean + dev < 0, i.e. unless the Hessian is negative definite; else status 0.
 *   7. status 0 only: the stationary point  det = 4*c3*c5 - c4*c4, ua = (c4*c2 - 2*c5*c1)/det, va = (c4*c1 - 2*c3*c2)/det,
 *      apex_x = xc + ua*hx, apex_y = yc + va*hy, apex_depth = P(ua, va) with
 *      P(u, v) = c0 + c1*u + c2*v + c3*(u*u) + c4*(u*v) + c5*(v*v) summed left to right;  radius_i = -1/curvature_i.
 *   8. status 0 and 2: fit_rms = sqrt(sum (d - P(u, v))^2 / m) over the fit pixels, a second sweep with the solved coefficients.
 *   Every float64 sum is formed in an order fixed by the box and the launch geometry alone (pixel -> lane -> wave -> workgroup), without
 *   float atomics: two calls on the same inputs give the same bits, whatever the batch a frame is part of.
 *
 * Every function returns 0 or a negative VISTAF_E_* code (vistaf_ftp.h); vistaf_ftp_last_error() holds the message.
 */
#ifndef VISTAF_SHAPE_H
#define VISTAF_SHAPE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* per-contact record written by vistaf_shape_measure: d_shapes[(b*max_contacts + k)*VISTAF_NSHAPE + i] (double), row k = row k of frame b's
 * contacts table.  Unused rows and fields are NaN, as in the contacts table. */
#define VISTAF_NSHAPE 24
#define VISTAF_SHAPE_CONTACT_PIXELS 0        /* n; equals the table's VISTAF_CONTACT_CONTACT_PIXELS                                   */
#define VISTAF_SHAPE_BOUNDARY_PIXELS 1       /* contact pixels with a 4-neighbour outside the frame or outside the contact            */
#define VISTAF_SHAPE_FOOTPRINT_CX 2          /* unweighted centroid of the contact pixels (crop coordinates); NaN if n == 0            */
#define VISTAF_SHAPE_FOOTPRINT_CY 3
#define VISTAF_SHAPE_MAJOR_AXIS_MM 4         /* full axes of the ellipse with the footprint's second moments                          */
#define VISTAF_SHAPE_MINOR_AXIS_MM 5
#define VISTAF_SHAPE_ORIENTATION_RAD 6       /* direction of the major axis, (-pi/2, pi/2]; 0 for an isotropic footprint               */
#define VISTAF_SHAPE_FIT_PIXELS 7            /* m                                                                                     */
#define VISTAF_SHAPE_FIT_STATUS 8            /* VISTAF_SHAPEFIT_*                                                                     */
#define VISTAF_SHAPE_APEX_X 9                /* stationary point of the fitted quadric (crop px) ...                                  */
#define VISTAF_SHAPE_APEX_Y 10
#define VISTAF_SHAPE_APEX_DEPTH_MM 11        /* ... and its value there; 9..11 NaN unless status 0                                    */
#define VISTAF_SHAPE_CURVATURE_1_PER_MM 12   /* eigenvalues of the Hessian, |1| >= |2|, negative for a cap; status 0 and 2            */
#define VISTAF_SHAPE_CURVATURE_2_PER_MM 13
#define VISTAF_SHAPE_CURVATURE_AXIS_RAD 14   /* direction of curvature_1's eigenvector, (-pi/2, pi/2]                                  */
#define VISTAF_SHAPE_RADIUS_1_MM 15          /* -1/curvature: the sphere or cylinder that would leave that cap; NaN unless status 0   */
#define VISTAF_SHAPE_RADIUS_2_MM 16
#define VISTAF_SHAPE_FIT_RMS_MM 17           /* root mean square residual over the fit pixels; status 0 and 2                         */
                                             /* 18..23 reserved (NaN) */

#define VISTAF_SHAPEFIT_OK 0                 /* a cap: apex, curvatures, radii and rms are given                                      */
#define VISTAF_SHAPEFIT_NONE 1               /* fewer than 6 fit pixels, or they do not determine a quadric                           */
#define VISTAF_SHAPEFIT_NOT_A_CAP 2          /* fitted, but the Hessian is not negative definite (a saddle, a bowl, a ridge)          */

typedef struct vistaf_shape_handle vistaf_shape_handle;

/* A shape read-out for h x w planes, at most max_batch frames per call, tables of max_contacts rows (1..VISTAF_MAX_CONTACTS = 64: the K of
 * the vistaf_ftp_contacts call that feeds it), fit_min_fraction in [0, 1).  Everything a call needs exists after create (the one kernel
 * of a call needs no workspace on the device).  VISTAF_E_INVALID for a NULL `out` or arguments outside these ranges. */
int vistaf_shape_create(int h, int w, int max_batch, int max_contacts, double fit_min_fraction, vistaf_shape_handle **out);

/* Measure every contact of `batch` frames.  Inputs (device): d_depth_mm [B,h,w] float32 (the height map of a predict), d_contact_index
 * [B,h,w] int8, d_contacts [B, max_contacts, VISTAF_NCONTACT] double and d_count [B] int32 as vistaf_ftp_contacts wrote them with the same
 * max_contacts, d_mm_per_px [B] double.  Output (device): d_shapes [B, max_contacts, VISTAF_NSHAPE] double.  Asynchronous on `stream`;
 * one launch, allocates nothing.  VISTAF_E_INVALID for a NULL argument, `batch` outside 1..max_batch or a depth_eps_mm that is not finite,
 * VISTAF_E_HIP for a runtime failure. */
int vistaf_shape_measure(vistaf_shape_handle *sh, const float *d_depth_mm, const int8_t *d_contact_index, const double *d_contacts,
                         const int32_t *d_count, const double *d_mm_per_px, float depth_eps_mm, int batch, double *d_shapes, void *stream);

void vistaf_shape_destroy(vistaf_shape_handle *sh);

#ifdef __cplusplus
}
#endif
#endif /* VISTAF_SHAPE_H */
