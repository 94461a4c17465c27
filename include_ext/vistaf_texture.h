/* vistaf_texture.h -- C ABI of the surface texture read-out, part of libvistaf_ftp.so.
 *
 * An extension with no counterpart in the reference.  The other per-contact read-outs describe a touch as a body (vistaf_shape.h fits the cap
 * and keeps only the rms of what is left); this one describes the surface of what is touching: the fine structure left once the form is taken
 * away -- its roughness (ISO 25178-2 height and slope parameters about the form), whether it is directional and which way the ridges run, and
 * the pitch of a periodic surface, from a masked autocorrelation of the residual over a window of lags.  Two plain functions and no handle:
 * the caller hands in the workspace.  It reads the depth plane of a predict and the int8 index plane, table and counts vistaf_ftp_contacts
 * wrote.  It lives in include_ext/ because it is not part of the drop-in boundary the headers of include/ pin; its ctypes signatures are
 * `_lib.TEXTURE_SIGNATURES`.
 *
 * THE DEFINITION for frame b, row k of a table of K = max_contacts rows; s = mm_per_px[b], L = max_lag, f = eval_min_fraction.  float64
 * throughout unless said otherwise, every operation a single IEEE operation in the order written, no fused multiply-add but in step 6.
 *   0. ROWS.  kk = min(max(count[b], 0), K).  A row k >= kk is all NaN and its ACF window is all NaN.  Plane values outside 0..kk-1 count as
 *      -1, a NaN depth counts as 0.  The box is the table's BBOX_X0..Y1 clipped to the frame (csrc/contact_rows.hpp: ContactBox); a box that
 *      is not finite, or empty after clipping, holds no pixel.
 *   1. EVALUATION PIXELS: the pixels of the box with index == k, depth > float32(depth_eps_mm) and, unless f == 0, depth >=
 *      float32(f * MAX_DEPTH_MM of the table's row) -- the fit pixels of vistaf_shape.h: the rim of a contact is the skin bridging, not the
 *      object.  m = their number (EVAL_PIXELS).
 *   2. FORM: the least-squares polynomial of degree form_degree over the evaluation pixels, basis 1 (degree 0; N = 1), 1, u, v (degree 1;
 *      N = 3) or 1, u, v, u*u, u*v, v*v (degree 2; N = 6) in the coordinates u, v of vistaf_shape.h step 5 (the table's own box, centred and
 *      scaled by its half sizes of at least 1).  Normal equations A c = rhs from the sums of vistaf_shape.h step 5, accumulated in the order
 *      of step 9; the verdict is chol_solve<N> of A - 2^-32 diag(A), the solution chol_solve<N> of A (csrc/form_fit.hpp, the copy the shape
 *      read-out uses).  FORM_STATUS = 1 (no form) when m < max(N, 6), when either factorisation fails or when a coefficient is not finite (an
 *      infinite depth among the pixels): every field but EVAL_PIXELS and FORM_STATUS is then NaN and the row's evaluation pixels are NaN in
 *      the residual plane.  FORM_C0..C5 are the coefficients, 0 for the terms above the degree.
 *   3. RESIDUAL: r = float32(double(depth) - P(u, v)), P = c0 + c1*u + c2*v + c3*(u*u) + c4*(u*v) + c5*(v*v) summed left to right, stored in
 *      d_residual_mm at the evaluation pixel.  Every other element of the plane is NaN; every element is written exactly once per call.
 *      Everything below reads this float32 plane, each r widened to float64.
 *   4. HEIGHT PARAMETERS, sums over the evaluation pixels: SA_MM = sum|r| / m, SQ_MM = sqrt(sum r*r / m), SSK = (sum (r*r)*r / m) /
 *      (SQ*SQ*SQ), SKU = (sum (r*r)*(r*r) / m) / ((SQ*SQ)*(SQ*SQ)), SP_MM = max r, SV_MM = -min r, SZ_MM = SP + SV; SP_PIXEL, SV_PIXEL the flat
 *      index y*w + x of the first extreme in row-major order.  sum r*r == 0: FORM_STATUS = 2 (flat), SA = SQ = SP = SV = SZ = 0 with their
 *      pixels, SSK, SKU and every later field NaN.
 *   5. SLOPE PARAMETERS.  A gradient pixel is an evaluation pixel whose four 4-neighbours are inside the frame and evaluation pixels of k;
 *      g = their number (GRAD_PIXELS).  rx = (r(x+1,y) - r(x-1,y)) / (2*s), ry = (r(x,y+1) - r(x,y-1)) / (2*s); Jxx = sum rx*rx, Jyy = sum
 *      ry*ry, Jxy = sum rx*ry.  SDQ = sqrt((Jxx + Jyy) / g), SDR = sum(sqrt((1 + rx*rx) + ry*ry) - 1) / g.  Dominant gradient direction
 *      without trigonometry: hd = (Jxx - Jyy)/2, rad = sqrt(hd*hd + Jxy*Jxy), e = (hd + rad, Jxy) when hd >= 0, else (Jxy, rad - hd);
 *      (GRAD_DIR_X, GRAD_DIR_Y) = e / sqrt(ex*ex + ey*ey), negated when X < 0, or X == 0 and Y < 0; (1, 0) when e == (0, 0).  The lay of the
 *      surface is perpendicular to it.  COHERENCE = rad / ((Jxx + Jyy)/2): 1 for ridges, 0 for an isotropic surface.  g == 0 leaves SDQ,
 *      SDR, the direction and COHERENCE NaN.
 *   6. AUTOCORRELATION.  For a lag t = (dx, dy), |dx|, |dy| <= L: N(t) = the number of pixels p with p and p + t both evaluation pixels of
 *      k, C(t) = sum over them of r(p) * r(p+t) (the product of two widened float32 values is exact in float64, so the fused multiply-add
 *      the kernel uses gives the bits of a multiplication and an addition).  N and C are computed for the half plane dy > 0, or dy == 0 and
 *      dx >= 0, and mirrored: N(-t) = N(t), C(-t) = C(t).  A lag is VALID when N(t) >= max(16, m / 8) (integer division).
 *      A(t) = (C(t) / double(N(t))) / (C(0) / double(m)) for a valid lag, NaN otherwise.  The window goes to d_acf, entry [dy+L][dx+L];
 *      ACF_VALID_LAGS counts the valid lags of the full window.  When t = 0 is not valid (m < 16) no lag is, and every later field is NaN.
 *   7. CENTRAL LOBE: the 4-connected set of valid lags with A > acf_threshold that contains t = 0; LOBE_LAGS its size.  The RING is the valid
 *      lags outside the lobe that are 4-adjacent to it.  LOBE_STATUS = 1 (open) when the lobe touches the window border or is 4-adjacent to
 *      an invalid lag, else 0.  |t| = sqrt(double(dx*dx + dy*dy)).  SAL_MM = s * min |t| over the ring, SAL_LAG_X, SAL_LAG_Y the lag that
 *      attains it within the half plane of step 6, ties to the smallest (dy, dx); RMAX_MM = s * max |t| over the ring; STR = SAL_MM /
 *      RMAX_MM, the texture aspect ratio (with an open lobe an upper bound, which the status says).  An empty ring leaves these five NaN.
 *   8. PITCH along the dominant gradient (GX, GY) = (GRAD_DIR_X, GRAD_DIR_Y): a(0) = 1 and a(j) = A(floor(j*GX + 0.5), floor(j*GY + 0.5)) for
 *      j = 1..L, the profile stopping before the first invalid lag (at once when the direction is NaN); PROFILE_SAMPLES = the number of its
 *      samples, a(0) included.  The peak is the smallest j in 2..L-1 with a(j+1) in the profile, a(j-1) < a(j) >= a(j+1), a(j) >= peak_min
 *      and some a(i) <= acf_threshold, 1 <= i < j.  PITCH_MM = s * (j + 0.5*(a(j-1) - a(j+1)) / (a(j-1) - 2*a(j) + a(j+1))), PITCH_ACF =
 *      a(j).  No peak leaves both NaN.
 *   9. DETERMINISM.  No float atomics, no memset.  Every float64 sum is formed in an order fixed by the box and the launch geometry (pixel
 *      -> lane -> wave -> workgroup; for step 6 the pixels of a box row in x order, the box rows dealt to the waves of a workgroup in turn):
 *      two calls give the same bits, and a frame gives the same bits alone or in any batch.
 *
 * Every function returns 0 or a negative VISTAF_E_* code (vistaf_ftp.h); vistaf_ftp_last_error() holds the message.
 */
#ifndef VISTAF_TEXTURE_H
#define VISTAF_TEXTURE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* per-contact record: d_textures[(b*max_contacts + k)*VISTAF_NTEXTURE + i] (double), row k = row k of frame b's contacts table */
#define VISTAF_NTEXTURE 40
#define VISTAF_TEXTURE_EVAL_PIXELS 0
#define VISTAF_TEXTURE_FORM_STATUS 1          /* VISTAF_TEXTUREFORM_*                                                       */
#define VISTAF_TEXTURE_FORM_C0 2              /* .. FORM_C5 = 7                                                             */
#define VISTAF_TEXTURE_FORM_C1 3
#define VISTAF_TEXTURE_FORM_C2 4
#define VISTAF_TEXTURE_FORM_C3 5
#define VISTAF_TEXTURE_FORM_C4 6
#define VISTAF_TEXTURE_FORM_C5 7
#define VISTAF_TEXTURE_SA_MM 8
#define VISTAF_TEXTURE_SQ_MM 9
#define VISTAF_TEXTURE_SSK 10
#define VISTAF_TEXTURE_SKU 11
#define VISTAF_TEXTURE_SP_MM 12
#define VISTAF_TEXTURE_SV_MM 13
#define VISTAF_TEXTURE_SZ_MM 14
#define VISTAF_TEXTURE_SP_PIXEL 15
#define VISTAF_TEXTURE_SV_PIXEL 16
#define VISTAF_TEXTURE_GRAD_PIXELS 17
#define VISTAF_TEXTURE_SDQ 18
#define VISTAF_TEXTURE_SDR 19
#define VISTAF_TEXTURE_GRAD_DIR_X 20
#define VISTAF_TEXTURE_GRAD_DIR_Y 21
#define VISTAF_TEXTURE_COHERENCE 22
#define VISTAF_TEXTURE_ACF_VALID_LAGS 23
#define VISTAF_TEXTURE_LOBE_LAGS 24
#define VISTAF_TEXTURE_LOBE_STATUS 25         /* 0: closed, 1: open                                                         */
#define VISTAF_TEXTURE_SAL_MM 26
#define VISTAF_TEXTURE_SAL_LAG_X 27
#define VISTAF_TEXTURE_SAL_LAG_Y 28
#define VISTAF_TEXTURE_RMAX_MM 29
#define VISTAF_TEXTURE_STR 30
#define VISTAF_TEXTURE_PITCH_MM 31
#define VISTAF_TEXTURE_PITCH_ACF 32
#define VISTAF_TEXTURE_PROFILE_SAMPLES 33
                                              /* 34..39 reserved (NaN) */
#define VISTAF_TEXTUREFORM_OK 0
#define VISTAF_TEXTUREFORM_NONE 1
#define VISTAF_TEXTUREFORM_FLAT 2

#define VISTAF_TEXTURE_MIN_LAG 2
#define VISTAF_TEXTURE_MAX_LAG 31             /* a window row of 2L+1 lags fits a 64-bit mask and one lag column maps to one lane of a wave */

/* The bytes of the workspace vistaf_texture_measure needs for up to max_batch frames of h x w, tables of max_contacts rows and windows of
 * max_lag: h, w >= 1 with h*w < 2^31, max_batch in 1..2^19, max_contacts in 1..VISTAF_MAX_CONTACTS = 64, max_lag in 2..31.  Makes no HIP
 * call.  VISTAF_E_INVALID, with the argument's name in the message, for a NULL `bytes` or a size outside these ranges. */
int vistaf_texture_workspace_bytes(int h, int w, int max_batch, int max_contacts, int max_lag, size_t *bytes);

/* Measure every contact of `batch` frames.  Inputs (device): d_depth_mm [B,h,w] float, the height map of the predict; d_contact_index
 * [B,h,w] int8, d_contacts [B, max_contacts, VISTAF_NCONTACT] double and d_count [B] int32 as vistaf_ftp_contacts wrote them with the same
 * max_contacts; d_mm_per_px [B] double.  Parameters: depth_eps_mm finite; eval_min_fraction in [0, 1); form_degree 0, 1 or 2; max_lag in
 * 2..31; acf_threshold and peak_min in (0, 1).  Outputs (device): d_textures [B, max_contacts, VISTAF_NTEXTURE] double, d_residual_mm
 * [B,h,w] float (the form-removed depth, NaN where no residual is defined) and d_acf [B, max_contacts, 2L+1, 2L+1] double (the normalised
 * autocorrelation, entry [dy+L][dx+L], NaN = invalid lag).  d_workspace: device memory, 256-byte aligned, of at least the bytes the function
 * above gives for `batch` frames (so any batch up to the max_batch it was sized for); its contents need not be kept between calls.
 * Asynchronous on `stream`: no host read-back, no allocation, no memset, no atomics.  Every argument is checked before any HIP call:
 * VISTAF_E_INVALID, with the argument's name in the message, for a NULL or out-of-range argument, a misaligned pointer or a workspace
 * smaller than required; VISTAF_E_HIP for a runtime failure. */
int vistaf_texture_measure(const float *d_depth_mm, const int8_t *d_contact_index, const double *d_contacts, const int32_t *d_count,
                           const double *d_mm_per_px, float depth_eps_mm, double eval_min_fraction, int form_degree, int max_lag,
                           double acf_threshold, double peak_min, int h, int w, int batch, int max_contacts, double *d_textures,
                           float *d_residual_mm, double *d_acf, void *d_workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VISTAF_TEXTURE_H */
