/* vistaf_match.h -- C ABI of the indenter match read-out, part of libvistaf_ftp.so.
 *
 * An extension with no counterpart in the reference.  The other per-contact read-outs describe a touch; this one recognises it: the caller
 * supplies T depth imprints of known indenters (metric height maps, each with a class id and a rotational symmetry order) and for every row of
 * the per-contact table the read-out says which of them touches, how it is turned and where it sits, with the normalised correlation score, the
 * best score of another class, the amplitude and residual of the fit, and a label that is withheld when the match is weak or ambiguous.  Four
 * plain functions and no handle: the caller builds the bank on the host, moves its bytes to the device and hands in the workspace.  It reads the
 * depth plane of a predict and the int8 index plane, table and counts vistaf_ftp_contacts wrote.  It lives in include_ext/ because it is not
 * part of the drop-in boundary the headers of include/ pin; its ctypes signatures are `_lib.MATCH_SIGNATURES`.
 *
 * THE DEFINITION.  T templates of P x P float32 mm (P odd), R rotation steps, K = max_contacts, m = max_shift.  float64 throughout unless said
 * otherwise, every operation a single IEEE operation in the order written, no fused multiply-add outside the matrix-core product of step 4.
 *   1. BANK (host, once).  c = (P-1)/2.  The DISC is the offsets (dx, dy), |dx|, |dy| <= c, with dx*dx + dy*dy <= c*c, in row-major order (dy
 *      outer); D their number.  Template t is searched over R_t rotations: 1 when symmetry[t] == 0 (a body of revolution), else R /
 *      symmetry[t].  The rows of the bank are ordered by t, then r = 0..R_t-1; M = sum R_t.  theta_r = 2*pi*r/R, the table entry (cos, sin)
 *      = (cos(theta_r), sin(theta_r)) with theta_r = ((2*pi)*r)/R, computed once.  Row (t, r) at disc offset j: the bilinear sample v of
 *      template t at x = (c + cos*dx) + sin*dy, y = (c - sin*dx) + cos*dy -- the template turned by +theta from x towards y -- with x0 =
 *      floor(x), fx = x - x0 (y alike), v00 = template[y0][x0], v10 = template[y0][x0+1], v01 = template[y0+1][x0], v11 = template[y0+1][x0+1],
 *      each widened, 0 outside the square, and v = (v00*(1-fx) + v10*fx)*(1-fy) + (v01*(1-fx) + v11*fx)*fy.  mu = (the sequential sum of v
 *      over the disc) / D, norm = sqrt(the sequential sum of (v-mu)*(v-mu)), the row holds (v-mu)/norm.  A row with norm == 0 or a non-finite
 *      value refuses the build, naming the template index.
 *   2. ROWS.  kk = min(max(count[b], 0), K).  A row k >= kk is all NaN, and so are its patch and its scores.  rho = template_mm_per_px /
 *      mm_per_px[b]; a mm_per_px[b] or rho that is not finite or not > 0 gives every row of the frame STATUS = NO_SCALE.  Otherwise a row whose
 *      CENTROID_X or CENTROID_Y is not finite has STATUS = NO_PIXELS.  The patch and the scores of such rows are NaN.
 *   3. METRIC PATCH.  q = c + m, S = P + 2m.  Sample (i, j), 0 <= i, j < S, lies at crop coordinates x = cx + (j-q)*rho, y = cy + (i-q)*rho,
 *      (cx, cy) the table's depth-weighted centroid, and is the bilinear sample (the expression of step 1) of the ISOLATED depth: a pixel
 *      counts as its depth when it is inside the frame, has index == k and is finite, else as 0.  It is rounded to float32 and stored in
 *      d_patches [B,K,S,S]: an output, the rotation-unnormalised, scale-normalised crop a downstream classifier would want.  Everything below
 *      reads it widened.  Flag CLIPPED: some sample's 2 x 2 footprint leaves the frame.  With rho > 1 this is point sampling of the depth
 *      plane, not an area average: a template much coarser than the sensor aliases, and prefiltering is the caller's.
 *   4. SCORES.  For a shift s = (sx, sy) in [-m, m]^2, index (sy+m)*(2m+1) + (sx+m): w_s[j] = patch[q+sy+dy_j][q+sx+dx_j].  S1 = sum w, S2 =
 *      sum w*w, var = S2 - (S1*S1)/D, nz = the number of entries with w > float32(depth_eps_mm).  The shift is VALID when nz >= min_pixels
 *      and var > 0.  g(row, s) = sum_j bank[row][j] * w_s[j] -- the [M x D] . [D x (2m+1)^2] product, on the matrix cores -- and score = g /
 *      sqrt(var).  The score volume is not stored: the workspace holds per (b, k, row) the best score over the valid shifts, ties to the
 *      smallest shift index, with its g and shift.  d_scores [B,K,T] is an output: per template the maximum over its rows, NaN without a
 *      valid shift.
 *   5. BEST.  The maximum over valid (t, r, s) wins, ties to the smallest t, then r, then sy, then sx.  No valid shift: STATUS = NO_SUPPORT.
 *   6. REFINEMENT (the neighbouring dots are recomputed, a sequential-by-lane sum, not the matrix cores).  Rotation: a-, a0, a+ the scores
 *      at rows r-1, r, r+1 modulo R_t at the best shift; delta = (0.5*(a- - a+)) / ((a- - 2*a0) + a+) when R_t >= 3 and that denominator is
 *      < 0, else 0.  ANGLE_RAD = (((r + delta)*(2*pi))/R), plus 2*pi/symmetry when negative, minus it when not below it: in [0,
 *      2*pi/symmetry); 0 for symmetry 0.  Shift: the same parabola along sx (neighbours (sx-1, sy), (sx+1, sy)) and along sy when both
 *      neighbours are inside the window and valid, else that delta is 0.  Flag BORDER_SHIFT: m > 0 and |sx| == m or |sy| == m.  X_PX = cx +
 *      (sx + delta_x)*rho, OFFSET_X_MM = (sx + delta_x)*template_mm_per_px; Y alike.
 *   7. FIT of w ~ SCALE*template + BASE at the best (row, s): SCALE = g / norm[row], BASE_MM = S1/D - SCALE*mu[row], RESID_RMS_MM =
 *      sqrt(max(var - g*g, 0)/D).
 *   8. DECISION.  SECOND_SCORE / SECOND_CLASS: the best d_scores entry among templates whose class differs from the winner's (ties to the
 *      smallest t) and that class; NaN / -1 when there is none.  MARGIN = SCORE - SECOND_SCORE.  ROT_CONTRAST = SCORE - the minimum over the
 *      winner's searched rotations of their best-over-shifts score: 0 for R_t = 1, small when the rotation is unobservable.  Flag WEAK: SCORE <
 *      accept_score.  Flag AMBIGUOUS: MARGIN < accept_margin.  LABEL = the winner's class when neither is set, else -1.
 *   9. STATUS other than OK: every field but STATUS is NaN, except VALID_SHIFTS = 0 for NO_SUPPORT (whose patch is written).
 *  10. DETERMINISM.  No atomics, no memset.  Every sum is formed in an order fixed by the bank and the launch geometry: two calls give the same
 *      bits, and a frame gives the same bits alone or in any batch.
 *
 * THE BANK, as vistaf_match_build_bank writes it (all offsets from its first byte; n8(x) = x rounded up to a multiple of 8, n256 to 256):
 *   header   int32 [16] at 0: [0] VISTAF_MATCH_MAGIC, [1] T, [2] P, [3] R, [4] M, [5] D, [6] Dp = D rounded up to a multiple of 4, [7] 0,
 *            [8..9] the bits of the double template_mm_per_px, [10..15] 0
 *   cossin   double [R][2] at 64
 *   rowtab   int32 [M][2] (t, r), behind it
 *   klass    int32 [T], symmetry int32 [T], then padding to a multiple of 8
 *   disc     int32 [D][2] (dx, dy)
 *   mu       double [M], norm double [M]
 *   rows     double [M][Dp] at the next multiple of 256, the padding of every row zero
 * vistaf_match_measure takes the header by value (h_bank_header, the 16 int32 in HOST memory) and never reads anything back from the device; it
 * holds the header against bank_bytes.
 *
 * Every function returns 0 or a negative VISTAF_E_* code (vistaf_ftp.h); vistaf_ftp_last_error() holds the message.
 */
#ifndef VISTAF_MATCH_H
#define VISTAF_MATCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* per-contact record: d_matches[(b*max_contacts + k)*VISTAF_NMATCH + i] (double), row k = row k of frame b's contacts table */
#define VISTAF_NMATCH 24
#define VISTAF_MATCH_STATUS 0                 /* VISTAF_MATCHST_*                                                            */
#define VISTAF_MATCH_FLAGS 1                  /* bits VISTAF_MATCHFL_*                                                       */
#define VISTAF_MATCH_LABEL 2                  /* the winner's class, -1 when WEAK or AMBIGUOUS                               */
#define VISTAF_MATCH_TEMPLATE 3
#define VISTAF_MATCH_CLASS 4
#define VISTAF_MATCH_ROTATION 5               /* r of the best row, 0..R_t-1                                                 */
#define VISTAF_MATCH_SHIFT_X 6
#define VISTAF_MATCH_SHIFT_Y 7
#define VISTAF_MATCH_SCORE 8
#define VISTAF_MATCH_ANGLE_RAD 9
#define VISTAF_MATCH_X_PX 10
#define VISTAF_MATCH_Y_PX 11
#define VISTAF_MATCH_OFFSET_X_MM 12
#define VISTAF_MATCH_OFFSET_Y_MM 13
#define VISTAF_MATCH_SECOND_CLASS 14
#define VISTAF_MATCH_SECOND_SCORE 15
#define VISTAF_MATCH_MARGIN 16
#define VISTAF_MATCH_ROT_CONTRAST 17
#define VISTAF_MATCH_SCALE 18
#define VISTAF_MATCH_BASE_MM 19
#define VISTAF_MATCH_RESID_RMS_MM 20
#define VISTAF_MATCH_SUPPORT_PIXELS 21        /* nz at the best shift                                                        */
#define VISTAF_MATCH_VALID_SHIFTS 22
                                              /* 23 reserved (NaN) */
#define VISTAF_MATCHST_OK 0
#define VISTAF_MATCHST_NO_PIXELS 1
#define VISTAF_MATCHST_NO_SCALE 2
#define VISTAF_MATCHST_NO_SUPPORT 3

#define VISTAF_MATCHFL_CLIPPED 1
#define VISTAF_MATCHFL_BORDER_SHIFT 2
#define VISTAF_MATCHFL_WEAK 4
#define VISTAF_MATCHFL_AMBIGUOUS 8

#define VISTAF_MATCH_MAGIC 0x31424d56         /* "VMB1" */
#define VISTAF_MATCH_HEADER_INTS 16
#define VISTAF_MATCH_MIN_P 5
#define VISTAF_MATCH_MAX_P 33
#define VISTAF_MATCH_MAX_R 64
#define VISTAF_MATCH_MAX_T 64
#define VISTAF_MATCH_MAX_SYMMETRY 8
#define VISTAF_MATCH_MAX_SHIFT 8
#define VISTAF_MATCH_MAX_ROWS 2048

/* The bytes of a bank of T templates of P x P searched over R rotation steps with the symmetry orders symmetry[0..T): T in 1..64, P odd in
 * 5..33, R in 1..64, symmetry[t] in 0..8 with R % symmetry[t] == 0 when it is not 0, M = sum R_t <= 2048.  Makes no HIP call.
 * VISTAF_E_INVALID, with the argument's name in the message, for a NULL pointer or a value outside these ranges. */
int vistaf_match_bank_bytes(int T, int P, int R, const int32_t *symmetry, size_t *bytes);

/* Build the bank (THE BANK above) into HOST memory h_bank (8-byte aligned) of bank_bytes = what the function above gives: templates [T,P,P]
 * float32 mm (host), klass [T] >= 0, symmetry [T], template_mm_per_px finite and > 0.  Makes no HIP call; the caller moves the bytes to the
 * device.  VISTAF_E_INVALID as above, for a bank_bytes that differs, and for a template whose rotated row is flat (norm == 0) or not finite:
 * "templates[<t>] ...". */
int vistaf_match_build_bank(const float *templates, const int32_t *klass, const int32_t *symmetry, int T, int P, int R, double template_mm_per_px,
                            void *h_bank, size_t bank_bytes);

/* The bytes of the workspace vistaf_match_measure needs for up to max_batch frames of h x w, tables of max_contacts rows, a bank of M rows
 * of P x P templates and shifts up to max_shift: h, w >= 1 with h*w < 2^31, max_batch in 1..2^19, max_contacts in 1..64, P odd in 5..33,
 * max_shift in 0..8, M in 1..2048.  Makes no HIP call.  VISTAF_E_INVALID with the argument's name otherwise. */
int vistaf_match_workspace_bytes(int h, int w, int max_batch, int max_contacts, int P, int max_shift, int M, size_t *bytes);

/* Match every contact of `batch` frames.  Inputs (device): d_depth_mm [B,h,w] float, the height map of the predict; d_contact_index [B,h,w]
 * int8, d_contacts [B, max_contacts, VISTAF_NCONTACT] double and d_count [B] int32 as vistaf_ftp_contacts wrote them with the same
 * max_contacts; d_mm_per_px [B] double; d_bank, 8-byte aligned, the bank_bytes bytes vistaf_match_build_bank wrote.  h_bank_header (HOST): the
 * first VISTAF_MATCH_HEADER_INTS int32 of that bank; it is checked (magic, ranges, M <= T*R, D, and that these sizes give bank_bytes) and nothing
 * is read back from the device.  That the header is the one of the bank at d_bank -- that its M is the sum of R_t over the symmetry table
 * there -- is the caller's to keep: a header of another bank of the same size is not detected and gives wrong rows.  Parameters: depth_eps_mm finite; max_shift in 0..8; min_pixels >= 1; accept_score and accept_margin finite.
 * Outputs (device): d_matches [B, max_contacts, VISTAF_NMATCH] double, d_scores [B, max_contacts, T] double and d_patches [B, max_contacts, S,
 * S] float, S = P + 2*max_shift.  d_workspace: device memory, 256-byte aligned, of at least the bytes the function above gives for `batch`
 * frames; its contents need not be kept between calls.  Asynchronous on `stream`, three launches: no host read-back, no allocation, no
 * memset, no atomics.  Every argument is checked before any HIP call: VISTAF_E_INVALID, with the argument's name in the message, for a NULL
 * or out-of-range argument, a misaligned pointer, a header that does not fit bank_bytes or a workspace smaller than required; VISTAF_E_HIP for
 * a runtime failure. */
int vistaf_match_measure(const float *d_depth_mm, const int8_t *d_contact_index, const double *d_contacts, const int32_t *d_count,
                         const double *d_mm_per_px, const void *d_bank, size_t bank_bytes, const int32_t *h_bank_header, float depth_eps_mm,
                         int max_shift, int min_pixels, double accept_score, double accept_margin, int h, int w, int batch, int max_contacts,
                         double *d_matches, double *d_scores, float *d_patches, void *d_workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VISTAF_MATCH_H */
