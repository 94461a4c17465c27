/* vistaf_pressure.h -- C ABI of the pressure read-out, part of libvistaf_ftp.so.
 *
 * An extension with no counterpart in the reference: the library reports force as one scalar per frame, and the only way that force is
 * spread over the skin is the taxel read-out's Winkler share (vistaf_taxel.h), pressure proportional to indentation.  This gives the
 * contact pressure map that linear elasticity assigns to the depth plane: the normal traction that holds the surface of an elastic layer
 * (Young's modulus E, Poisson's ratio nu, thickness t, bonded to a rigid base; t = +inf: a half-space) in the shape u.  In the Fourier
 * domain that is one multiplication, p^ = G(|k|) u^, with G in closed form; between its limits G is the Winkler foundation (thin layer)
 * and the Boussinesq half-space (thick layer).  E, nu and t are the caller's: the repository holds no material data.  It is an object of
 * its own: it never touches another handle and reads only what it is handed, the depth planes, scales, forces and status of a predict and
 * the index planes, tables and counts vistaf_ftp_contacts wrote for them.
 *
 * THE DEFINITION for frame b of h x w; s = mm_per_px[b], eps = depth_eps_mm, F = frame_force_N[b].  Float64 throughout.
 *   0. U is the float32 depth plane with non-finite values and values <= float32(eps) replaced by 0, widened to float64.  The transform
 *      size is Ph = h + pad_px, Pw = w + pad_px, zero fill; Wh = Pw/2 + 1 (integer division).
 *   1. U^[a][c] = sum_y sum_x U[y][x] exp(-2 pi i (a y / Ph + c x / Pw)),  a = 0..Ph-1, c = 0..Wh-1.
 *   2. fy = (a <= Ph/2 ? a : a - Ph) / Ph,  fx = c / Pw,  q = 2 pi sqrt(fx*fx + fy*fy) / s  (rad/mm);  Es = E / (1 - nu*nu),  k = 3 - 4 nu.
 *        half-space:  G = Es q / 2 (G(0) = 0: the mean pressure is indeterminate, the plane has the mean the padded transform gives it, 0);
 *        layer:       x = q t,  e = exp(-2x),
 *                     S = (k (1 - e*e) - 4 x e) / (k (1 + e*e) + (4 x*x + 10 - 24 nu + 16 nu*nu) e),   G = Es q / (2 S),
 *                     and at q = 0  G = E (1 - nu) / ((1 + nu) (1 - 2 nu) t), the oedometric (Winkler) modulus over t.
 *      S is ((3-4nu) sinh 2x - 2x) / ((3-4nu) cosh 2x + 2x^2 + 5 - 12nu + 8nu^2) without the overflow; S = 1 to double precision for x >= 19.
 *   3. p[y][x] = 1000 / (Ph Pw) * Re sum_a sum_c' G U^ exp(+2 pi i (a y / Ph + c' x / Pw)) over the full spectrum c' = 0..Pw-1, for y < h,
 *      x < w only.  The half that is not stored comes from Hermitian symmetry: weight 2 for 0 < c < Pw/2 (and for c = (Pw-1)/2 of an odd
 *      Pw), weight 1 for c = 0 and for the Nyquist column c = Pw/2 of an even Pw.  kPa (E in MPa, depth in mm), stored as float32.
 *      A frame whose status is not VISTAF_FRAME_OK has a plane of zeros; nothing of its depth, scale or force is interpreted.
 *   4. THE TABLES are functions of the float32 plane as stored, p widened to float64, and (when given) of the int8 index plane, the table
 *      and the count of vistaf_ftp_contacts: kk = min(max(count[b], 0), K), K = max_contacts.  THE PIXELS of row k < kk are the pixels of
 *      its box (BBOX_X0..Y1 of the row, clipped to the frame; a box that is not finite or empty holds none) with index == k; n their
 *      number.  p+ = max(p, 0), p- = max(-p, 0), px = s*s.  Over the pixels of the row: Pp = sum p+, Pn = sum p-, Xp = sum x p+, Yp = sum y p+
 *      (exact products), Sx = sum x, Sy = sum y (integers), Pe = sum of p+ over the EDGE pixels, those with a 4-neighbour that is outside
 *      the frame or not a pixel of the row.  The contact row, VISTAF_NPRESSURE doubles:
 *        PIXELS           n
 *        FORCE_MODEL_N    1e-3 * px * Pp           the load the model puts on the contact, with the caller's E
 *        TENSILE_MODEL_N  1e-3 * px * Pn           the pull the model needs there (the clamped depth map is not an equilibrium shape)
 *        FORCE_N          F * (FORCE_MODEL_N / the frame's FORCE_MODEL_N); 0 when that is 0; NaN without d_frame_force_N
 *        MEAN_KPA         (Pp - Pn) / n
 *        PEAK_KPA         the largest p, PEAK_INDEX the row-major index of the first pixel that attains it
 *        COP_X, COP_Y     Xp / Pp, Yp / Pp: the centre of pressure
 *        OFFSET_X_MM, OFFSET_Y_MM   (COP_X - Sx/n) * s, (COP_Y - Sy/n) * s: centre of pressure minus footprint centroid
 *        PEAK_OVER_MEAN   PEAK_KPA / MEAN_KPA when MEAN_KPA > 0
 *        EDGE_SHARE       Pe / Pp: a flat punch loads its rim, a ball its middle
 *      Fields whose divisor is 0 (n for the means, Pp for the shares and centres) are NaN; a row k >= kk is all NaN.
 *      The frame row, VISTAF_NPRESSUREFRAME doubles:
 *        CONTACTS         kk (0 without the contact inputs)
 *        FORCE_MODEL_N    the rows' FORCE_MODEL_N added in ascending row order
 *        TENSILE_MODEL_N  1e-3 * px * sum of p- over the whole plane
 *        OUTSIDE_MODEL_N  1e-3 * px * sum of |p| over the pixels of no row (index outside 0..kk-1; every pixel without the contact inputs)
 *        SCALE            F / FORCE_MODEL_N when that is > 0, else NaN: what the calibrated force says about the caller's modulus ...
 *        E_EFFECTIVE_MPA  ... SCALE * E, the modulus under which the model carries exactly F
 *        PEAK_KPA, PEAK_INDEX   over the whole plane, first pixel;  PEAK_ROW the row that pixel belongs to, -1 when it belongs to none
 *        COP_X, COP_Y     (sum_k Xp) / (sum_k Pp), (sum_k Yp) / (sum_k Pp), ascending rows; NaN when the divisor is 0
 *        STATUS           status[b] (0 without d_status)
 *      The rows of a frame whose status is not VISTAF_FRAME_OK are NaN except STATUS.
 *   5. Every float64 sum is formed in an order fixed by the frame and the launch geometry alone (k-step by k-step in the contractions;
 *      pixel -> lane -> wave -> workgroup in the tables), without float atomics: a frame gives the same bits alone, in any position of a
 *      batch and on a second call.
 *
 * Every function returns 0 or a negative VISTAF_E_* code (vistaf_ftp.h); vistaf_ftp_last_error() holds the message.
 */
#ifndef VISTAF_PRESSURE_H
#define VISTAF_PRESSURE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* per-contact record: d_rows[(b*max_contacts + k)*VISTAF_NPRESSURE + i] (double), row k = row k of frame b's contacts table */
#define VISTAF_NPRESSURE 16
#define VISTAF_PRESSURE_PIXELS 0
#define VISTAF_PRESSURE_FORCE_MODEL_N 1
#define VISTAF_PRESSURE_TENSILE_MODEL_N 2
#define VISTAF_PRESSURE_FORCE_N 3
#define VISTAF_PRESSURE_MEAN_KPA 4
#define VISTAF_PRESSURE_PEAK_KPA 5
#define VISTAF_PRESSURE_PEAK_INDEX 6
#define VISTAF_PRESSURE_COP_X 7
#define VISTAF_PRESSURE_COP_Y 8
#define VISTAF_PRESSURE_OFFSET_X_MM 9
#define VISTAF_PRESSURE_OFFSET_Y_MM 10
#define VISTAF_PRESSURE_PEAK_OVER_MEAN 11
#define VISTAF_PRESSURE_EDGE_SHARE 12
                                             /* 13..15 reserved (NaN) */

/* per-frame record: d_frame[b*VISTAF_NPRESSUREFRAME + i] (double) */
#define VISTAF_NPRESSUREFRAME 12
#define VISTAF_PRESSUREFRAME_CONTACTS 0
#define VISTAF_PRESSUREFRAME_FORCE_MODEL_N 1
#define VISTAF_PRESSUREFRAME_TENSILE_MODEL_N 2
#define VISTAF_PRESSUREFRAME_OUTSIDE_MODEL_N 3
#define VISTAF_PRESSUREFRAME_SCALE 4
#define VISTAF_PRESSUREFRAME_E_EFFECTIVE_MPA 5
#define VISTAF_PRESSUREFRAME_PEAK_KPA 6
#define VISTAF_PRESSUREFRAME_PEAK_INDEX 7
#define VISTAF_PRESSUREFRAME_PEAK_ROW 8
#define VISTAF_PRESSUREFRAME_COP_X 9
#define VISTAF_PRESSUREFRAME_COP_Y 10
#define VISTAF_PRESSUREFRAME_STATUS 11

typedef struct vistaf_pressure_handle vistaf_pressure_handle;

/* A pressure read-out for h x w planes (1..4096 each way), at most max_batch (1..65535) frames per call, tables of max_contacts rows
 * (0..VISTAF_MAX_CONTACTS = 64; 0: the plane and the frame row only), pad_px in 0..4096, E_mpa > 0 and finite, 0 <= nu <= 0.49,
 * thickness_mm > 0 or +inf.  Makes no call of the runtime: the twiddle tables are built here, on the host, and go to the device current
 * at the first measure together with the workspace.  VISTAF_E_INVALID for a NULL `out` or arguments outside these ranges. */
int vistaf_pressure_create(int h, int w, int max_batch, int max_contacts, int pad_px, double E_mpa, double nu, double thickness_mm,
                           vistaf_pressure_handle **out);

/* Measure `batch` frames.  Inputs (device): d_depth_mm [B,h,w] float32 (the height map of a predict); d_contact_index [B,h,w] int8,
 * d_contacts [B, max_contacts, VISTAF_NCONTACT] double and d_count [B] int32 as vistaf_ftp_contacts wrote them -- all three and d_rows NULL
 * together for the plane and the frame row only, which a handle of max_contacts 0 requires; d_mm_per_px [B] double; d_frame_force_N [B]
 * double or NULL; d_status [B] int32 or NULL (every frame OK).  Outputs (device): d_pressure_kpa [B,h,w] float32, d_rows
 * [B, max_contacts, VISTAF_NPRESSURE] double, d_frame [B, VISTAF_NPRESSUREFRAME] double.  Asynchronous on `stream`; no memset, no atomics;
 * the first call of a handle uploads the tables (synchronously) and allocates the workspace, later calls allocate nothing.  Every argument
 * is checked before the first HIP call: VISTAF_E_INVALID for a NULL handle, depth, scale, plane or frame output, contact arguments that
 * are not all given or all NULL, `batch` outside 1..max_batch, a depth_eps_mm that is not finite or a pointer that is not aligned to its
 * element; VISTAF_E_HIP for a runtime failure. */
int vistaf_pressure_measure(vistaf_pressure_handle *pr, const float *d_depth_mm, const int8_t *d_contact_index, const double *d_contacts,
                            const int32_t *d_count, const double *d_mm_per_px, const double *d_frame_force_N, const int32_t *d_status,
                            float depth_eps_mm, int batch, float *d_pressure_kpa, double *d_rows, double *d_frame, void *stream);

void vistaf_pressure_destroy(vistaf_pressure_handle *pr);

#ifdef __cplusplus
}
#endif
#endif /* VISTAF_PRESSURE_H */
