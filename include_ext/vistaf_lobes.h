/* vistaf_lobes.h -- C ABI of the lobe read-out, part of libvistaf_ftp.so.
 *
 * An extension with no counterpart in the reference.  Every other per-contact read-out is keyed on one row of the contacts table, one
 * 8-connected component of the kept mask.  On a soft skin two fingertips pressed a few millimetres apart leave ONE connected footprint with
 * two depth maxima: one row, a centroid in the valley between them, an ellipse of a body that does not exist.  This read-out looks at the
 * depth relief inside a component: it finds the maxima, measures how far each stands above the saddle that joins it to higher ground (its
 * prominence, the mountaineer's measure), keeps the ones that stand out as peaks, cuts the contact into one lobe per peak and hands back a
 * table of the lobes in the exact layout of the contacts table, so that the tracker, the shape, centreline and every other read-out can be
 * run on touches instead of footprints.  Two plain functions and no handle: the caller hands in the workspace.  It reads only what it is
 * handed.  It lives in include_ext/ because it is not part of the drop-in boundary the headers of include/ pin; its ctypes signatures are
 * `_lib.LOBES_SIGNATURES`.
 *
 * THE DEFINITION for frame b, row k of a table of K = max_contacts rows; s = mm_per_px[b]; y points down:
 *   0. ROWS AND PIXELS.  kk = min(max(count[b], 0), K).  A row k >= kk is unused.  The pixels of row k are the pixels with index == k inside
 *      the table's box (BBOX_X0..Y1) clipped to the frame; a box that is not finite, or empty after clipping, holds no pixel
 *      (csrc/contact_rows.hpp: ContactBox).  d(p) is the float32 depth sample; a sample that is not finite counts as 0.0f everywhere here.
 *   1. ORDER.  p > q ("p is greater") when d(p) > d(q), or when the depths are equal and p has the smaller row-major index: a strict total
 *      order on the pixels of k.
 *   2. ASCENT.  up(p) is the greatest of p and those of its 8 neighbours that are pixels of k; p is a maximum when up(p) = p; top(p) is the
 *      fixed point of iterating up; the basin of a maximum m is {p : top(p) = m}.  RAW_MAXIMA counts the maxima.  A flat plateau can hold
 *      several (a flat disc has two under this rule); step 5 removes them.
 *   3. PASSES.  A pass is an 8-adjacent pair (lo, hi) of pixels of k in different basins with hi > lo.  Passes are ordered by lo, then by hi.
 *   4. MERGE.  Start with one component per basin; the elder of a component is its greatest maximum.  Take the passes in descending order; a
 *      pass whose ends already lie in one component does nothing.  Otherwise the component whose elder is smaller dies: its elder m gets
 *      saddle(m) = lo, into(m) = the basin, in the other component, of that pass's end, and prominence(m) = double(d(m)) - double(d(lo));
 *      then the two components are joined.  A maximum that never dies -- the contact's greatest; on a hand-made plane whose label has
 *      several pieces, the greatest of each -- has prominence double(d(m)), no saddle and no neighbour.
 *   5. PEAKS.  tau = max(min_prominence_mm, min_prominence_frac * double(d(the contact's greatest maximum))).  A maximum is a peak when it
 *      never died or when prominence > tau.  The comparison is strict: that is what removes plateau maxima at tau = 0.
 *   6. LOBES.  lobe(m) = m for a peak, else lobe(the maximum of into(m)); the chain ends, every lobe is 8-connected and its greatest pixel
 *      is its peak (tests/test_lobes.py, on random masks).  A pixel belongs to lobe(top(p)).  Lobes are numbered by their peaks in
 *      descending order; PEAKS is their number and PEAKS_WRITTEN = min(PEAKS, max_lobes).
 *   7. d_lobes [B, K, max_lobes, VISTAF_NLOBE] double, one record per written lobe, the records behind PEAKS_WRITTEN all NaN.  Coordinates
 *      are the frame's.  SADDLE_* are NaN and NEIGHBOUR is -1 for a peak that never died (lobe 0).  NEIGHBOUR is the number of the lobe of
 *      into(peak), in the numbering of all PEAKS lobes.  CONTACT_PIXELS counts the lobe's pixels with d > float(depth_eps_mm), compared in
 *      float32 as in the contacts table; with S, SX, SY the float64 sums of d, x * d, y * d over them:
 *          AREA_MM2 = double(CONTACT_PIXELS) * (s * s)      VOLUME_CM3 = S * (s * s) / 1000.0
 *          CENTROID_X = SX / S, CENTROID_Y = SY / S         NaN without contact pixels
 *          FORCE_SHARE_N = FORCE_N of row k * S / S_all     S_all: the same sum over all pixels of the row; NaN when S_all is 0
 *      so the shares of a contact's lobes add up to its force (up to rounding).  BASINS: the raw maxima that ended in this lobe.
 *      The order of the float64 sums is the kernel's (pixel -> lane -> wave -> workgroup) and is not part of this definition: two orders of
 *      n positive terms differ by at most n * 2^-52 relative, and the tests allow 4 * n * 2^-52.
 *   8. d_rows [B, K, VISTAF_NLOBEROW] double.  THRESHOLD_MM is the tau used.  SEPARATION_MM = sqrt(double(dx^2 + dy^2)) * s between the
 *      peaks of lobes 0 and 1, NaN when PEAKS < 2.  DEEPEST_SADDLE_MM: the largest SADDLE_DEPTH_MM among all PEAKS lobes, NaN when none has
 *      a saddle.  NEXT_PROMINENCE_MM: the largest prominence among the maxima that are not peaks -- how near the contact is to splitting
 *      further -- NaN when there is none.  STATUS = VISTAF_LOBEST_OK or _NO_PIXELS, plus the flag _TRUNCATED when PEAKS > max_lobes.  A row
 *      in use without a pixel has fields 0..3 equal to 0, STATUS 1, the rest and all its lobe records NaN.  An unused row is all NaN.
 *      Nothing is raised for what the data does.
 *   9. d_lobe_index [B,h,w] int8, if given, is written whole: the lobe number on the pixels of rows in use, -2 on the pixels of lobes at or
 *      beyond max_lobes, -1 elsewhere.
 *  10. THE SPLIT TABLE.  The written lobes of all rows in use of a frame become contacts in the exact layout vistaf_ftp_contacts writes:
 *      d_split_contacts [B, K, VISTAF_NCONTACT] double, d_split_count [B] int32, d_split_index [B,h,w] int8, ordered by that table's own
 *      rule -- maximum depth descending, ties by arg-max index ascending: the order of step 1 on the peaks across the frame.  count is the
 *      number of written lobes whatever K is; the table is truncated to K, and pixels of lobes beyond K, like pixels labelled -2, are -1
 *      in the plane.  Unused rows are NaN.  Fields 0..12 have the contacts header's meanings applied to the lobe: PIXELS, CONTACT_PIXELS,
 *      AREA_MM2, VOLUME_CM3 = double(float32(S)) * (s * s) / 1000.0 (0.0 without contact pixels), MAX_DEPTH_MM and ARGMAX_INDEX of the
 *      peak, the centroid, the inclusive box of the lobe's pixels.
 *      FORCE_N holds FORCE_SHARE_N.  THIS DIFFERS FROM THE CONTACTS TABLE'S MEANING: there FORCE_N is the session's force curve evaluated at
 *      the contact's own volume, as if it were alone in the frame; here it is the parent contact's force divided among its lobes in
 *      proportion to their depth sums, so that the lobes of a contact add up to what the contacts table reports for it.
 *      d_split_parent [B, K, 2] int32 holds (parent row, lobe number) of each split row, (-1, -1) on unused rows.  A frame with
 *      count <= 0 gives split_count 0.
 *  11. DETERMINISM.  All integer work is exact, every double is a fixed expression and every sum is formed in an order the box alone fixes:
 *      a frame gives the same bits alone, in any batch position and on a second call.
 *
 * DEFAULTS.  The Python layer uses min_prominence_mm = 0.02 and min_prominence_frac = 0.10: a maximum must stand 0.02 mm, and a tenth of the
 * contact's greatest depth, above its saddle to count as a touch of its own.  They are a judgement about the noise of a smoothed depth map
 * that nobody has measured on this sensor; min_prominence_frac exists so that one setting serves light and heavy touches.
 *
 * Every function returns 0 or a negative VISTAF_E_* code (vistaf_ftp.h); vistaf_ftp_last_error() holds the message.
 */
#ifndef VISTAF_LOBES_H
#define VISTAF_LOBES_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VISTAF_LOBES_MAX 64                  /* the largest max_lobes */

/* per-lobe record: d_lobes[((b*max_contacts + k)*max_lobes + j)*VISTAF_NLOBE + i] (double), lobe j of row k of frame b */
#define VISTAF_NLOBE 16
#define VISTAF_LOBE_X 0
#define VISTAF_LOBE_Y 1
#define VISTAF_LOBE_DEPTH_MM 2
#define VISTAF_LOBE_PROMINENCE_MM 3
#define VISTAF_LOBE_SADDLE_X 4
#define VISTAF_LOBE_SADDLE_Y 5
#define VISTAF_LOBE_SADDLE_DEPTH_MM 6
#define VISTAF_LOBE_NEIGHBOUR 7
#define VISTAF_LOBE_PIXELS 8
#define VISTAF_LOBE_CONTACT_PIXELS 9
#define VISTAF_LOBE_AREA_MM2 10
#define VISTAF_LOBE_VOLUME_CM3 11
#define VISTAF_LOBE_CENTROID_X 12
#define VISTAF_LOBE_CENTROID_Y 13
#define VISTAF_LOBE_FORCE_SHARE_N 14
#define VISTAF_LOBE_BASINS 15

/* per-row record: d_rows[(b*max_contacts + k)*VISTAF_NLOBEROW + i] (double), row k = row k of frame b's contacts table */
#define VISTAF_NLOBEROW 12
#define VISTAF_LOBEROW_PIXELS 0
#define VISTAF_LOBEROW_RAW_MAXIMA 1
#define VISTAF_LOBEROW_PEAKS 2
#define VISTAF_LOBEROW_PEAKS_WRITTEN 3
#define VISTAF_LOBEROW_STATUS 4
#define VISTAF_LOBEROW_THRESHOLD_MM 5
#define VISTAF_LOBEROW_SEPARATION_MM 6
#define VISTAF_LOBEROW_DEEPEST_SADDLE_MM 7
#define VISTAF_LOBEROW_NEXT_PROMINENCE_MM 8
                                             /* 9..11 reserved (NaN) */

/* values and flags of the STATUS field */
#define VISTAF_LOBEST_OK 0
#define VISTAF_LOBEST_NO_PIXELS 1
#define VISTAF_LOBEST_TRUNCATED 16

/* The bytes of the workspace vistaf_lobes_measure needs for `batch` frames of h x w and tables of max_contacts rows: h, w in 1..32767 with
 * h*w <= 2^29 - 1, batch >= 1, max_contacts in 1..VISTAF_MAX_CONTACTS = 64.  Makes no HIP call.  VISTAF_E_INVALID, with the argument's name
 * in the message, for a NULL `bytes` or a size outside these ranges. */
int vistaf_lobes_workspace_bytes(int h, int w, int batch, int max_contacts, size_t *bytes);

/* Measure every contact of `batch` frames.  Inputs (device): d_contact_index [B,h,w] int8, d_contacts [B, max_contacts, VISTAF_NCONTACT]
 * double and d_count [B] int32 as vistaf_ftp_contacts wrote them with the same max_contacts, d_mm_per_px [B] double, d_depth_mm [B,h,w]
 * float32 (required); max_lobes in 1..VISTAF_LOBES_MAX; min_prominence_mm, min_prominence_frac and depth_eps_mm finite and >= 0.  Outputs
 * (device): d_lobes [B, max_contacts, max_lobes, VISTAF_NLOBE] double, d_rows [B, max_contacts, VISTAF_NLOBEROW] double and, unless NULL,
 * d_lobe_index [B,h,w] int8 and the split set d_split_contacts [B, max_contacts, VISTAF_NCONTACT] double, d_split_count [B] int32,
 * d_split_index [B,h,w] int8, d_split_parent [B, max_contacts, 2] int32: all four NULL or all four given, a mixture is refused.
 * d_workspace: device memory, 256-byte aligned, of at least the bytes the function above gives for these sizes; its contents need not be
 * kept between calls.  Asynchronous on `stream`: no host read-back, no allocation, no memset, no float atomics; every output byte the
 * function owns is written by a kernel.  Every argument is checked before any HIP call: VISTAF_E_INVALID, with the argument's name in the
 * message, for a NULL or out-of-range argument, a mixed split set, a misaligned pointer or a workspace smaller than required;
 * VISTAF_E_HIP for a runtime failure. */
int vistaf_lobes_measure(const int8_t *d_contact_index, const double *d_contacts, const int32_t *d_count, const double *d_mm_per_px,
                         const float *d_depth_mm, int batch, int h, int w, int max_contacts, int max_lobes, double min_prominence_mm,
                         double min_prominence_frac, double depth_eps_mm, double *d_lobes, double *d_rows, int8_t *d_lobe_index,
                         double *d_split_contacts, int32_t *d_split_count, int8_t *d_split_index, int32_t *d_split_parent, void *d_workspace,
                         size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VISTAF_LOBES_H */
