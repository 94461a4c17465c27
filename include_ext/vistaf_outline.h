/* vistaf_outline.h -- C ABI of the contact outline read-out, part of libvistaf_ftp.so.
 *
 * An extension with no counterpart in the reference.  vistaf_ftp_contacts (vistaf_ftp.h) says where a touch is and vistaf_shape.h gives the
 * ellipse of its footprint; this gives the footprint's outline: its boundary loops and holes, the corner polyline of its outer loop, its
 * convex hull and the caliper box -- what a host would get from findContours, convexHull and minAreaRect on the index plane, without
 * copying the plane.  Two plain functions and no handle: the caller hands in the workspace.  It reads only what it is handed, the int8 index
 * plane, table and counts vistaf_ftp_contacts wrote.  It lives in include_ext/ because it is not part of the drop-in boundary the headers of
 * include/ pin; its ctypes signatures are `_lib.OUTLINE_SIGNATURES`.
 *
 * THE DEFINITION for frame b, row k of a table of K = max_contacts rows; s = mm_per_px[b]:
 *   0. kk = min(max(count[b], 0), K).  A row k >= kk is all NaN and writes no vertices.
 *   1. The PIXELS of row k are the pixels with index == k inside the table's box (BBOX_X0..Y1) clipped to the frame; a box that is not
 *      finite, or empty after clipping, holds no pixel (csrc/contact_rows.hpp: ContactBox).  The frame's outside, and the box's, is "not k".
 *      Depth is not read: this is the 8-connected component itself, NOT the `depth > eps` subset of vistaf_shape.h, whose BOUNDARY_PIXELS
 *      (pixels of that subset with a 4-neighbour outside it) is a different quantity from every count below.
 *   2. LATTICE.  Pixel (x, y) is the square [x, x+1] x [y, y+1]; vertices are the integer corners 0..w by 0..h.  A directed unit edge
 *      (x, y, d) starts at vertex (x, y) and runs in direction d = 0: +x, 1: +y, 2: -x, 3: -y.  Its right pixel R and left pixel L:
 *          d = 0: R (x, y)      L (x, y-1)          d = 2: R (x-1, y-1)  L (x-1, y)
 *          d = 1: R (x-1, y)    L (x, y)            d = 3: R (x, y-1)    L (x-1, y-1)
 *      It is a BOUNDARY EDGE of k when R is a pixel of k and L is not; every boundary edge has exactly one owner.
 *   3. SUCCESSOR.  With Q the end vertex of the edge and AL, AR the left and right pixels of the edge (Q, d): the next edge is
 *      (Q, (d+3) % 4) if AL is a pixel of k, else (Q, d) if AR is, else (Q, (d+1) % 4).  This is the 8-connectivity rule: two pixels that
 *      meet only at a corner lie on one loop.  Every boundary edge lies on exactly one closed loop.  The twice-area of a loop,
 *      A2 = sum over its edges (x, y) -> (x', y') of x*y' - x'*y, is even and non-zero: positive for an outer loop, negative for a hole.
 *      The sum of A2 / 2 over the loops of k is its pixel count; positive loops = 8-connected pieces, negative loops = holes (4-connected
 *      background components that do not reach the outside).
 *   4. The PRINCIPAL LOOP is the positive loop with the largest A2; ties go to the loop whose first edge in (y, x, d) order comes first.
 *      (That first edge of a positive loop is a d = 0 edge and the edge before it is not, so it starts at a corner.)  A table written by
 *      vistaf_ftp_contacts gives one positive loop per row; a hand-made plane may give several, which PIECES reports.
 *   5. CORNERS of a loop: the start vertices of its edges whose predecessor has another d.  The corner list of the principal loop begins
 *      at the start vertex of its first edge in (y, x, d) order and follows the loop.
 *   6. HULL: the convex hull of the corner vertices of all positive loops of k (= the hull of the union of its pixel squares), strictly
 *      convex (collinear points dropped), decided by int64 cross products, listed in the loops' orientation (positive shoelace) from the
 *      vertex with the smallest (y, x): m >= 4 vertices H_0..H_{m-1}, twice-area HA2 (int64).
 *   7. CALIPERS, float64 throughout; every integer is converted once, every operation is a single IEEE operation, no fused multiply-add.
 *      For hull edge i: e = H_{i+1} - H_i = (ex, ey), L2 = ex*ex + ey*ey; over all hull vertices j, a_j = (H_j - H_i) . e and
 *      c_j = ex*(y_j - y_i) - ey*(x_j - x_i) (int64), amin, amax, cmax their extremes;
 *          area_i = double(amax - amin) * double(cmax) / double(L2),  along_i = double(amax - amin) / sqrt(double(L2)),
 *          across_i = double(cmax) / sqrt(double(L2)).
 *      BOX: the edge i* of smallest area_i, ties to the smallest i.  BOX_LENGTH_MM = max(along, across) * s, BOX_WIDTH_MM = min(along,
 *      across) * s, BOX_CX = double(x_i) + double(ex*(amin + amax) - ey*cmax) / double(2*L2), BOX_CY = double(y_i) + double(ey*(amin + amax)
 *      + ex*cmax) / double(2*L2) (numerators int64), BOX_ANGLE_RAD = DIR(ey, ex) when along >= across, else DIR(ex, -ey), where DIR(p, q)
 *      is atan2(p, q) folded into (-pi/2, pi/2]: pi is added at or below -pi/2 and subtracted above pi/2.
 *      MIN_FERET_MM = s * the smallest across_i.  MAX_FERET_MM = sqrt(double(D2)) * s for the largest D2 = |H_j - H_i|^2 (int64) over
 *      i < j; MAX_FERET_ANGLE_RAD = DIR(dy, dx) of the first such pair (smallest i, then smallest j).
 *   8. DETERMINISM.  All integer work is exact and every double is a fixed expression of integers and s: a frame gives the same bits alone,
 *      in any batch position and on a second call.
 *
 * POLYLINES.  d_vertices [B, max_vertices, 2] int32 holds (x, y) pairs; d_offsets [B, K+1] int32 has offsets[0] = 0 and offsets[k+1] -
 * offsets[k] = CORNERS_WRITTEN of row k.  Row k is written whole when CORNERS of rows 0..k together do not exceed max_vertices, otherwise
 * not at all: once one row fails, the later ones fail too.  Overflow is reported through CORNERS_WRITTEN < CORNERS, never raised.  What lies
 * behind offsets[K] is left untouched.  Either pointer may be NULL: then no polyline is written and CORNERS_WRITTEN is 0; a NULL d_vertices
 * together with a non-NULL d_offsets is refused.
 *
 * Every function returns 0 or a negative VISTAF_E_* code (vistaf_ftp.h); vistaf_ftp_last_error() holds the message.
 */
#ifndef VISTAF_OUTLINE_H
#define VISTAF_OUTLINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* per-contact record: d_outlines[(b*max_contacts + k)*VISTAF_NOUTLINE + i] (double), row k = row k of frame b's contacts table.  A row in use
 * that has no pixel has fields 0..4 and 7..9 equal to 0 and the rest NaN; a row not in use is all NaN. */
#define VISTAF_NOUTLINE 24
#define VISTAF_OUTLINE_PIXELS 0               /* pixels of row k                                                          */
#define VISTAF_OUTLINE_PIECES 1               /* positive loops                                                           */
#define VISTAF_OUTLINE_HOLES 2                /* negative loops                                                           */
#define VISTAF_OUTLINE_EDGES 3                /* unit edges of the principal loop                                         */
#define VISTAF_OUTLINE_EDGES_ALL 4            /* unit edges of every loop of k                                            */
#define VISTAF_OUTLINE_PERIMETER_MM 5         /* double(EDGES) * s                                                        */
#define VISTAF_OUTLINE_ENCLOSED_PIXELS 6      /* A2 / 2 of the principal loop                                             */
#define VISTAF_OUTLINE_CORNERS 7              /* corners of the principal loop                                            */
#define VISTAF_OUTLINE_CORNERS_WRITTEN 8      /* how many of them were written (the capacity rule above)                  */
#define VISTAF_OUTLINE_HULL_VERTICES 9        /* m                                                                        */
#define VISTAF_OUTLINE_HULL_AREA_MM2 10       /* double(HA2) / 2 * s * s                                                  */
#define VISTAF_OUTLINE_SOLIDITY 11            /* double(PIXELS) / (double(HA2) / 2)                                       */
#define VISTAF_OUTLINE_MAX_FERET_MM 12
#define VISTAF_OUTLINE_MAX_FERET_ANGLE_RAD 13
#define VISTAF_OUTLINE_MIN_FERET_MM 14
#define VISTAF_OUTLINE_BOX_CX 15
#define VISTAF_OUTLINE_BOX_CY 16
#define VISTAF_OUTLINE_BOX_LENGTH_MM 17
#define VISTAF_OUTLINE_BOX_WIDTH_MM 18
#define VISTAF_OUTLINE_BOX_ANGLE_RAD 19
                                              /* 20..23 reserved (NaN) */

/* The bytes of the workspace vistaf_outline_measure needs for `batch` frames of h x w and tables of max_contacts rows: h, w in 1..32767 with
 * h*w <= 2^29 - 1 (an edge slot is an int32 and a frame has up to 4*h*w of them), batch >= 1, max_contacts in 1..VISTAF_MAX_CONTACTS = 64.
 * Makes no HIP call.  VISTAF_E_INVALID, with the argument's name in the message, for a NULL `bytes` or a size outside these ranges. */
int vistaf_outline_workspace_bytes(int h, int w, int batch, int max_contacts, size_t *bytes);

/* Measure every contact of `batch` frames.  Inputs (device): d_contact_index [B,h,w] int8, d_contacts [B, max_contacts, VISTAF_NCONTACT]
 * double and d_count [B] int32 as vistaf_ftp_contacts wrote them with the same max_contacts, d_mm_per_px [B] double.  Outputs (device):
 * d_outlines [B, max_contacts, VISTAF_NOUTLINE] double and, unless NULL, d_vertices [B, max_vertices, 2] int32 and d_offsets
 * [B, max_contacts + 1] int32 (max_vertices >= 0).  d_workspace: device memory, 256-byte aligned, of at least the bytes the function above
 * gives for these sizes; its contents need not be kept between calls.  Asynchronous on `stream`: no host read-back, no allocation, no
 * memset, no float atomics.  Every argument is checked before any HIP call: VISTAF_E_INVALID, with the argument's name in the message, for a
 * NULL or out-of-range argument, a NULL d_vertices with a non-NULL d_offsets, a misaligned workspace or one smaller than required;
 * VISTAF_E_HIP for a runtime failure. */
int vistaf_outline_measure(const int8_t *d_contact_index, const double *d_contacts, const int32_t *d_count, const double *d_mm_per_px, int batch,
                           int h, int w, int max_contacts, int max_vertices, double *d_outlines, int32_t *d_vertices, int32_t *d_offsets,
                           void *d_workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VISTAF_OUTLINE_H */
