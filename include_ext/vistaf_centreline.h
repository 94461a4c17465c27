/* vistaf_centreline.h -- C ABI of the centreline read-out, part of libvistaf_ftp.so.
 *
 * An extension with no counterpart in the reference.  The other per-contact read-outs describe a touch as a body (vistaf_ftp_contacts,
 * vistaf_shape.h), a boundary (vistaf_outline.h), a surface (vistaf_texture.h) and a known part (vistaf_match.h); this describes an elongated
 * one -- a cable, a rod, the edge of a plate lying across the skin -- by its centreline: where it runs, which way it leaves at each end, how
 * long it is along itself, how wide along the way, how far it bends and whether it runs off the skin.  It is what a host would get from
 * cv2.ximgproc.thinning, distanceTransform and a graph walk on the index plane, without copying the plane.  Two plain functions and no
 * handle: the caller hands in the workspace.  It reads only what it is handed: the int8 index plane, table and counts vistaf_ftp_contacts
 * wrote, mm_per_px and, if given, the depth plane.  It lives in include_ext/ because it is not part of the drop-in boundary the headers of
 * include/ pin; its ctypes signatures are `_lib.CENTRELINE_SIGNATURES`.
 *
 * THE DEFINITION for frame b, row k of a table of K = max_contacts rows; s = mm_per_px[b]; y points down:
 *   0. ROWS.  kk = min(max(count[b], 0), K).  A row k >= kk is all NaN and writes no stations.
 *   1. PIXELS.  The pixels of row k are the pixels with index == k inside the table's box (BBOX_X0..Y1) clipped to the frame; a box that is
 *      not finite, or empty after clipping, holds no pixel (csrc/contact_rows.hpp: ContactBox).  Every other position is "not k": the other
 *      pixels of the frame, the outside of the box and the outside of the frame.
 *   2. DISTANCE.  D2(p) is the smallest squared Euclidean distance between pixel centres from pixel p of k to a "not k" position, an exact
 *      int32.  The ring of positions just outside the frame counts (nothing farther out can be nearer).
 *   3. SKELETON S: Guo-Hall thinning of the pixels of k in two sub-iterations, neighbours outside the box = 0.  With P2 = N, P3 = NE, P4 = E,
 *      P5 = SE, P6 = S, P7 = SW, P8 = W, P9 = NW of a pixel:
 *          C = (!P2 & (P3|P4)) + (!P4 & (P5|P6)) + (!P6 & (P7|P8)) + (!P8 & (P9|P2)),
 *          N = min((P9|P2) + (P3|P4) + (P5|P6) + (P7|P8), (P2|P3) + (P4|P5) + (P6|P7) + (P8|P9)),
 *          m = (P2|P3|!P5) & P4 in the first sub-iteration, (P6|P7|!P9) & P8 in the second;
 *      a pixel is deleted when C == 1, 2 <= N <= 3 and m == 0, all pixels of a sub-iteration decided on the plane as it was when the
 *      sub-iteration began.  The pair is repeated until a pair deletes nothing; THINNING_PASSES counts the pairs that deleted something.
 *      This is cv::ximgproc::thinning's THINNING_GUOHALL.  On random masks it keeps the number of 8-connected pieces and of holes, never
 *      empties a mask and is idempotent (tests/test_centrelines.py); a solid square thins to one pixel.
 *   4. WALK.  Hops are steps between 8-adjacent pixels of S; "first" among pixels always means the smallest (y, x).  The SEED is the first
 *      pixel of S with the largest D2.  A0 is the first pixel with the most hops from the seed, B0 the first pixel with the most hops from
 *      A0.  The PATH starts at B0 and steps to the first neighbour, in the order N, E, S, W, NE, SE, SW, NW, whose hop count from A0 is one
 *      less, until A0.  It is listed from its end with the smaller (y, x), A, to the other, B: n = STATIONS pixels P_0 = A .. P_{n-1} = B.
 *      A table written by vistaf_ftp_contacts gives one piece per row; on a hand-made plane with several the path lies in the seed's piece
 *      (SKELETON_PIXELS, END_PIXELS and BRANCH_PIXELS count them all).
 *   5. MEASURES, float64: every integer is converted once, every operation is a single IEEE operation, no fused multiply-add, no
 *      trigonometry; sums over stations are formed serially in station order from the first term.  With a / b the axis-parallel / diagonal
 *      steps of the path and core = double(a) + double(b) * sqrt(2.0):
 *          PATH_LENGTH_MM = core * s
 *          LENGTH_MM      = (((core + sqrt(double(D2(A)))) + sqrt(double(D2(B)))) - 1.0) * s      the end radii carry the thinned path to the
 *                                                                                                  tips: a 60 x 7 bar gives exactly 60
 *          CHORD_MM       = sqrt(double(|B - A|^2)) * s
 *          TORTUOSITY     = PATH_LENGTH_MM / CHORD_MM                                               NaN when n < 2
 *          SAGITTA_MM     = double(c) / sqrt(double(|B - A|^2)) * s                                 NaN when n < 2
 *              c_i = (xB - xA) * (y_i - yA) - (yB - yA) * (x_i - xA) (int64), c the c_i of largest magnitude, ties to the smallest i =
 *              SAGITTA_STATION: signed, positive where the curve bulges to +y of a chord that runs to +x.
 *          station i is INTERIOR when |P_i - A|^2 >= 4 * D2(P_i) and |P_i - B|^2 >= 4 * D2(P_i) (integers): at least its own width from both tips
 *          width_i        = (2.0 * sqrt(double(D2(P_i))) - 1.0) * s
 *          WIDTH_MEAN_MM  = (sum of width_i over the interior stations) / double(INTERIOR_STATIONS); WIDTH_MIN_MM / WIDTH_MAX_MM and their
 *                           stations over the same set, ties to the smallest i; all NaN when there is none
 *          WIDTH_SEED_MM  = the same expression at the seed; ELONGATION = LENGTH_MM / WIDTH_SEED_MM
 *          (A_TX, A_TY)   = (double(x_j - xA), double(y_j - yA)) / sqrt(double(|P_j - A|^2)) with j = min(n - 1, tangent_span): the unit
 *                           vector into the contact; (B_TX, B_TY) likewise from B to P_{n-1-j}; NaN when n < 2
 *          A_AT_BORDER    = 1 when min(xA + 1, yA + 1, w - xA, h - yA)^2 <= D2(A), else 0: the outside of the frame is among the nearest
 *                           "not k" of the end, so the contact runs off the skin there.  B_AT_BORDER alike.
 *      With d_depth_mm (float32, each sample converted once): DEPTH_MEAN_MM = (sum over all stations) / double(n); DEPTH_A_MM / DEPTH_B_MM
 *      the same over the first / last min(n, tangent_span + 1) stations; DEPTH_PEAK_MM the largest sample on the path (a sample replaces
 *      the running one when it compares greater, from station 0) and DEPTH_PEAK_STATION its station.  NaN when the pointer is NULL.
 *      END_PIXELS: pixels of S with exactly one 8-neighbour in S.  BRANCH_PIXELS: pixels of S whose ring P2, P3, .., P9, P2 has three or
 *      more 0 -> 1 transitions.
 *   6. STATUS = VISTAF_CLST_OK, _NO_PIXELS or _POINT (n == 1), plus the flags _BRANCHED (BRANCH_PIXELS > 0) and _TRUNCATED
 *      (STATIONS_WRITTEN < STATIONS).  A row in use without a pixel has fields 0..6 equal to 0, STATUS 1 and the rest NaN.  Nothing is
 *      raised for what the data does.
 *   7. POLYLINES.  d_stations [B, max_stations, 2] int32 holds the (x, y) of P_i, d_station_d2 [B, max_stations] int32 their D2 -- the width
 *      profile as exact integers -- and d_offsets [B, K+1] int32 has offsets[0] = 0 and offsets[k+1] - offsets[k] = STATIONS_WRITTEN of row k.
 *      Row k is written whole when STATIONS of rows 0..k together do not exceed max_stations, otherwise not at all: once one row fails, the
 *      later ones fail too.  What lies behind offsets[K] is left untouched.  d_stations and d_offsets NULL: nothing is written and
 *      STATIONS_WRITTEN is 0; d_station_d2 may be NULL on its own.  A NULL d_stations with a non-NULL d_offsets or d_station_d2, or a
 *      non-NULL d_stations with a NULL d_offsets, is refused.
 *   8. d_skeleton [B,h,w] int8, if given, is written whole: k on the pixels of S of row k, -1 elsewhere.
 *   9. DETERMINISM.  All integer work is exact and every double is a fixed expression of integers, s and the depth samples: a frame gives
 *      the same bits alone, in any batch position and on a second call, and they equal the NumPy restatement (tests/centreline_helpers.py).
 *
 * Every function returns 0 or a negative VISTAF_E_* code (vistaf_ftp.h); vistaf_ftp_last_error() holds the message.
 */
#ifndef VISTAF_CENTRELINE_H
#define VISTAF_CENTRELINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* per-contact record: d_centrelines[(b*max_contacts + k)*VISTAF_NCENTRELINE + i] (double), row k = row k of frame b's contacts table */
#define VISTAF_NCENTRELINE 40
#define VISTAF_CENTRELINE_PIXELS 0
#define VISTAF_CENTRELINE_SKELETON_PIXELS 1
#define VISTAF_CENTRELINE_THINNING_PASSES 2
#define VISTAF_CENTRELINE_END_PIXELS 3
#define VISTAF_CENTRELINE_BRANCH_PIXELS 4
#define VISTAF_CENTRELINE_STATIONS 5
#define VISTAF_CENTRELINE_STATIONS_WRITTEN 6
#define VISTAF_CENTRELINE_STATUS 7
#define VISTAF_CENTRELINE_A_X 8
#define VISTAF_CENTRELINE_A_Y 9
#define VISTAF_CENTRELINE_B_X 10
#define VISTAF_CENTRELINE_B_Y 11
#define VISTAF_CENTRELINE_PATH_LENGTH_MM 12
#define VISTAF_CENTRELINE_LENGTH_MM 13
#define VISTAF_CENTRELINE_CHORD_MM 14
#define VISTAF_CENTRELINE_TORTUOSITY 15
#define VISTAF_CENTRELINE_SAGITTA_MM 16
#define VISTAF_CENTRELINE_SAGITTA_STATION 17
#define VISTAF_CENTRELINE_INTERIOR_STATIONS 18
#define VISTAF_CENTRELINE_WIDTH_MEAN_MM 19
#define VISTAF_CENTRELINE_WIDTH_MIN_MM 20
#define VISTAF_CENTRELINE_WIDTH_MIN_STATION 21
#define VISTAF_CENTRELINE_WIDTH_MAX_MM 22
#define VISTAF_CENTRELINE_WIDTH_MAX_STATION 23
#define VISTAF_CENTRELINE_WIDTH_SEED_MM 24
#define VISTAF_CENTRELINE_ELONGATION 25
#define VISTAF_CENTRELINE_A_TX 26
#define VISTAF_CENTRELINE_A_TY 27
#define VISTAF_CENTRELINE_B_TX 28
#define VISTAF_CENTRELINE_B_TY 29
#define VISTAF_CENTRELINE_A_AT_BORDER 30
#define VISTAF_CENTRELINE_B_AT_BORDER 31
#define VISTAF_CENTRELINE_DEPTH_MEAN_MM 32
#define VISTAF_CENTRELINE_DEPTH_A_MM 33
#define VISTAF_CENTRELINE_DEPTH_B_MM 34
#define VISTAF_CENTRELINE_DEPTH_PEAK_MM 35
#define VISTAF_CENTRELINE_DEPTH_PEAK_STATION 36
                                              /* 37..39 reserved (NaN) */

/* values and flags of the STATUS field */
#define VISTAF_CLST_OK 0
#define VISTAF_CLST_NO_PIXELS 1
#define VISTAF_CLST_POINT 2
#define VISTAF_CLST_BRANCHED 8
#define VISTAF_CLST_TRUNCATED 16

/* The bytes of the workspace vistaf_centreline_measure needs for `batch` frames of h x w and tables of max_contacts rows: h, w in 1..32767
 * with h*w <= 2^29 - 1, batch >= 1, max_contacts in 1..VISTAF_MAX_CONTACTS = 64.  Makes no HIP call.  VISTAF_E_INVALID, with the argument's
 * name in the message, for a NULL `bytes` or a size outside these ranges. */
int vistaf_centreline_workspace_bytes(int h, int w, int batch, int max_contacts, size_t *bytes);

/* Measure every contact of `batch` frames.  Inputs (device): d_contact_index [B,h,w] int8, d_contacts [B, max_contacts, VISTAF_NCONTACT]
 * double and d_count [B] int32 as vistaf_ftp_contacts wrote them with the same max_contacts, d_mm_per_px [B] double, d_depth_mm [B,h,w]
 * float32 or NULL; tangent_span in 1..1024, max_stations >= 0.  Outputs (device): d_centrelines [B, max_contacts, VISTAF_NCENTRELINE]
 * double and, unless NULL, d_stations [B, max_stations, 2] int32, d_station_d2 [B, max_stations] int32, d_offsets [B, max_contacts + 1]
 * int32 and d_skeleton [B,h,w] int8.  d_workspace: device memory, 256-byte aligned, of at least the bytes the function above gives for
 * these sizes; its contents need not be kept between calls.  Asynchronous on `stream`: no host read-back, no allocation, no memset, no
 * float atomics; every output byte the function owns is written by a kernel.  Every argument is checked before any HIP call:
 * VISTAF_E_INVALID, with the argument's name in the message, for a NULL or out-of-range argument, a combination of NULL polyline pointers
 * that step 7 refuses, a misaligned pointer or a workspace smaller than required; VISTAF_E_HIP for a runtime failure. */
int vistaf_centreline_measure(const int8_t *d_contact_index, const double *d_contacts, const int32_t *d_count, const double *d_mm_per_px,
                              const float *d_depth_mm, int batch, int h, int w, int max_contacts, int tangent_span, int max_stations,
                              double *d_centrelines, int32_t *d_stations, int32_t *d_station_d2, int32_t *d_offsets, int8_t *d_skeleton,
                              void *d_workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VISTAF_CENTRELINE_H */
