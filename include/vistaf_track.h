/* vistaf_track.h -- C ABI of the contact tracker, part of libvistaf_ftp.so.
 *
 * An extension with no counterpart in the reference: vistaf_ftp_contacts (vistaf_ftp.h) gives one table per frame whose rows are ordered by
 * peak depth, so row k of frame t has nothing to do with row k of frame t+1.  The tracker associates the rows of consecutive frames on the
 * device, from the index planes and tables that call writes, and gives every contact a persistent id, its motion and what became of it.
 * It is an object of its own: it never touches a vistaf_ftp_handle and reads only what it is handed.
 *
 * THE LINK between frame t-1 (rows 0..m-1) and frame t (rows 0..n-1), m, n = min(count, max_contacts); m = 0 before the first frame:
 *   1. O[i][j] = number of pixels with index[t-1] == i and index[t] == j (an exact integer)
 *   2. best_next[i] = the j with the largest O[i][j] > 0, ties to the lowest j, -1 if none; best_prev[j] the same over i, ties to the lowest i
 *   3. i -> j is an overlap link iff best_next[i] == j and best_prev[j] == i
 *   4. gate stage, only when gate_px > 0 (a small contact that moved further than its own size): among the rows i with best_next[i] == -1
 *      and the rows j with best_prev[j] == -1 whose centroids are finite, d2 = dx*dx + dy*dy in float64 from the tables' centroid_x / _y
 *      (no fused multiply-add); candidates are the pairs with d2 <= gate_px*gate_px; the candidate with the smallest (d2, i, j) is linked,
 *      both rows leave, and so on until no candidate is left
 *   5. a linked j inherits its parent's track id with age + 1; an unlinked j is born and takes next_id++, rows in ascending order, frames
 *      in order; ids are never reused until vistaf_track_reset
 *   6. a frame with count == 0 ends every track: whatever follows it is born.  The count of a frame whose status is not VISTAF_FRAME_OK is 0
 *      (vistaf_ftp_contacts), so such a frame ends every track too.  Bridging gaps is not part of the tracker.
 * Every step is integer arithmetic or a single float64 operation in a fixed order: two updates from the same state give the same bits.
 *
 * Every function returns 0 or a negative VISTAF_E_* code (vistaf_ftp.h); vistaf_ftp_last_error() holds the message.
 */
#ifndef VISTAF_TRACK_H
#define VISTAF_TRACK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* per-track record written by vistaf_track_update: d_tracks[(b*max_contacts + k)*VISTAF_NTRACK + i] (double), row k = row k of frame b's
 * contacts table.  Unused rows and fields are NaN, as in the contacts table. */
#define VISTAF_NTRACK 16
#define VISTAF_TRACK_ID 0               /* persistent id of the contact's track                                                   */
#define VISTAF_TRACK_AGE_FRAMES 1       /* 0 at birth, parent's age + 1 otherwise                                                 */
#define VISTAF_TRACK_PARENT_ROW 2       /* row of the previous frame's table this contact continues, -1 if born                    */
#define VISTAF_TRACK_EVENTS 3           /* bitmask of VISTAF_TRACKEV_*                                                            */
#define VISTAF_TRACK_OVERLAP_PX 4       /* O[parent][row]; 0 if gated or born                                                     */
#define VISTAF_TRACK_DX 5               /* centroid_x minus the parent's, one float64 subtraction; NaN at birth                    */
#define VISTAF_TRACK_DY 6
#define VISTAF_TRACK_DFORCE_N 7         /* force_N minus the parent's; NaN at birth                                               */
#define VISTAF_TRACK_DVOLUME_CM3 8      /* volume_cm3 minus the parent's; NaN at birth                                            */
#define VISTAF_TRACK_ORIGIN_TRACK_ID 9  /* for VISTAF_TRACKEV_SPLIT the track id of row best_prev[row] of the previous frame, else -1 */
                                        /* 10..15 reserved (NaN) */

#define VISTAF_TRACKEV_BORN 1           /* no parent: a new track id                                                              */
#define VISTAF_TRACKEV_SPLIT 2          /* born, but best_prev[row] >= 0: it broke off a contact whose track went elsewhere        */
#define VISTAF_TRACKEV_MERGED 4         /* some unlinked row i of the previous frame has best_next[i] == row                       */
#define VISTAF_TRACKEV_GATED 8          /* linked by the gate stage, without overlap                                              */

/* d_fate[b*max_contacts + i] (int32): what became, in frame b, of row i of the frame before it */
#define VISTAF_FATE_ENDED (-1)             /* no successor                                             */
#define VISTAF_FATE_ABSORBED(j) (-(2 + (j))) /* unlinked, most of its overlap went to contact j         */
#define VISTAF_FATE_NO_ROW INT32_MIN       /* the frame before had no row i; values >= 0: the row that continues the track */

typedef struct vistaf_track_handle vistaf_track_handle;

/* A tracker for h x w index planes, at most max_batch frames per update, tables of max_contacts rows (1..VISTAF_MAX_CONTACTS = 64: the K of
 * the vistaf_ftp_contacts calls that feed it), gate_px >= 0 and finite (0: no gate stage).  Allocates every buffer on the current device.
 * VISTAF_E_INVALID for a NULL `out` or arguments outside these ranges. */
int vistaf_track_create(int h, int w, int max_batch, int max_contacts, double gate_px, vistaf_track_handle **out);

/* Link `batch` frames, consecutive in time; frame 0 follows the last frame of the previous update (the tracker keeps that frame's index
 * plane, rows, ids, ages and next_id on the device).  Inputs (device), as vistaf_ftp_contacts wrote them with the same max_contacts:
 *   d_contact_index [B,h,w] int8, d_contacts [B, max_contacts, VISTAF_NCONTACT] double, d_count [B] int32
 * Outputs (device): d_tracks [B, max_contacts, VISTAF_NTRACK] double, d_fate [B, max_contacts] int32.
 * Plane values outside 0..min(count, max_contacts)-1 count as -1.  Asynchronous on `stream`; allocates nothing.  VISTAF_E_INVALID for a NULL
 * argument or `batch` outside 1..max_batch, VISTAF_E_HIP for a runtime failure. */
int vistaf_track_update(vistaf_track_handle *tr, const int8_t *d_contact_index, const double *d_contacts, const int32_t *d_count, int batch,
                        double *d_tracks, int32_t *d_fate, void *stream);

/* Forget the carried frame and restart ids at 0; takes effect at the head of the next update, on that update's stream. */
int vistaf_track_reset(vistaf_track_handle *tr);

void vistaf_track_destroy(vistaf_track_handle *tr);

#ifdef __cplusplus
}
#endif
#endif /* VISTAF_TRACK_H */
