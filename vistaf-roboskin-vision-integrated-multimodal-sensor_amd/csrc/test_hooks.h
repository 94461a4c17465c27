/* Test-only entry points of libvistaf_ftp.so.  NOT part of the drop-in boundary (include/vistaf_ftp.h): nothing a caller of the
 * path needs lives here.  The parity tests use them to run the fallback / opt-in kernels of a stage against the default ones and
 * to read planes that the production path does not materialise.
 * Hooks: vistaf_ftp_test_set (tiers of a session); the production launchers on planes of the caller -- vistaf_ftp_test_select,
 * _select_instance, _select_chained, _polyfit, _gauss (selection, IRLS fit, blur), _chamfer, _cc_label, _cc_largest, _chamfer_dispatch,
 * _blob_filter (mask topology), _unwrap (phase unwrap), _inpaint (the Telea tiers), _top_peaks, _carrier_choose, _build_tables,
 * _build_full_tables, _dft_forward, _dft_inverse (demodulation: peak search, carrier choice, twiddle tables, the float64 GEMM stages), _morph
 * (the three dilate / erode kernels), _tempseg_plane, _tempseg_sign (the planes between the stages of the stripe segmentation, its sign split);
 * vistaf_ftp_test_scratch_regions (scratch layouts) and vistaf_ftp_test_dft_full_mag (the full-spectrum magnitude, asynchronous: also a timing
 * aid).  The entry points of the three binary-mask chains (vistaf_ftp_test_bad_chain and friends) are declared in test_hooks_masks.h, those of
 * the back end of a predict in test_hooks_post.h: vistaf_ftp_test_smooth_reliable, _core_flip, _hole_candidates, _hole_tmp, _hole_zin, _hole_merge,
 * _height_finish (frontier taper, composition, clamp, mm curve), _to_mm (the mm curve alone), _tail (the force tails), _backend (blob filter, tail and output copy, fused or
 * separate), _backend_fits and _frame_records (launch_fill_scalars, launch_mark_empty).
 * Definitions: vistaf_ftp_test_set, which reads the handle, in api.hip; the _tempseg hooks in tempseg.hip; every other hook in api_hooks.hip,
 * which never sees a handle.  Where a stage of a predict chooses between kernel tiers the hook calls the function the session calls
 * (stages.hpp). */
#ifndef VISTAF_TEST_HOOKS_H
#define VISTAF_TEST_HOOKS_H
#include "../../include/vistaf_ftp.h"
#include "../../include/vistaf_temp.h"
#ifdef __cplusplus
extern "C" {
#endif
/* name: "inpaint_tier"  2 window march + whole-frame fallback (default), 1 whole-frame kernel only, 0 cluster front end first
 *       "big_flood_handback" 0 (default), 1 (frames beyond the uint16 rank range only): the bitmap flood hands every frame back to the
 *                      generic kernel, as it does for masks larger than its bitmap
 *       "chamfer_twopass" 1 forces the one-wave two-pass chamfer transform (also for the wide frontier band of native crops, where batches
 *                      below 16 frames take the closed form)
 *       "telea_two_tier" 1 (default) 111 KB first tier of the window march + full-size retry, 0 full-size march only
 *       "unwrap_fast"  1 (default) frames whose wrapped field is verified path-independent take the parallel integration (k_unwrap_fast.hip)
 *                      instead of the priority flood, 0 always the flood (the parent plane is only produced by the flood)
 *       "big_chain"    1 (default) large frames (>= 512 x 512): selections and IRLS fits as chains of streaming kernels over the whole batch (k_big.hip),
 *                      0 one workgroup per frame (k_select / k_robust_polyfit)
 *       "telea_mw"     1 (default) 16-wave window kernel (ordering pass + dataflow fills) in front of the single-wave tiers, 0 single-wave tiers only
 *       "big_queue_lds" 1 (default) the march of a cluster no LDS window takes (k_inpaint_big.hip) keeps its queue in LDS whenever the cluster's cell
 *                      counts bound it, 0 always in the wave's slice of global memory (the path of clusters beyond that bound)
 *       "big_gq_cap"   capacity (entries, a power of two >= 64) that the big-cluster march checks its global queue slice against; 0 (default)
 *                      the slice's own size.  Only shrinks the capacity: the slice stride stays, pushes stay bounds-checked (overflow -> status 2)
 *       "big_fallback" 1 (default) a frame whose big-cluster queue overflowed (status 2) is re-marched whole by the whole-frame kernel,
 *                      0 the frame keeps status 2 and its overflowed cluster stays unfilled (shows that an overflow happened)
 *       "fused_chains" 1 (default) the element-wise passes around a Gaussian of at most 15 taps (illumination normalise / apodise, masked
 *                      smoothing's prologue and division, frontier taper / clamp / mm curve) run inside the blur's tile (k_blurchain.hip) and the
 *                      planes between them (inorm, z0, mplane, num, den, z0f, snum) are not written; 0 one streaming kernel per pass
 *       "fused_backend" 1 (default) frames whose label forest fits LDS (the ones launch_cc_label labels with the mask staged in LDS) run the blob
 *                      filter, the force tail and the copy to the caller's planes in one launch (k_backend.hip); 0 the separate kernels
 *                      (labels, peak plane clear, peaks, decision, tail, copy).  Same bits either way.  With stage timing on, the fused launch is charged
 *                      to the mm / blob stage as a whole (tail and copy included); the tail stage then holds k_fill_scalars and the two copies only
 *       "fused_masks"  7 (default) bits 1 / 2 / 4: the bad-pixel, the reliable and the contact / background mask chain of frames whose bit planes (and,
 *                      for the reliable mask, label forest) fit LDS -- mask_chain_fits of mask_bits.hpp -- run as one launch each (k_maskchain.hip) and
 *                      the planes between their steps (bad0, rel1, rel2, contact, the reliable stage's labels; area off the roots) are not written;
 *                      a cleared bit, or a frame or configuration the tier does not take: the separate kernels.  Same bits either way
 *       "select_resident" 1 (default) the exact selections of planes of up to 65536 pixels run k_select_resident (every element loaded once, its key
 *                      kept in a register for all sweeps) and the core threshold and the core median below it share one chained launch; 0 the
 *                      streaming k_select, one launch per selection (two for the core pair).  Same bits either way
 *       "dft_staged"   1 (default) the demodulation stages whose patch dft_staged_fits takes (kernels.hpp; vistaf_ftp_test_dft_staged_fits of test_hooks_dft.h tells)
 *                      read their GEMM operands from LDS: the row stage (k_dft_fwd1_staged: the twiddle table in chunks of 32 columns, the next chunk
 *                      in flight) and the last stage with its epilogue (k_dft_inv2_staged: the workgroup's columns of Q and each wave's rows of Gy,
 *                      the column tiles finished two at a time); 0 the kernels that fetch one element per lane and k-step from global memory.  Every
 *                      accumulator receives the same k-steps in the same order with the same operands: same bits either way.  test_hooks_dft.h has the
 *                      direct hooks that run either kernel of a stage
 *       "gauss_strip"  1 (default) a Gaussian of more than 15 taps on frames gauss_strip_fits (kernels.hpp) takes -- up to 97 taps, the strip's LDS need
 *                      within 48 KB -- runs both passes in one launch, a workgroup per frame and strip of 32 columns with the intermediate plane in
 *                      LDS (k_gauss_strip); 0, or a blur it does not take: the row and the column kernel.  Same bits either way
 *       "fit_window"   1 (default) on frame sizes with a window instance (polyfit_window_variant of kernels.hpp: the column kernels of 32 rows per
 *                      thread and more) the ramp removal and the first detrend fit, which fits its output under the same mask, share one launch
 *                      of the window kernel one ladder step down (k_robust_polyfit_colwin: a thread's slots start at its own first mask row, the
 *                      second fit takes its samples from the registers), followed by the chained plain-size kernel for the frames whose mask
 *                      rows did not fit ("fit_need" of vistaf_ftp_get_intermediate: 1 per such frame); 0, or plane_order_for_removal = 0: one
 *                      plain kernel per fit.  The third fit always runs the plain kernel.  Same bits either way.  test_hooks_fit.h has the direct hooks
 *       "keep_planes"   1 also writes the float64 demodulated field of every frame ("field" of vistaf_ftp_get_intermediate) */
int vistaf_ftp_test_set(vistaf_ftp_handle *hd, const char *name, int value);

/* The production launchers of three kernel families on device planes of the caller, so that a test can feed them inputs no fringe image
 * produces.  Every call runs on `stream`, waits for it and returns 0 (or a VISTAF_E_* code; text in vistaf_ftp_last_error).
 * variant: 0 dispatch as a session does (the k_big.hip chain for planes of 512 x 512 pixels and more -- large_frame of kernels.hpp --, in batches it takes),
 *          1 the one-workgroup-per-frame kernels whatever the size,
 *          2 the k_big.hip chain; VISTAF_E_INVALID when it does not take (B, plane size).  Its scratch is allocated and freed by the call.
 *          3 (vistaf_ftp_test_select only) the streaming one-workgroup-per-frame kernel k_select whatever the size; under variant 1 planes of
 *            up to 65536 pixels take the register-resident k_select_resident and only larger ones k_select. */

/* launch_select: per frame b, the order statistics reqs[0..nreq) of { x = vals[b][i] : mask[b * mask_stride + i] != 0, x finite, then
 * x = |x| if use_abs, then x <= le_thr[b] if le_thr } into out[b * nreq + j] and their count into counts[b] (may be NULL).  A request is
 * float32(q) / float32(100) for the percentile q, negative for the median.  mask_stride: 0 (one mask for the batch) or P.  No valid
 * element: every result is the quiet NaN 0x7fc00000 and the count 0 (block_percentile / block_median of select.hpp, k_sb_setup of
 * k_big.hip); that is where the reference's nanpercentile_safe / nanmedian_safe hand back the caller's fallback value. */
int vistaf_ftp_test_select(const float *vals, const uint8_t *mask, size_t mask_stride, const float *le_thr, int use_abs, const float *reqs, int nreq,
                           float *out, int *counts, int B, int P, int variant, void *stream);

/* The kernel vistaf_ftp_test_select(.., B, P, variant) launches (SelectVariant of kernels.hpp: 0 the k_big.hip chain, 1 the streaming k_select,
 * 2..5 k_select_resident with 16, 32, 49, 64 key slots per thread, for planes of up to 1024 slots pixels), or a negative error.  Launches nothing. */
int vistaf_ftp_test_select_instance(int B, int P, int nreq, int variant);

/* launch_select_chained: nreq <= 4 requests over the same plane and mask in one launch of the resident kernel.  Request 0 is what
 * vistaf_ftp_test_select computes without a threshold; request j > 0 runs over the elements that also satisfy x <= result[j - 1] (float
 * comparison: -0.0 <= 0.0 holds, a NaN result leaves no element), i.e. what a further vistaf_ftp_test_select with le_thr = the previous results
 * computes.  out[j * B + b] (one [B] array per request), counts[b] the count of request 0 (may be NULL).  Returns the instance launched (2..5 as
 * above), VISTAF_E_INVALID when the plane has more than 65536 pixels (a session then runs one launch per request). */
int vistaf_ftp_test_select_chained(const float *vals, const uint8_t *mask, size_t mask_stride, int use_abs, const float *reqs, int nreq, float *out,
                                   int *counts, int B, int P, void *stream);

/* launch_robust_polyfit: coef[b * 6 + 0..6) (entries 3..5 zero for order 1) and resid[b] = z[b] - fit over the whole plane (NaN where z is).
 * Fewer than min_count fitted pixels (mask != 0 and z finite), or min_mask_count > 0 and fewer mask pixels than that: coefficients all
 * zero and resid = z - 0.  Returns the launched instance (FitVariant of kernels.hpp: 0 chain, 1 generic, 2 generic with plain division,
 * 3..7 column kernels of 16, 32, 48, 56, 64 rows per thread, 8..10 the four-group kernels of 48, 56, 64 rows) or a negative error. */
int vistaf_ftp_test_polyfit(const float *z, const uint8_t *mask, int order, int iters, float c, int min_count, int min_mask_count, float *coef,
                            float *resid, int B, int h, int w, int variant, void *stream);

/* (test_hooks_fit.h: the same with the window kernel and as a chained pair of fits) */

/* launch_gauss_blur (src != dst) with the taps a session builds for `sigma`, dispatched as a session does: up to 15 taps the one-kernel LDS
 * tile, beyond that the strip kernel where gauss_strip_fits (kernels.hpp) takes the blur, else the row and the column kernel. */
int vistaf_ftp_test_gauss(const float *src, float *dst, double sigma, int B, int h, int w, void *stream);
/* (test_hooks_gauss.h: the same with a kernel variant, and what a blur takes) */

/* The one-wave two-pass chamfer transform (cv::distanceTransform DIST_L2, 3x3) forced, whatever kernel a session would pick for (h, w, cap_px).
 * pair != 0: launch_chamfer_pair, ONE launch for dist_a[b] = distance to the zero pixels and dist_b[b] = distance to the non-zero pixels of
 * mask[b] (w <= 1280; beyond 512 columns only a band of more than 64 rows, cap_px >= 60 and h > 64, takes the two-pass kernel); pair == 0: launch_chamfer, dist_a only, to the zero pixels or (invert != 0) to the non-zero pixels (w <= 512).
 * Planes are [B, h, w]; the integer temporaries are allocated and freed by the call. */
int vistaf_ftp_test_chamfer(const uint8_t *mask, int pair, int invert, float *dist_a, float *dist_b, int B, int h, int w, int cap_px, void *stream);

/* The mask topology launchers (k_cc_dist.hip, k_post.hip) on device planes of the caller.  Every call refuses a NULL plane (and_static apart), a
 * size below 1 and an unknown variant with VISTAF_E_INVALID before anything is allocated or launched, runs on `stream`, waits for it, and
 * returns the tier it launched (the value of the pure function the launcher itself dispatches on) or a negative VISTAF_E_* code.
 *
 * launch_cc_label: labels[b][p] = the smallest pixel index of the 8-connected component of pixel p of mask[b] (mask != 0), -1 off the mask.
 * variant: 0 dispatch as a session does, 1 the global union-find kernels (k_cc_init, k_cc_merge, k_cc_flatten) whatever the size.
 * Returns CcLabelTier of kernels.hpp: 0 the LDS forest with the mask staged in LDS (up to 54606 pixels), 1 the LDS forest alone (up to
 * 65535 pixels), 2 the global kernels. */
int vistaf_ftp_test_cc_label(const uint8_t *mask, int32_t *labels, int B, int h, int w, int variant, void *stream);

/* launch_cc_largest on a label plane as above: out[b][p] = (labels[b][p] == root of the largest component of frame b) && and_static[p];
 * ties go to the smallest root, a frame without a component gives zeros.  and_static: one [P] plane for the batch, or NULL (all ones).
 * variant: 0 dispatch (the three kernels over the whole batch when big_frames(B, P)), 1 k_cc_largest (one workgroup per frame), 2 the batch
 * kernels, whatever the size.  Returns CcLargestTier: 1 k_cc_largest, 2 the batch kernels.  The area and key scratch is the call's own. */
int vistaf_ftp_test_cc_largest(const int32_t *labels, const uint8_t *and_static, uint8_t *out, int B, int P, int variant, void *stream);

/* launch_chamfer (pair == 0: dist_a = distance to the zero pixels, or with invert != 0 to the non-zero pixels) or launch_chamfer_pair
 * (pair != 0: dist_a to the zero, dist_b to the non-zero pixels) as a session calls them: nothing forced.  Returns ChamferTier: 0
 * k_chamfer_lds, 1 k_chamfer2, 2 k_rowdist + k_chamfer_cols.  Tiers 0 and 2 are the closed form over a band of rows: equal to the two-pass
 * transform wherever that one is at most cap_px + 2, and beyond cap_px + 2 (and no smaller than it) everywhere else. */
int vistaf_ftp_test_chamfer_dispatch(const uint8_t *mask, int pair, int invert, float *dist_a, float *dist_b, int B, int h, int w, int cap_px,
                                     void *stream);

/* launch_blob_filter, the separate kernels (k_blob_peaks, k_blob_apply): kept[b][p] = cand[b][p] && peak of p's component >= threshold of
 * frame b, and depth_inout is zeroed at the candidates that are not kept.  labels: as vistaf_ftp_test_cc_label writes them for the plane
 * `cand` (every candidate pixel must carry a root: the kernel indexes the peak plane with it).  gmax: [B] float32, the frame maxima whose
 * bits k_to_mm leaves.  The threshold is float32(max(min_peak_mm, rel_frac * gmax[b])) formed in float64, min_peak_mm alone for
 * rel_frac < 0.  Returns 0. */
int vistaf_ftp_test_blob_filter(float *depth_inout, const uint8_t *cand, const int32_t *labels, const float *gmax, double min_peak_mm, double rel_frac,
                                uint8_t *kept, int B, int P, void *stream);

/* launch_unwrap (k_unwrap.hip: the consistency check of k_unwrap_fast.hip, then the rank kernels, the priority flood and the replay / tree
 * kernel of the frames it hands on) on device planes [B, h, w] of the caller.  Its scratch (unwrap_scratch_bytes) is allocated and freed by
 * the call, which runs on `stream` and waits for it.
 * unwrapped[b][p] = float32(float64(wrapped[b][p]) + 2 pi k) with k the integer wrap count of unwrap_quality_guided's spanning tree from the
 * seed (the largest quality on the mask, the first such pixel in raster order), the quiet NaN 0x7fc00000 wherever the growth never arrives;
 * parent[b][p] = the pixel's parent in that tree (the seed: itself; -1 where the growth never arrives).  The parent plane is a by-product of
 * the flood: a frame the consistency check settles (need[b] == 0) leaves parent[b] as the caller passed it.
 * variant: 0 as a session does: the consistency check first, need[b] = 0 for the frames it settles (an empty mask among them: nothing on it
 *            contradicts, the plane is all NaN) and 1 for the frames handed to the flood (an inconsistent pair, a pair within 1e-5 of the
 *            branch cut, more runs or edges than the check's tables, a wrap count beyond +-126),
 *          1 the floods only (the check is off; `need` may be NULL and is not written),
 *          2 as 1, with big_handback: the bitmap flood hands every frame to the generic one-wave flood.
 * Returns UnwrapTier of kernels.hpp, the value of the pure function launch_unwrap dispatches on: 0 uint16 ranks and the batched flood in LDS
 * ((h + 2)(w + 2) <= 65533), 1 32-bit ranks and the bitmap flood, 2 the generic flood (variant 2 beyond the uint16 range, and every frame of
 * 2^26 padded pixels and more).  status[b] is only ever written with 2 (the generic flood's frontier overflowed): pass zeros.
 * Refused with VISTAF_E_INVALID before anything is allocated: a NULL plane (`need` too under variant 0), B < 1, h < 8 or w < 8 (what
 * vistaf_ftp_create accepts), an unknown variant, variant 0 on a shape the check does not take (h > 32767 or w > 65535).
 * Contract on the planes, which a session guarantees and the kernels rely on: quality is finite and >= +0 on the mask (compute_reliable_mask
 * excludes non-finite values, and the blur of a non-negative product has no -0.0: the rank keys order by the float's bits); wrapped is finite
 * and in [-pi, pi] (float32 pi included), so every pixel pair differs by at most 2 pi. */
int vistaf_ftp_test_unwrap(const float *wrapped, const float *quality, const uint8_t *mask, float *unwrapped, int32_t *parent, int32_t *need,
                           int32_t *status, int B, int h, int w, int variant, void *stream);

/* The Telea inpaint launchers (k_inpaint*.hip) on device planes [B, h, w] of the caller: img_inout[b] becomes cv2.inpaint(img, bad != 0, range,
 * INPAINT_TELEA) of itself, bit for bit, known pixels untouched.  Scratch is allocated and freed by the call, which runs on `stream` and waits
 * for it.  status [B]: pass zeros; only ever written with 2 (VISTAF_FRAME_QUEUE_OVERFLOW).  fb [B]: written by every variant but 1.
 * variant: 0 what the bad-pixel stage of a session launches with the default tiers (inpaint_dispatch of stages.hpp, the session's own function):
 *            the window tiers and the whole-frame kernel, or above 8 * 14464 pixels the cluster front end, the big-cluster march and its
 *            hand-back.  fb[b] = 1: the whole-frame kernel took frame b,
 *          1 launch_inpaint_telea alone on every frame; round_u8 != 0: 8-bit semantics (values 0..255, every estimate rounded as OpenCV's
 *            uchar path does), which is what vistaf_temp_inpaint_map runs,
 *          2 the bounding-box pass and the 16-wave window kernel alone (ranges 1..4), 3 the single-wave window kernel alone at first-tier
 *            capacity, 4 at full size.  No retry, no whole-frame kernel: fb[b] = 1 is that tier's hand-back, and such a frame is exactly as
 *            it was passed (nothing has been written back); fb[b] = 0: the tier completed the frame,
 *          5 Tiers::inpaint 0: the cluster front end whatever the size, the big-cluster march (queue in LDS where the cell counts allow) and the
 *            hand-back to the whole-frame kernel (fb[b] = 1: frame b went there), 6 as 5 with big_queue_lds off (ranges 1..5 for both).
 * Refused with VISTAF_E_INVALID before anything is allocated: a NULL plane, B < 1, h < 8 or w < 8, range outside 1..100 (cv::inpaint clamps to
 * that), an unknown variant, round_u8 with a variant other than 1, a range the variant's kernels do not take.
 * Contract on the planes, which a session guarantees: the image is finite (the grey image; z0 after launch_hole_zin). */
int vistaf_ftp_test_inpaint(float *img_inout, const uint8_t *bad, int range, int round_u8, int32_t *fb, int32_t *status, int B, int h, int w, int variant,
                            void *stream);

/* The scratch layout of one stage, from a counting pass of the function its launcher carves with (ScratchLayout, host_util.hpp).  Makes no HIP
 * call.  stage: "unwrap", "telea", "inpaint_big" (padding range + 1), "inpaint_cl", "inpaint_win", "big", "tstats" (one frame: B is ignored),
 * and "pressure" (the workspace of vistaf_pressure.h; range = pad_px).
 * Region i, in carve order: names + 32 * i (NUL-terminated), offset[i], bytes[i], align[i]; *total = the size the stage's *_scratch_bytes
 * returns (for "inpaint_big": at this range, not at the widest padding).  Returns the number of regions, or VISTAF_E_INVALID for an unknown
 * stage, a bad shape, or more regions than `cap`. */
int vistaf_ftp_test_scratch_regions(const char *stage, int B, int h, int w, int range, int cap, char *names, size_t *offset, size_t *bytes, size_t *align,
                                    size_t *total);

/* launch_dft_full_mag (the reference frame's full-spectrum magnitude, k_dft.hip) on planes and tables of the caller's, for the direct tests
 * and the timing of tests/diag/bench_pressure.py: planes [B,h,w] float32, Ex_half [w][Wf/2+1] and Ey_full [Hf][h] complex128, tmp [B*h][Wf/2+1] complex128,
 * mag [B,Hf,Wf] float64, all on the device.  Asynchronous on `stream`. */
int vistaf_ftp_test_dft_full_mag(const float *planes, const void *Ex_half, const void *Ey_full, void *tmp, double *mag, int B, int h, int w, int Hf,
                                 int Wf, void *stream);

/* The demodulation launchers (k_dft.hip, k_dft_tables.hip) on device planes and tables of the caller's, so that a test chooses their contents.
 * Every call refuses a NULL plane (the optional ones apart), a bad size and a stride smaller than what it strides over with VISTAF_E_INVALID
 * before anything is allocated or launched, runs on `stream`, waits for it, and returns 0 or a negative VISTAF_E_* code.  complex128 planes
 * and tables are arrays of (re, im) doubles.
 * A CarrierGeom (kernels.hpp) crosses the boundary as two HOST arrays per frame, in struct order:
 *   gd[7]  float64: peak_x, peak_y, kx, ky, dpx, dpy, period;   gi[10] int32: x0, y0, ph, pw, px_i, py_i, px_raw, py_raw, ok, keep_carrier. */

/* launch_top_peaks: out[b][3 i .. 3 i + 2] = (x, y, value) of the i-th largest magnitude of mag[b] ([B, Hf, Wf] float64, non-negative) with the
 * box [cy - dc, cy + dc) x [cx - dc, cx + dc) around the centre counted as zero; descending, equal values by ascending linear index.  out is
 * [B][192]: entries from 3 * npeaks on are not written.  npeaks 1..64, Hf * Wf >= npeaks. */
int vistaf_ftp_test_top_peaks(const double *mag, int B, int Hf, int Wf, int dc, int npeaks, double *out, void *stream);

/* launch_carrier_choose on peak lists of the caller's (peaks [B][192] as above, the first npk entries of each, 1..64; integer positions inside the
 * plane, or the call is refused) and the magnitude planes the refinement reads: choose_carrier_peak, refine_peak_parabolic_log and the patch
 * geometry of half width bw, into gd [B][7] and gi [B][10] on the host. */
int vistaf_ftp_test_carrier_choose(const double *peaks, int npk, const double *mag, int Hf, int Wf, int bw, double max_dy_frac, double *gd, int32_t *gi,
                                   int B, void *stream);

/* launch_build_tables from geometries of the caller's (gd / gi on the host: B of them for geom_stride 1, one for geom_stride 0), Hf = h + 2 pad,
 * Wf = w + 2 pad.  Frame b's tables start at Ex / Gx + b * w * pmax and Ey / Gy + b * h * pmax elements.
 * pair == 0: packed for the frame's own ph x pw (each clamped to pmax): Ex [w][pw], Ey [ph][h], Gx [pw][w], Gy [h][ph]; `win` is not touched.
 * pair != 0: laid out for pmax x pmax with exact zeros beyond ph / pw, and win [B][pmax][pmax] receives hann(ph) x hann(pw) in float32 (zeros
 * beyond), formed from the table of 1-D windows a pair session builds. */
int vistaf_ftp_test_build_tables(const double *gd, const int32_t *gi, int geom_stride, int B, int h, int w, int pad, int Hf, int Wf, int pmax, int pair,
                                 void *Ex, void *Ey, void *Gx, void *Gy, float *win, void *stream);

/* launch_build_full_tables: Exf [w][Wf / 2 + 1], Eyf [Hf][h], the tables vistaf_ftp_test_dft_full_mag takes. */
int vistaf_ftp_test_build_full_tables(void *Exf, void *Eyf, int h, int w, int pad, int Hf, int Wf, void *stream);

/* launch_dft_forward: T [B * h][pw] = (float32(iw - mu[b])) . Ex (mu may be NULL: 0), patch[b * patch_stride + a * pw + c] =
 * win[a][c] * sum_y Ey[a][y] T[b][y][c].  Table strides (elements per frame) are both 0 (one table for the batch: Ex [w][pw], Ey [ph][h]) or both
 * non-zero (per-frame tables); win_stride 0 or elements per frame.  T belongs to the caller: the row stage can be read on its own. */
int vistaf_ftp_test_dft_forward(const float *iw, const float *mu, const void *Ex, const void *Ey, size_t tab_stride_x, size_t tab_stride_y, const float *win,
                                int win_stride, void *T, void *patch, int patch_stride, int B, int h, int w, int ph, int pw, void *stream);

/* launch_dft_inverse: Q [B][ph][w] = patch . Gx (Gx [pw][w]), field = Gy . Q (Gy [h][ph]); amp = float32 |field|; field (may be NULL) the float64
 * field itself; with cref (may be NULL; then amp_ref, prod and wrapped are not touched) wrapped = float32 angle(field * conj(cref)) and
 * prod = amp_ref * amp, the reference planes at b * ref_stride (0: one for the batch).  gi_or_null: [B][10] on the host, of which ph and pw limit
 * each frame's sums inside the ph x pw layout (rows a >= its ph of Q are not written). */
int vistaf_ftp_test_dft_inverse(const void *patch, int patch_stride, const void *Gx, const void *Gy, size_t tab_stride_x, size_t tab_stride_y, void *Q, void *field,
                                float *amp, const void *cref, const float *amp_ref, size_t ref_stride, float *prod, float *wrapped, const int32_t *gi_or_null,
                                int B, int h, int w, int ph, int pw, void *stream);

/* launch_morph (k_basic.hip) on device planes [B, h, w] of the caller: dst[b][p] = 1 where the dilation (dilate != 0: any pixel != 0 under the
 * element) or the erosion (every pixel under the element != 0) of src[b] holds at p, pixels outside the image never contributing
 * (cv::morphologyDefaultBorderValue), ANDed with and_static[p] != 0 (one [h, w] plane for the batch, or NULL) and and_frame[b][p] != 0 ([B, h, w], or
 * NULL); 0 elsewhere.  src != dst.
 * shape: 0 ellipse_se(kx), cv::getStructuringElement(MORPH_ELLIPSE, (kx, kx)) with the anchor at kx / 2 (ky ignored; kx 1..33, the even sizes
 *          are not symmetric about the anchor),
 *        1 rect_se(odd_up(kx), odd_up(ky)), the rectangle as the callers of launch_morph round its sides up to odd (kx 1..127, ky 1..33),
 *        2 a test element no cv shape gives, the hourglass: row i of kx rows spans |i - kx / 2| pixels either side of the anchor (ky ignored;
 *          kx odd, 3..33).  Its rows are not nested towards the centre as an ellipse's or a rectangle's are, so a pixel outside the image
 *          that wrongly took part in an erosion changes the result (with the cv shapes the clamped pixel is always under the element anyway).
 * tier:  0 dispatch as launch_morph does when the caller has prefix scratch (morph_tier of mask_bits.hpp),
 *        1 k_morph (the span scan) forced,
 *        2 k_row_prefix + k_morph_prefix (uint16 row counts) forced; refused for w >= 65536,
 *        3 k_morph_bits (bit planes in LDS) forced; refused where morph_bits_ok says no (an element not symmetric about the anchor or wider
 *          than 127, a frame beyond h * ceil(w / 64) = 4096 words),
 *        4 dispatch without prefix scratch, as k_inpaint_cl.hip calls it.
 * Returns the tier that ran (MorphTier of kernels.hpp: 1, 2 or 3) or a negative VISTAF_E_* code.  The prefix scratch is allocated and freed by the
 * call, which runs on `stream` and waits for it.  Refused with VISTAF_E_INVALID before anything is allocated: a NULL src or dst, src == dst,
 * B, h or w below 1 (or B or h above 65535: the grid), a size out of the ranges above, an unknown shape or tier. */
int vistaf_ftp_test_morph(const uint8_t *src, uint8_t *dst, int B, int h, int w, int shape, int kx, int ky, int dilate, const uint8_t *and_static,
                          const uint8_t *and_frame, int tier, void *stream);

/* One plane that the LAST vistaf_tempseg_segment call left in the session's workspace (tempseg.hip), copied to the DEVICE pointer dst.  Nothing is
 * computed: these are the planes the stages themselves read and write.  `bytes` must be the plane's exact size.
 *   float32 [H, W]     "gray", "g", "blur", "norm", "inorm": BGR2GRAY; gray with the median outside the ROI; its Gaussian (not written when
 *                      seg_illum_sigma <= 0); g / blur; norm / mean over roi_eff
 *   uint8 [H, W]       "sat0", "mask_a": gray >= threshold inside the ROI, before the dilation; the sign mask A before the dark side is chosen
 *   float64 [H, W]     "mag": |fftshift(fft2(inorm))| of the float32 transform
 *   float64 [192]      "peaks": (x, y, value) of the n_peaks largest, as vistaf_ftp_test_top_peaks writes them
 *   complex128 [H, W]  "z": the band-passed field
 *   float32 [1]        "med": median of gray over roi_eff
 *   96 bytes           "geom": gd[7] float64 then gi[10] int32 of the CarrierGeom, in the order given above
 * Refused: a NULL argument, an unknown name or a wrong byte count (VISTAF_E_INVALID); a session whose last segment call did not return 0, or that
 * has not segmented yet (VISTAF_E_STATE).  Runs on `stream` and waits for it. */
int vistaf_ftp_test_tempseg_plane(vistaf_tempseg_handle *handle, const char *name, void *dst, size_t bytes, void *stream);

/* k_ts_sign and its reduction (tempseg.hip) on device planes of n pixels of the caller: mask_a[i] = roi_eff[i] != 0 &&
 * float32(Re(z[i] * exp(-i phi0))) >= 0, the real part formed as re * cos(phi0) - im * (-sin(phi0)) in float64 (so -0.0 and every value that
 * rounds to a float32 zero count as >= 0), 0 elsewhere; sums4 (HOST, 4 doubles) = sum of gray and pixel count over A, then over roi_eff and
 * not A.  z complex128 [n], gray float32 [n].  Refused with VISTAF_E_INVALID: a NULL argument, n < 1, a phi0 that is not finite.  The scratch
 * is the call's own; runs on `stream` and waits for it. */
int vistaf_ftp_test_tempseg_sign(const void *z, double phi0, const uint8_t *roi_eff, const float *gray, uint8_t *mask_a, double *sums4, size_t n,
                                 void *stream);
#ifdef __cplusplus
}
#endif
#endif
