/* Test-only entry points of libvistaf_ftp.so for the three binary-mask chains of a predict (k_maskchain.hip against the separate kernels).  NOT
 * part of the drop-in boundary (include/vistaf_ftp.h), like everything in test_hooks.h, which documents the session hook "fused_masks".  Their
 * ctypes signatures are `_lib.MASK_CHAIN_SIGNATURES`; tests/test_mask_chains.py holds that table against these prototypes. */
#ifndef VISTAF_TEST_HOOKS_MASKS_H
#define VISTAF_TEST_HOOKS_MASKS_H
#include "../../include/vistaf_ftp.h"
#ifdef __cplusplus
extern "C" {
#endif
/* The three binary-mask chains of a predict, as a session runs them (the session's own functions, stages.hpp; the hooks are in api_hooks.hip), on device planes [B, h, w] of the
 * caller.  fused: 1 the one-launch kernel of k_maskchain.hip where mask_chain_fits takes (h, w, element, operations), 0 the separate kernels.
 * Every call refuses a NULL plane, B, h or w below 1, a kernel size outside 1..33, iterations outside 0..16 and a `fused` other than 0 / 1 with
 * VISTAF_E_INVALID before anything is allocated, runs on `stream`, waits for it and returns the tier taken (1 the fused kernel, 0 the separate
 * kernels) or a negative VISTAF_E_* code.  Scratch planes of the separate kernels are the call's own.  Elements are the ellipses a session
 * builds: max(3, ksize | 1) for the bad-pixel dilation and the closing, ksize as given for the contact dilation.
 *
 * vistaf_ftp_test_mask_chain_fits: mask_chain_fits for `chain` (1 bad, 2 reliable, 4 contact) with that element, nops operations (bad / contact: the
 * dilations; reliable: 2 * close_iters) and, for the reliable chain, the chamfer ball of margin_px (0: none): 1 / 0.  Launches nothing.
 *
 * _bad_chain: bad1 = `iters` dilations (none for ksize <= 1) of valid[p] && (img >= thr_hi[b] || grad >= thr_g[b]); bad_count[b] its pixels.
 * valid: one [h, w] plane.
 * _reliable_chain: rel0 = roi[p] && finite(q) && q >= amp_thr[b] (roi: one [h, w] plane); reliable = erosion by the chamfer ball of margin_px
 * (0: none) of roi & the largest 8-connected component (ties: the smallest root) of roi & closing(rel0, close_iters); rel_count[b] its pixels;
 * status[b] becomes 1 where that is 0 and status[b] was 0, and is otherwise left alone.
 * _contact_chain: with t = thr3[3 b .. 3 b + 2], the count of reliable && finite(|r|) && |r| >= (t[0], or t[1] when t[0] is not finite) over
 * rel_count[b] (at least 1) chooses the threshold: t[1] below min_frac, t[2] above max_frac, each only if finite; thr_used[b] is that
 * threshold; contact_d = reliable & `iters` dilations of the mask at it; background = reliable & ~contact_d, bg_count[b] its pixels, and
 * where bg_count[b] < int(0.15 * rel_count[b]) the background plane is the reliable plane.  reliable holds 0 / 1. */
int vistaf_ftp_test_mask_chain_fits(int chain, int h, int w, int ksize, int nops, int margin_px);
int vistaf_ftp_test_bad_chain(const float *img, const float *grad, const uint8_t *valid, const float *thr_hi, const float *thr_g, int ksize, int iters,
                              uint8_t *bad1, int *bad_count, int B, int h, int w, int fused, void *stream);
int vistaf_ftp_test_reliable_chain(const float *quality, const uint8_t *roi, const float *amp_thr, int close_ksize, int close_iters, int margin_px,
                                   uint8_t *rel0, uint8_t *reliable, int *rel_count, int32_t *status, int B, int h, int w, int fused, void *stream);
int vistaf_ftp_test_contact_chain(const float *resid, const uint8_t *reliable, const float *thr3, const int *rel_count, double min_frac, double max_frac,
                                  int ksize, int iters, float *thr_used, uint8_t *contact_d, uint8_t *background, int *bg_count, int B, int h, int w,
                                  int fused, void *stream);
#ifdef __cplusplus
}
#endif
#endif
