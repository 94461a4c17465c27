/* Test-only entry points of libvistaf_ftp.so for the LDS-staged demodulation kernels (k_dft.hip: k_dft_fwd1_staged, k_dft_inv2_staged) against the
 * kernels that read their operands from global memory.  NOT part of the drop-in boundary (include/vistaf_ftp.h), like everything in test_hooks.h,
 * which documents the session hook "dft_staged" and the two hooks these extend.  Their ctypes signatures are `_lib.DFT_STAGED_SIGNATURES`;
 * tests/test_dft_staged.py runs them. */
#ifndef VISTAF_TEST_HOOKS_DFT_H
#define VISTAF_TEST_HOOKS_DFT_H
#include "../../include/vistaf_ftp.h"
#ifdef __cplusplus
extern "C" {
#endif
/* vistaf_ftp_test_dft_forward and vistaf_ftp_test_dft_inverse of test_hooks.h (same arguments, same checks, same results) with a `variant`:
 * 0 dispatch as a session does (what the plain hooks run), 1 the kernels that read their operands from global memory (session hook
 * "dft_staged" = 0), 2 the LDS-staged kernel of the stage (k_dft_fwd1_staged of the forward, k_dft_inv2_staged of the inverse transform; stages 2
 * and 3 have one kernel each); VISTAF_E_INVALID where vistaf_ftp_test_dft_staged_fits says that the shape does not take it, or for another variant. */
int vistaf_ftp_test_dft_forward_v(const float *iw, const float *mu, const void *Ex, const void *Ey, size_t tab_stride_x, size_t tab_stride_y, const float *win,
                                  int win_stride, void *T, void *patch, int patch_stride, int B, int h, int w, int ph, int pw, int variant, void *stream);
int vistaf_ftp_test_dft_inverse_v(const void *patch, int patch_stride, const void *Gx, const void *Gy, size_t tab_stride_x, size_t tab_stride_y, void *Q,
                                  void *field, float *amp, const void *cref, const float *amp_ref, size_t ref_stride, float *prod, float *wrapped,
                                  const int32_t *gi_or_null, int B, int h, int w, int ph, int pw, int variant, void *stream);

/* What a demodulation of h x w frames with a ph x pw patch layout takes when "dft_staged" is 1, as bits: 1 the row stage runs k_dft_fwd1_staged
 * (pw <= 24), 2 the last stage runs k_dft_inv2_staged (ph <= 22: 2 KB of LDS per patch row + 4 KB, 48 KB at most); or a negative error.  Launches nothing. */
int vistaf_ftp_test_dft_staged_fits(int h, int w, int ph, int pw, int per_frame_tables);

#ifdef __cplusplus
}
#endif
#endif
