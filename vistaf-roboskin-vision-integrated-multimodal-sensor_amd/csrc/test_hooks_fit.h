/* Test-only entry points of libvistaf_ftp.so for the IRLS fits' window kernel and chained launch (k_fit.hip: k_robust_polyfit_colwin and
 * k_robust_polyfit_col_retry against k_robust_polyfit_col).  NOT part of the drop-in boundary (include/vistaf_ftp.h), like everything in
 * test_hooks.h, which documents the session hook "fit_window" and the hook vistaf_ftp_test_polyfit that the first of these extends.  Their ctypes
 * signatures are `_lib.FIT_WINDOW_SIGNATURES`; tests/test_fit_window.py runs them. */
#ifndef VISTAF_TEST_HOOKS_FIT_H
#define VISTAF_TEST_HOOKS_FIT_H
#include "../../include/vistaf_ftp.h"
#ifdef __cplusplus
extern "C" {
#endif
/* vistaf_ftp_test_polyfit of test_hooks.h (same arguments, same checks, same results in coef and resid) with another `variant`: 0 dispatch as a
 * session does with "fit_window" = 1 -- on frame sizes with a window instance the window kernel, then the plain-size kernel for the frames it
 * flagged; 1 the window kernel alone (VISTAF_E_INVALID where the frame size has none): frames it flags keep coef and resid as the caller left
 * them; 2 the plain kernel, whatever the frame size.  need_out (device, B ints, or null): per frame 1 some thread's mask rows span more slots than
 * the window instance keeps, 0 they do not, -1 no window kernel ran.  Returns the instance launched first (FitVariant of kernels.hpp: the codes
 * of vistaf_ftp_test_polyfit, then 11 win16, 12 win32, 13 win48, 14 win56, 15 win32_g4, 16 win48_g4, 17 win56_g4) or a negative error. */
int vistaf_ftp_test_polyfit_window(const float *z, const uint8_t *mask, int order, int iters, float c, int min_count, int min_mask_count, float *coef,
                                   float *resid, int B, int h, int w, int variant, int32_t *need_out, void *stream);

/* Two fits as the detrend chains them: the first (order1, min_mask_count1) of z into resid1, the second (order2, min_mask_count2) of resid1 under
 * the same mask into resid2; coef holds the second fit's coefficients.  variant 0: one chained launch where a column kernel takes the frame size
 * (window kernel and the chained plain-size kernel behind it), else two launches; 1 the chained window kernel alone; 2 two plain launches.
 * need_out and the return value as above. */
int vistaf_ftp_test_polyfit_chain(const float *z, const uint8_t *mask, int order1, int order2, int iters, float c, int min_count, int min_mask_count1,
                                  int min_mask_count2, float *coef, float *resid1, float *resid2, int B, int h, int w, int variant, int32_t *need_out,
                                  void *stream);

/* The instance variant 0 launches first for a batch of B frames of h x w: a window instance (11..17), or the plain one where the frame size has
 * no window; or a negative error.  Launches nothing. */
int vistaf_ftp_test_polyfit_window_instance(int B, int h, int w);

#ifdef __cplusplus
}
#endif
#endif
