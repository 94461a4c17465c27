/* Test-only entry points of libvistaf_ftp.so for the long Gaussian blurs (k_basic.hip: k_gauss_strip against k_gauss_rows + k_gauss_cols[_lds]).
 * NOT part of the drop-in boundary (include/vistaf_ftp.h), like everything in test_hooks.h, which documents the session hook "gauss_strip" and
 * the hook vistaf_ftp_test_gauss that the first of these extends.  Their ctypes signatures are `_lib.GAUSS_STRIP_SIGNATURES`;
 * tests/test_gauss_strip.py runs them. */
#ifndef VISTAF_TEST_HOOKS_GAUSS_H
#define VISTAF_TEST_HOOKS_GAUSS_H
#include "../../include/vistaf_ftp.h"
#ifdef __cplusplus
extern "C" {
#endif
/* vistaf_ftp_test_gauss of test_hooks.h (same arguments, same checks, same result in dst) with a `variant`: 0 dispatch as a session does with
 * "gauss_strip" = 1 (what the plain hook runs), 1 the row and the column kernel whatever the tap count, 2 the strip kernel (k_gauss_strip: both
 * passes in one launch, a workgroup per frame and strip of 32 columns, the intermediate plane in LDS); VISTAF_E_INVALID before any launch where
 * vistaf_ftp_test_gauss_strip_fits says that the blur does not take it, or for another variant.  Returns the tier launched (GaussTier of
 * kernels.hpp: 1 the two kernels, 2 the strip kernel, 3 the one-kernel tile of up to 15 taps) or a negative error. */
int vistaf_ftp_test_gauss_variant(const float *src, float *dst, double sigma, int B, int h, int w, int variant, void *stream);

/* gauss_strip_fits of kernels.hpp: 1 when a blur of `ksize` taps of h x w frames takes the strip kernel (17 to 97 taps, and the plane of h x 32
 * floats plus a chunk of 32 rows of 32 + ksize - 1 columns, the row pitch rounded up to an odd multiple of four floats, plus two copies of
 * the taps of 104 floats each, within 48 KB of LDS), else 0; or a negative error.  Launches nothing. */
int vistaf_ftp_test_gauss_strip_fits(int h, int w, int ksize);

#ifdef __cplusplus
}
#endif
#endif
