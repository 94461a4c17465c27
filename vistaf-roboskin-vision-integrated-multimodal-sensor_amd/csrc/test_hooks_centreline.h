/* Test-only entry point of libvistaf_ftp.so for the centreline read-out (k_centreline.hip, include_ext/vistaf_centreline.h).  NOT part of the
 * drop-in boundary (include/vistaf_ftp.h), like everything in test_hooks.h.  Its ctypes signature is `_lib.CENTRELINE_TEST_SIGNATURES`;
 * tests/test_centrelines.py uses it to show that both storage tiers ran. */
#ifndef VISTAF_TEST_HOOKS_CENTRELINE_H
#define VISTAF_TEST_HOOKS_CENTRELINE_H
#include "../../include/vistaf_ftp.h"
#ifdef __cplusplus
extern "C" {
#endif
/* cl_box_in_lds of k_centreline.hip: 1 when the seven bit planes of a contact whose clipped box is bw x bh pixels -- (bh + 2) rows of
 * ceil(bw / 64) 64-bit words each -- fit the 60 KB of LDS the row kernel works in, 0 when that contact's planes live in the caller's
 * workspace instead (the same code, slower); VISTAF_E_INVALID for bw or bh outside 1..32767.  Launches nothing. */
int vistaf_ftp_test_centreline_tier(int bw, int bh);
#ifdef __cplusplus
}
#endif
#endif
