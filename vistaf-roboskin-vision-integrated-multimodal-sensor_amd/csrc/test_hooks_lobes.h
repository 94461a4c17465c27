/* Test-only entry point of libvistaf_ftp.so for the lobe read-out (k_lobes.hip, include_ext/vistaf_lobes.h).  NOT part of the drop-in
 * boundary (include/vistaf_ftp.h), like everything in test_hooks.h.  Its ctypes signature is `_lib.LOBES_TEST_SIGNATURES`;
 * tests/test_lobes.py uses it to show that both storage tiers ran. */
#ifndef VISTAF_TEST_HOOKS_LOBES_H
#define VISTAF_TEST_HOOKS_LOBES_H
#include "../../include/vistaf_ftp.h"
#ifdef __cplusplus
extern "C" {
#endif
/* lb_box_in_lds of k_lobes.hip: 1 when the tables of a contact whose clipped box is bw x bh pixels -- 12 bytes per pixel, 32 per possible
 * maximum (ceil(bw / 2) * ceil(bh / 2) of them) and 8 per slot of the sort (that number rounded up to a power of two) -- fit the 60 KB of
 * LDS the row kernel works in, 0 when that contact's tables live in the caller's workspace instead (the same code, slower);
 * VISTAF_E_INVALID for bw or bh outside 1..32767.  Launches nothing. */
int vistaf_ftp_test_lobes_tier(int bw, int bh);
#ifdef __cplusplus
}
#endif
#endif
