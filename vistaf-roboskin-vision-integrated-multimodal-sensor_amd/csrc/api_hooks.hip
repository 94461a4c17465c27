// The vistaf_ftp_test_* entry points of libvistaf_ftp.so (csrc/test_hooks*.h; not part of the public header, not on the predict path): the
// production launchers, and the stage functions a session calls (stages.hpp), on device planes of the caller's, each dispatched or forced by a
// `variant`.  A hook checks its arguments, allocates its scratch, makes one call and waits for the stream.  None of them sees a session:
// vistaf_ftp_test_set, the one hook that reads the handle, is in api.hip.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "stages.hpp"
#include "mask_bits.hpp"       // mask_chain_fits

using namespace vf;
#include "test_hooks.h"
#include "test_hooks_masks.h"
#include "test_hooks_dft.h"
#include "test_hooks_gauss.h"
#include "test_hooks_fit.h"
#include "test_hooks_post.h"

namespace {

int refuse(const std::string &msg) { return set_error(VISTAF_E_INVALID, msg); }

// The temporaries of one hook call and the end of the call.  Whatever the call allocated is freed when it returns, on every path; an early
// return with buffers in hand first waits for the stream, which may hold launches that use them.
struct HookTemps {
    explicit HookTemps(void *stream) : st((hipStream_t)stream) {}
    HookTemps(const HookTemps &) = delete;
    ~HookTemps() { if (!mem.ptrs.empty()) (void)hipStreamSynchronize(st); mem.free_all(); }
    template <typename T>
    int alloc(T **p, size_t count) { return mem.alloc(p, count); }
    template <typename T>
    int upload(T **p, const std::vector<T> &host) { return mem.upload(p, host); }
    // one buffer cut into the regions layout(ScratchLayout &) takes; *bufs: the struct of pointers it returns
    template <class Bufs, class Layout>
    int carve(Bufs *bufs, Layout layout) { void *buf = nullptr; return ensure_carved(mem, buf, bufs, layout); }
    // after the last launch: the launch error, the wait for the stream, the frees; `tier`, or a negative VISTAF_E_* code
    int finish(int tier = 0)
    {
        const hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(st);
        mem.free_all();
        if (e1 != hipSuccess) return set_error(VISTAF_E_HIP, std::string("launch: ") + hipGetErrorString(e1));
        if (e2 != hipSuccess) return set_error(VISTAF_E_HIP, std::string("sync: ") + hipGetErrorString(e2));
        return tier;
    }
    const hipStream_t st;

private:
    DeviceAllocs mem;
};

// ---- the sizes a hook takes.  The limits differ on purpose.
// a plane the launchers index with 32-bit integers; min_side: the shortest side the kernels take
bool plane_ok(int B, int h, int w, int min_side = 1) { return B >= 1 && h >= min_side && w >= min_side && (size_t)h * w <= 0x7fffffffull; }
// a batch the launchers index as a whole with 32-bit integers, and the grid limits of a batch
bool batch_ok(int B, int h, int w) { return B >= 1 && B <= 65535 && h >= 1 && w >= 1 && (size_t)B * h * w <= 0x7fffffffull; }
// B is a grid's y extent; the pixel count leaves room for the launchers' rounding up to whole workgroups in int
bool frame_ok(int B, int h, int w) { return B >= 1 && B <= 65535 && h >= 1 && w >= 1 && (size_t)h * w <= 0x40000000ull; }
bool chain_shape_ok(int B, int h, int w, int ksize, int iters, int fused)
{
    return B >= 1 && h >= 1 && w >= 1 && (size_t)h * w <= 0x7fffffffull / 4 && ksize >= 1 && ksize <= 33 && iters >= 0 && iters <= 16 && (fused == 0 || fused == 1);
}
bool padded_ok(int h, int w, int pad, int Hf, int Wf) { return pad >= 0 && pad <= (1 << 20) && Hf == h + 2 * pad && Wf == w + 2 * pad && (size_t)Hf * Wf <= 0x7fffffffull; }
bool variant_012(int variant) { return variant >= 0 && variant <= 2; }
const char *const kVariant012 = "variant must be 0, 1 or 2";

// whether a call wants the scratch of the k_big.hip chain (big_scratch_bytes), by `variant`: 0 as vistaf_ftp_create allocates it (frames of
// 512 x 512 and more), 1 never, 2 always, refused where the chain does not take the batch
int chain_wanted(int variant, int h, int w, bool chain_ok, bool *want)
{
    if (!variant_012(variant)) return refuse(kVariant012);
    if (variant == 2 && !chain_ok) return refuse("variant 2: the k_big.hip chain does not take this batch");
    *want = variant == 2 || (variant == 0 && large_frame((size_t)h * w));
    return 0;
}

// A test element no cv shape gives: row i spans |i - k / 2| either side of the anchor (widest at the first and last row, the anchor alone in
// the middle).  Its rows are not nested towards the centre, so a pixel outside the image that wrongly took part would show.
RowSpanSE hourglass_se(int k)
{
    RowSpanSE se;
    se.k = k;
    for (int i = 0; i < 33; i++) { se.lo[i] = 1; se.hi[i] = -1; }
    for (int i = 0; i < k; i++) { const int a = std::abs(i - k / 2); se.lo[i] = (int8_t)(-a); se.hi[i] = (int8_t)a; }
    return se;
}

// ---- the demodulation hooks
// CarrierGeom <-> the two caller arrays of the hooks, in struct order: gd[7] = peak_x, peak_y, kx, ky, dpx, dpy, period;
// gi[10] = x0, y0, ph, pw, px_i, py_i, px_raw, py_raw, ok, keep_carrier
CarrierGeom geom_pack(const double *gd, const int32_t *gi)
{
    CarrierGeom g;
    g.peak_x = gd[0]; g.peak_y = gd[1]; g.kx = gd[2]; g.ky = gd[3]; g.dpx = gd[4]; g.dpy = gd[5]; g.period = gd[6];
    g.x0 = gi[0]; g.y0 = gi[1]; g.ph = gi[2]; g.pw = gi[3]; g.px_i = gi[4]; g.py_i = gi[5]; g.px_raw = gi[6]; g.py_raw = gi[7];
    g.ok = gi[8]; g.keep_carrier = gi[9];
    return g;
}
void geom_unpack(const CarrierGeom &g, double *gd, int32_t *gi)
{
    gd[0] = g.peak_x; gd[1] = g.peak_y; gd[2] = g.kx; gd[3] = g.ky; gd[4] = g.dpx; gd[5] = g.dpy; gd[6] = g.period;
    gi[0] = g.x0; gi[1] = g.y0; gi[2] = g.ph; gi[3] = g.pw; gi[4] = g.px_i; gi[5] = g.py_i; gi[6] = g.px_raw; gi[7] = g.py_raw;
    gi[8] = g.ok; gi[9] = g.keep_carrier;
}
// the `staged` flag of the demodulation launchers for a hook's `variant`: 0 as a session dispatches (staged where dft_staged_fits says so), 1 the
// kernels that read global memory, 2 the staged kernel of stage `bit`, an error where the shape does not take it
int dft_hook_variant(int variant, int bit, int h, int w, int ph, int pw, bool per_frame, bool *staged)
{
    if (!variant_012(variant)) return refuse(kVariant012);
    if (variant == 2 && !(dft_staged_fits(h, w, ph, pw, per_frame) & bit)) return refuse("variant 2: the staged kernel does not take this shape");
    *staged = variant != 1;
    return 0;
}
// the table strides of both directions against what they stride over
bool table_strides_ok(size_t tab_stride_x, size_t tab_stride_y, int h, int w, int ph, int pw)
{
    return (tab_stride_x == 0) == (tab_stride_y == 0) && (!tab_stride_x || (tab_stride_x >= (size_t)w * pw && tab_stride_y >= (size_t)ph * h));
}
const char *const kStrideRefusal = "a stride is smaller than what it strides over, or only one table stride is zero";

// ---- the back-end hooks
bool sigma_ok(double sigma) { return sigma >= 0 && sigma <= 1e6 && gauss_fits(sigma > 0 ? sigma : 1.0); }
bool curve_ok(int type, double a, double b, double c) { return type >= 0 && type <= 5 && a == a && b == b && c == c; }
PostParams hook_post_params(double mm_per_px, double depth_eps_mm, double period_px, const Curve &force)
{
    PostParams pp;
    pp.mm_per_px = mm_per_px; pp.depth_eps_mm = depth_eps_mm; pp.period_px = period_px; pp.force_curve = force;
    return pp;
}
// the session's taps for `sigma` (none for sigma == 0)
std::vector<float> taps_of(double sigma) { return sigma > 0 ? gauss_taps(sigma) : std::vector<float>(); }

}  // namespace

extern "C" {

// ---- the selection, IRLS fit and plain blur launchers (csrc/test_hooks.h, test_hooks_fit.h, test_hooks_gauss.h)
int vistaf_ftp_test_select(const float *vals, const uint8_t *mask, size_t mask_stride, const float *le_thr, int use_abs, const float *reqs, int nreq,
                           float *out, int *counts, int B, int P, int variant, void *stream)
{
    if (!vals || !mask || !reqs || !out || B < 1 || P < 1 || nreq < 1 || (mask_stride != 0 && mask_stride != (size_t)P)) return refuse("bad argument");
    if (variant < 0 || variant > 3) return refuse("variant must be 0, 1, 2 or 3");
    bool want = false;
    TRY(chain_wanted(variant == 3 ? 1 : variant, 1, P, nreq <= 4 && big_frames(B, P), &want));
    HookTemps tmp(stream);
    uint8_t *scratch = nullptr;
    if (want) TRY(tmp.alloc(&scratch, big_scratch_bytes(B, 1, P)));
    launch_select(vals, mask, mask_stride, le_thr, use_abs != 0, reqs, nreq, out, counts, B, P, tmp.st, scratch, variant != 3);
    return tmp.finish();
}

int vistaf_ftp_test_select_instance(int B, int P, int nreq, int variant)
{
    if (B < 1 || P < 1 || nreq < 1 || variant < 0 || variant > 3) return refuse("bad argument");
    bool want = false;
    TRY(chain_wanted(variant == 3 ? 1 : variant, 1, P, nreq <= 4 && big_frames(B, P), &want));
    return select_variant(B, P, nreq, want, variant != 3);
}

int vistaf_ftp_test_select_chained(const float *vals, const uint8_t *mask, size_t mask_stride, int use_abs, const float *reqs, int nreq, float *out,
                                   int *counts, int B, int P, void *stream)
{
    if (!vals || !mask || !reqs || !out || B < 1 || P < 1 || nreq < 1 || nreq > 4 || (mask_stride != 0 && mask_stride != (size_t)P))
        return refuse("bad argument");
    float *outs[4] = {out, out + B, out + 2 * (size_t)B, out + 3 * (size_t)B};
    const int inst = launch_select_chained(vals, mask, mask_stride, use_abs != 0, reqs, nreq, outs, counts, B, P, (hipStream_t)stream);
    if (inst < 0) return refuse("no resident instance takes this plane size");
    return HookTemps(stream).finish(inst);
}

int vistaf_ftp_test_polyfit(const float *z, const uint8_t *mask, int order, int iters, float c, int min_count, int min_mask_count, float *coef,
                            float *resid, int B, int h, int w, int variant, void *stream)
{
    if (!z || !mask || !coef || !resid || !plane_ok(B, h, w) || order < 1 || order > 2 || iters < 1) return refuse("bad argument");
    bool want = false;
    TRY(chain_wanted(variant, h, w, big_frames(B, h * w), &want));
    HookTemps tmp(stream);
    uint8_t *scratch = nullptr;
    if (want) TRY(tmp.alloc(&scratch, big_scratch_bytes(B, h, w)));
    const int inst = polyfit_variant(B, h, w, scratch != nullptr);
    launch_robust_polyfit(z, mask, order, iters, c, min_count, min_mask_count, coef, resid, B, h, w, tmp.st, scratch);
    return tmp.finish(inst);
}

static int fit_window_hook(const float *z, const uint8_t *mask, int order, int iters, float c, int min_count, int min_mask_count, float *coef, float *resid,
                           const FitSecond *second, int B, int h, int w, int variant, int32_t *need_out, void *stream)
{
    if (!z || !mask || !coef || !resid || (second && !second->resid_out) || !plane_ok(B, h, w) || order < 1 || order > 2 ||
        (second && (second->order < 1 || second->order > 2)) || iters < 1)
        return refuse("bad argument");
    if (!variant_012(variant)) return refuse(kVariant012);
    const bool big = large_frame((size_t)h * w);      // the chain scratch as vistaf_ftp_create allocates it
    if (variant == 1 && polyfit_window_variant(B, h, w, big) < 0) return refuse("variant 1: no window instance for this frame size");
    HookTemps tmp(stream);
    uint8_t *scratch = nullptr;
    int32_t *need = nullptr;
    if (big) TRY(tmp.alloc(&scratch, big_scratch_bytes(B, h, w)));
    TRY(tmp.alloc(&need, (size_t)B));
    hipError_t e = hipMemsetAsync(need, 0xff, (size_t)B * sizeof(int32_t), tmp.st);       // -1: no window kernel ran
    const int inst = launch_robust_polyfit_window(z, mask, order, iters, c, min_count, min_mask_count, coef, resid, second, need, Tiers().fit_window != 0, variant,
                                                  B, h, w, tmp.st, scratch);
    if (e == hipSuccess && need_out) e = hipMemcpyAsync(need_out, need, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, tmp.st);
    TRY(tmp.finish());
    return e != hipSuccess ? set_error(VISTAF_E_HIP, std::string("need: ") + hipGetErrorString(e)) : inst;
}
int vistaf_ftp_test_polyfit_window(const float *z, const uint8_t *mask, int order, int iters, float c, int min_count, int min_mask_count, float *coef,
                                   float *resid, int B, int h, int w, int variant, int32_t *need_out, void *stream)
{
    return fit_window_hook(z, mask, order, iters, c, min_count, min_mask_count, coef, resid, nullptr, B, h, w, variant, need_out, stream);
}
int vistaf_ftp_test_polyfit_chain(const float *z, const uint8_t *mask, int order1, int order2, int iters, float c, int min_count, int min_mask_count1,
                                  int min_mask_count2, float *coef, float *resid1, float *resid2, int B, int h, int w, int variant, int32_t *need_out, void *stream)
{
    const FitSecond second = {order2, min_mask_count2, resid2};
    return fit_window_hook(z, mask, order1, iters, c, min_count, min_mask_count1, coef, resid1, &second, B, h, w, variant, need_out, stream);
}
int vistaf_ftp_test_polyfit_window_instance(int B, int h, int w)
{
    if (!plane_ok(B, h, w)) return refuse("bad argument");
    const bool big = large_frame((size_t)h * w);
    const int plain = polyfit_variant(B, h, w, big), win = polyfit_window_variant(B, h, w, big);
    return win >= 0 ? win : plain;
}

int vistaf_ftp_test_gauss_variant(const float *src, float *dst, double sigma, int B, int h, int w, int variant, void *stream)
{
    if (!src || !dst || src == dst || B < 1 || h < 1 || w < 1 || !(sigma > 0)) return refuse("bad argument");
    if (!variant_012(variant)) return refuse(kVariant012);
    if (!gauss_fits(sigma)) return gauss_refused();
    const std::vector<float> f = gauss_taps(sigma);
    if (variant == 2 && !gauss_strip_fits(h, w, (int)f.size())) return refuse("variant 2: the strip kernel does not take this blur");
    HookTemps tmp(stream);
    float *taps = nullptr, *plane = nullptr;
    TRY(tmp.upload(&taps, f));
    TRY(tmp.alloc(&plane, (size_t)B * h * w));
    return tmp.finish(launch_gauss_blur(src, plane, dst, taps, (int)f.size(), B, h, w, tmp.st, Tiers().gauss_strip != 0, variant));
}
int vistaf_ftp_test_gauss_strip_fits(int h, int w, int ksize)
{
    if (h < 1 || w < 1 || ksize < 1 || !(ksize & 1)) return refuse("bad argument");
    return gauss_strip_fits(h, w, ksize) ? 1 : 0;
}
int vistaf_ftp_test_gauss(const float *src, float *dst, double sigma, int B, int h, int w, void *stream)
{
    const int rc = vistaf_ftp_test_gauss_variant(src, dst, sigma, B, h, w, 0, stream);
    return rc < 0 ? rc : 0;
}

// ---- the mask topology launchers (chamfer, labelling, largest component, blob filter) and launch_morph
// The two chamfer hooks.  force: the one-wave two-pass kernel, which has no instance for every width; otherwise the dispatch, whose tier is
// the return value
static int chamfer_hook(const uint8_t *mask, int pair, int invert, float *dist_a, float *dist_b, int B, int h, int w, int cap_px, void *stream, bool force)
{
    if (!mask || !dist_a || (pair && !dist_b) || !plane_ok(B, h, w) || cap_px < 0) return refuse("bad argument");
    if (force && w > 512 && !(pair && w <= 1280)) return refuse("no two-pass instance for this width");
    const int tier = force ? 0 : pair ? chamfer_pair_tier(B, h, w, cap_px) : chamfer_tier(h, w, cap_px);
    const size_t n = (size_t)B * h * w;
    HookTemps tmp(stream);
    int32_t *tmp_a = nullptr, *tmp_b = nullptr;
    TRY(tmp.alloc(&tmp_a, n));
    if (pair) TRY(tmp.alloc(&tmp_b, n));
    if (pair) launch_chamfer_pair(mask, tmp_a, dist_a, tmp_b, dist_b, B, h, w, cap_px, tmp.st, force);
    else launch_chamfer(mask, invert != 0, tmp_a, dist_a, B, h, w, cap_px, tmp.st, force);
    return tmp.finish(tier);
}
int vistaf_ftp_test_chamfer(const uint8_t *mask, int pair, int invert, float *dist_a, float *dist_b, int B, int h, int w, int cap_px, void *stream)
{
    return chamfer_hook(mask, pair, invert, dist_a, dist_b, B, h, w, cap_px, stream, true);
}
int vistaf_ftp_test_chamfer_dispatch(const uint8_t *mask, int pair, int invert, float *dist_a, float *dist_b, int B, int h, int w, int cap_px, void *stream)
{
    return chamfer_hook(mask, pair, invert, dist_a, dist_b, B, h, w, cap_px, stream, false);
}

int vistaf_ftp_test_cc_label(const uint8_t *mask, int32_t *labels, int B, int h, int w, int variant, void *stream)
{
    if (!mask || !labels || !plane_ok(B, h, w)) return refuse("bad argument");
    if (variant < 0 || variant > 1) return refuse("variant must be 0 or 1");
    launch_cc_label(mask, labels, B, h, w, (hipStream_t)stream, variant == 1);
    return HookTemps(stream).finish(cc_label_tier(h, w, variant == 1));
}

int vistaf_ftp_test_cc_largest(const int32_t *labels, const uint8_t *and_static, uint8_t *out, int B, int P, int variant, void *stream)
{
    if (!labels || !out || B < 1 || P < 1) return refuse("bad argument");
    if (!variant_012(variant)) return refuse(kVariant012);
    HookTemps tmp(stream);
    int32_t *area = nullptr;
    unsigned long long *best = nullptr;
    TRY(tmp.alloc(&area, (size_t)B * P));
    TRY(tmp.alloc(&best, (size_t)B));
    launch_cc_largest(labels, area, best, and_static, out, B, P, tmp.st, variant);
    return tmp.finish(cc_largest_tier(B, P, true, variant));
}

int vistaf_ftp_test_blob_filter(float *depth_inout, const uint8_t *cand, const int32_t *labels, const float *gmax, double min_peak_mm, double rel_frac,
                                uint8_t *kept, int B, int P, void *stream)
{
    if (!depth_inout || !cand || !labels || !gmax || !kept || B < 1 || P < 1) return refuse("bad argument");
    HookTemps tmp(stream);
    unsigned int *peak_bits = nullptr;
    TRY(tmp.alloc(&peak_bits, (size_t)B * P));
    launch_blob_filter(depth_inout, cand, labels, peak_bits, (const unsigned int *)gmax, min_peak_mm, rel_frac, kept, B, P, tmp.st);
    return tmp.finish();
}

int vistaf_ftp_test_morph(const uint8_t *src, uint8_t *dst, int B, int h, int w, int shape, int kx, int ky, int dilate, const uint8_t *and_static,
                          const uint8_t *and_frame, int tier, void *stream)
{
    if (!src || !dst || src == dst || !batch_ok(B, h, w) || h > 65535) return refuse("bad argument");
    if (shape < 0 || shape > 2) return refuse("shape must be 0 (ellipse), 1 (rectangle) or 2 (hourglass)");
    if (shape == 2 && (kx < 3 || kx > 33 || kx % 2 == 0)) return refuse("hourglass size must be odd, 3..33");
    if (shape == 0 && (kx < 1 || kx > 33)) return refuse("ellipse size must be 1..33");
    if (shape == 1 && (kx < 1 || kx > 127 || ky < 1 || ky > 33)) return refuse("rectangle must be 1..127 wide and 1..33 tall");
    if (tier < 0 || tier > 4) return refuse("tier must be 0..4");
    const RowSpanSE se = shape == 0 ? ellipse_se(kx) : shape == 1 ? rect_se(odd_up(kx), odd_up(ky)) : hourglass_se(kx);
    if (tier == MORPH_PREFIX && w >= 65536) return refuse("tier 2: the uint16 row counts take rows shorter than 65536");
    if (tier == MORPH_BITS && !morph_bits_ok(se, h, w)) return refuse("tier 3: the bit-plane kernel does not take this frame or element");
    const bool scratch = tier == 0 || tier == MORPH_PREFIX;
    const int ran = (tier == 0 || tier == 4) ? morph_tier(se, h, w, scratch) : tier;
    HookTemps tmp(stream);
    uint16_t *prefix = nullptr;
    if (scratch) TRY(tmp.alloc(&prefix, (size_t)B * h * w));
    launch_morph(src, dst, B, h, w, se, dilate != 0, and_static, and_frame, tmp.st, prefix, (tier == 0 || tier == 4) ? 0 : tier);
    return tmp.finish(ran);
}

// ---- the three binary-mask chains (csrc/test_hooks_masks.h): the session's own functions
int vistaf_ftp_test_mask_chain_fits(int chain, int h, int w, int ksize, int nops, int margin_px)
{
    if (ksize < 1 || ksize > 33) return refuse("bad argument");
    RowSpanSE se;
    TRY(make_se(ksize, &se, chain != MCH_CONTACT));
    return mask_chain_fits(chain, h, w, se, nops, (float)margin_px) ? 1 : 0;
}

int vistaf_ftp_test_bad_chain(const float *img, const float *grad, const uint8_t *valid, const float *thr_hi, const float *thr_g, int ksize, int iters,
                              uint8_t *bad1, int *bad_count, int B, int h, int w, int fused, void *stream)
{
    if (!img || !grad || !valid || !thr_hi || !thr_g || !bad1 || !bad_count || !chain_shape_ok(B, h, w, ksize, iters, fused)) return refuse("bad argument");
    RowSpanSE se;
    TRY(make_se(ksize, &se));
    HookTemps tmp(stream);
    uint8_t *bad0 = nullptr;
    TRY(tmp.alloc(&bad0, (size_t)B * h * w));
    const int tier = bad_mask_chain(img, grad, valid, thr_hi, thr_g, se, ksize, iters, bad0, bad1, bad_count, fused != 0, B, h, w, tmp.st);
    return tier < 0 ? tier : tmp.finish(tier);
}

int vistaf_ftp_test_reliable_chain(const float *quality, const uint8_t *roi, const float *amp_thr, int close_ksize, int close_iters, int margin_px,
                                   uint8_t *rel0, uint8_t *reliable, int *rel_count, int32_t *status, int B, int h, int w, int fused, void *stream)
{
    if (!quality || !roi || !amp_thr || !rel0 || !reliable || !rel_count || !status || !chain_shape_ok(B, h, w, close_ksize, close_iters, fused) ||
        margin_px < 0 || margin_px > 1024)
        return refuse("bad argument");
    RowSpanSE se;
    TRY(make_se(close_ksize, &se));
    const size_t n = (size_t)B * h * w;
    HookTemps tmp(stream);
    ReliableScratch ws;
    TRY(tmp.carve(&ws, [&](ScratchLayout &L) {
        return ReliableScratch{L.take<uint8_t>(n), L.take<uint8_t>(n), L.take<int32_t>(n), L.take<int32_t>(n), L.take<int32_t>(n), L.take<float>(n),
                               L.take<unsigned long long>((size_t)B), L.take<uint16_t>(n)};
    }));
    const int tier = reliable_mask_chain(quality, roi, amp_thr, se, close_iters, margin_px, ws, false, rel0, reliable, rel_count, status, fused != 0, B, h, w, tmp.st);
    return tier < 0 ? tier : tmp.finish(tier);
}

int vistaf_ftp_test_contact_chain(const float *resid, const uint8_t *reliable, const float *thr3, const int *rel_count, double min_frac, double max_frac,
                                  int ksize, int iters, float *thr_used, uint8_t *contact_d, uint8_t *background, int *bg_count, int B, int h, int w,
                                  int fused, void *stream)
{
    if (!resid || !reliable || !thr3 || !rel_count || !thr_used || !contact_d || !background || !bg_count || !chain_shape_ok(B, h, w, ksize, iters, fused))
        return refuse("bad argument");
    RowSpanSE se;
    TRY(make_se(ksize, &se, false));
    const size_t n = (size_t)B * h * w;
    HookTemps tmp(stream);
    ContactScratchPlanes ws;
    int *contact_count = nullptr;
    TRY(tmp.carve(&ws, [&](ScratchLayout &L) { return ContactScratchPlanes{L.take<uint8_t>(n), L.take<uint8_t>(n), L.take<uint16_t>(n)}; }));
    TRY(tmp.alloc(&contact_count, (size_t)B));
    const int tier = contact_mask_chain(resid, reliable, thr3, rel_count, min_frac, max_frac, se, iters, ws, contact_count, thr_used, contact_d, background,
                                        bg_count, fused != 0, B, h, w, tmp.st);
    return tier < 0 ? tier : tmp.finish(tier);
}

// ---- the unwrap launcher (consistency check, rank kernels, floods, replay / tree)
int vistaf_ftp_test_unwrap(const float *wrapped, const float *quality, const uint8_t *mask, float *unwrapped, int32_t *parent, int32_t *need,
                           int32_t *status, int B, int h, int w, int variant, void *stream)
{
    if (!wrapped || !quality || !mask || !unwrapped || !parent || !status || !plane_ok(B, h, w, 8)) return refuse("bad argument");
    if (!variant_012(variant)) return refuse(kVariant012);
    if (variant == 0 && (!need || !unwrap_fast_supported(h, w)))
        return refuse("variant 0: need is null, or the consistency check does not take this shape");
    HookTemps tmp(stream);
    uint8_t *scratch = nullptr;
    TRY(tmp.alloc(&scratch, unwrap_scratch_bytes(B, h, w)));
    launch_unwrap(wrapped, quality, mask, unwrapped, parent, scratch, status, B, h, w, tmp.st, nullptr, nullptr, variant == 2, variant == 0 ? need : nullptr);
    return tmp.finish(unwrap_tier(h, w, variant == 2));
}

// ---- the Telea launchers (window tiers, cluster front end, big-cluster march, whole-frame kernel)
int vistaf_ftp_test_inpaint(float *img_inout, const uint8_t *bad, int range, int round_u8, int32_t *fb, int32_t *status, int B, int h, int w, int variant,
                            void *stream)
{
    if (!img_inout || !bad || !fb || !status || !plane_ok(B, h, w, 8) || range < 1 || range > 100) return refuse("bad argument");
    if (variant < 0 || variant > 6) return refuse("variant must be 0 .. 6");
    if (round_u8 && variant != 1) return refuse("round_u8: the whole-frame kernel (variant 1) only");
    if (variant == 2 && !inpaint_window_mw_supported(range)) return refuse("variant 2: the 16-wave window kernel does not take this range");
    if ((variant == 5 || variant == 6) && !inpaint_clusters_supported(range)) return refuse("variants 5 and 6: the cluster kernels do not take this range");
    const bool dispatch = variant == 0 || variant >= 5;
    const size_t n_tel = variant <= 1 || variant >= 5 ? inpaint_scratch_bytes(B, h, w) : 0, n_cl = dispatch ? inpaint_cl_scratch_bytes(B, h, w) : 0,
                 n_win = variant != 1 ? inpaint_win_scratch_bytes(B) : 0;
    HookTemps tmp(stream);
    InpaintBuffers buf;
    TRY(tmp.carve(&buf, [&](ScratchLayout &L) {
        return InpaintBuffers{L.take<uint8_t>(n_tel), L.take<uint8_t>(n_cl), L.take<uint8_t>(n_win), L.take<int32_t>((size_t)B)};
    }));
    const int32_t *only = nullptr;
    if (dispatch) {
        Tiers tiers;                                        // the defaults of a session
        if (variant >= 5) tiers.inpaint = 0;
        if (variant == 6) tiers.big_queue_lds = 0;
        only = inpaint_dispatch(img_inout, bad, range, tiers, true, buf, status, B, h, w, tmp.st, nullptr);
    } else if (variant == 1) launch_inpaint_telea(img_inout, bad, range, buf.scratch, status, nullptr, B, h, w, tmp.st, round_u8 != 0);
    else only = launch_inpaint_window(img_inout, bad, range, buf.win_scratch, B, h, w, tmp.st, nullptr, false, false, variant == 2 ? WNT_MW : variant == 3 ? WNT_FIRST : WNT_ALL);
    if (only) (void)hipMemcpyAsync(fb, only, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, tmp.st);
    return tmp.finish();
}

int vistaf_ftp_test_scratch_regions(const char *stage, int B, int h, int w, int range, int cap, char *names, size_t *offset, size_t *bytes, size_t *align,
                                    size_t *total)
{
    if (!stage || !names || !offset || !bytes || !align || !total || B < 1 || h < 1 || w < 1 || range < 1 || cap < 1) return refuse("bad argument");
    const std::string s(stage);
    std::vector<ScratchRegion> regions;
    if (s == "unwrap") *total = unwrap_scratch_bytes(B, h, w, &regions);
    else if (s == "telea") *total = telea_scratch_bytes(B, h, w, &regions);
    else if (s == "inpaint_big") *total = inpaint_big_scratch_bytes(B, h, w, range, &regions);
    else if (s == "inpaint_cl") *total = inpaint_cl_scratch_bytes(B, h, w, &regions);
    else if (s == "inpaint_win") *total = inpaint_win_scratch_bytes(B, &regions);
    else if (s == "big") *total = big_scratch_bytes(B, h, w, &regions);
    else if (s == "tstats") *total = tstats_scratch_bytes(h, w, &regions);
    else if (s == "pressure") *total = pressure_scratch_bytes(B, h, w, range, &regions);      // range: pad_px
    if (regions.empty()) return refuse("unknown stage: " + s);
    if ((int)regions.size() > cap) return refuse("more regions than cap");
    for (size_t i = 0; i < regions.size(); i++) {
        snprintf(names + 32 * i, 32, "%s", regions[i].name ? regions[i].name : "");
        offset[i] = regions[i].offset; bytes[i] = regions[i].bytes; align[i] = regions[i].align;
    }
    return (int)regions.size();
}

// ---- the demodulation launchers (k_dft.hip, k_dft_tables.hip; csrc/test_hooks.h, test_hooks_dft.h) on planes and tables of the caller's
int vistaf_ftp_test_dft_full_mag(const float *planes, const void *Ex_half, const void *Ey_full, void *tmp, double *mag, int B, int h, int w, int Hf,
                                 int Wf, void *stream)
{
    if (!planes || !Ex_half || !Ey_full || !tmp || !mag || B < 1 || h < 1 || w < 1 || Hf < h || Wf < w) return refuse("bad argument");
    launch_dft_full_mag(planes, nullptr, (const double2 *)Ex_half, (const double2 *)Ey_full, (double2 *)tmp, mag, B, h, w, Hf, Wf, (hipStream_t)stream);
    return launch_ok("launch_dft_full_mag");
}

int vistaf_ftp_test_top_peaks(const double *mag, int B, int Hf, int Wf, int dc, int npeaks, double *out, void *stream)
{
    if (!mag || !out || !batch_ok(B, Hf, Wf) || dc < 0 || npeaks < 1 || npeaks > 64 || (size_t)Hf * Wf < (size_t)npeaks) return refuse("bad argument");
    launch_top_peaks(mag, B, Hf, Wf, dc, npeaks, out, (hipStream_t)stream);
    return HookTemps(stream).finish();
}

int vistaf_ftp_test_carrier_choose(const double *peaks, int npk, const double *mag, int Hf, int Wf, int bw, double max_dy_frac, double *gd, int32_t *gi,
                                   int B, void *stream)
{
    if (!peaks || !mag || !gd || !gi || !batch_ok(B, Hf, Wf) || npk < 1 || npk > 64 || bw < 0 || bw > (1 << 20) || !(max_dy_frac >= 0.0) ||
        !(max_dy_frac <= 1e6))
        return refuse("bad argument");
    HookTemps tmp(stream);
    // the kernel reads the magnitude plane at the listed positions: a list that points outside the plane is refused, not launched
    std::vector<double> pk((size_t)B * 192);
    HIPCHK(hipStreamSynchronize(tmp.st));
    HIPCHK(hipMemcpy(pk.data(), peaks, pk.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int b = 0; b < B; b++)
        for (int i = 0; i < npk; i++) {
            const double x = pk[(size_t)b * 192 + 3 * i], y = pk[(size_t)b * 192 + 3 * i + 1];
            if (!(x >= 0.0 && x < (double)Wf && y >= 0.0 && y < (double)Hf)) return refuse("a listed peak lies outside the plane");
        }
    CarrierGeom *geom = nullptr;
    TRY(tmp.alloc(&geom, (size_t)B));
    launch_carrier_choose(peaks, npk, mag, Hf, Wf, bw, max_dy_frac, geom, B, tmp.st);
    std::vector<CarrierGeom> g((size_t)B);
    const hipError_t e0 = hipGetLastError();
    const hipError_t e1 = e0 == hipSuccess ? hipMemcpyAsync(g.data(), geom, g.size() * sizeof(CarrierGeom), hipMemcpyDeviceToHost, tmp.st) : e0;
    const int rc = tmp.finish();
    if (e1 != hipSuccess) return set_error(VISTAF_E_HIP, std::string("launch_carrier_choose: ") + hipGetErrorString(e1));
    if (rc) return rc;
    for (int b = 0; b < B; b++) geom_unpack(g[b], gd + 7 * (size_t)b, gi + 10 * (size_t)b);
    return 0;
}

int vistaf_ftp_test_build_tables(const double *gd, const int32_t *gi, int geom_stride, int B, int h, int w, int pad, int Hf, int Wf, int pmax, int pair,
                                 void *Ex, void *Ey, void *Gx, void *Gy, float *win, void *stream)
{
    if (!gd || !gi || !Ex || !Ey || !Gx || !Gy || (pair && !win) || !batch_ok(B, h, w) || !padded_ok(h, w, pad, Hf, Wf) || pmax < 1 || pmax > 4096 ||
        (geom_stride != 0 && geom_stride != 1) || (size_t)std::max(std::max(h, w), pmax) * pmax > 0x7fffffffull)
        return refuse("bad argument");
    std::vector<CarrierGeom> g((size_t)(geom_stride ? B : 1));
    for (size_t b = 0; b < g.size(); b++) g[b] = geom_pack(gd + 7 * b, gi + 10 * b);
    HookTemps tmp(stream);
    CarrierGeom *geom = nullptr;
    float *hann = nullptr;
    TRY(tmp.upload(&geom, g));
    if (pair) TRY(tmp.upload(&hann, hann_table(pmax)));      // as vistaf_ftp_predict_pairs uploads it
    launch_build_tables(geom, geom_stride, (double2 *)Ex, (double2 *)Ey, (double2 *)Gx, (double2 *)Gy, (size_t)w * pmax, (size_t)h * pmax, B, h, w, pad, Hf,
                        Wf, pmax, tmp.st, hann, pair ? win : nullptr);
    return tmp.finish();
}

int vistaf_ftp_test_build_full_tables(void *Exf, void *Eyf, int h, int w, int pad, int Hf, int Wf, void *stream)
{
    if (!Exf || !Eyf || !batch_ok(1, h, w) || !padded_ok(h, w, pad, Hf, Wf)) return refuse("bad argument");
    launch_build_full_tables((double2 *)Exf, (double2 *)Eyf, h, w, pad, Hf, Wf, (hipStream_t)stream);
    return HookTemps(stream).finish();
}

int vistaf_ftp_test_dft_forward(const float *iw, const float *mu, const void *Ex, const void *Ey, size_t tab_stride_x, size_t tab_stride_y, const float *win,
                                int win_stride, void *T, void *patch, int patch_stride, int B, int h, int w, int ph, int pw, void *stream)
{
    return vistaf_ftp_test_dft_forward_v(iw, mu, Ex, Ey, tab_stride_x, tab_stride_y, win, win_stride, T, patch, patch_stride, B, h, w, ph, pw, 0, stream);
}

int vistaf_ftp_test_dft_forward_v(const float *iw, const float *mu, const void *Ex, const void *Ey, size_t tab_stride_x, size_t tab_stride_y, const float *win,
                                  int win_stride, void *T, void *patch, int patch_stride, int B, int h, int w, int ph, int pw, int variant, void *stream)
{
    if (!iw || !Ex || !Ey || !win || !T || !patch || !batch_ok(B, h, w) || ph < 1 || pw < 1 || ph > 4096 || pw > 4096 || (size_t)B * h * pw > 0x7fffffffull)
        return refuse("bad argument");
    if (!table_strides_ok(tab_stride_x, tab_stride_y, h, w, ph, pw) || (win_stride != 0 && win_stride < ph * pw) || patch_stride < ph * pw)
        return refuse(kStrideRefusal);
    bool staged;
    TRY(dft_hook_variant(variant, DFT_STAGED_FWD1, h, w, ph, pw, tab_stride_x != 0, &staged));
    launch_dft_forward(iw, mu, (const double2 *)Ex, (const double2 *)Ey, tab_stride_x, tab_stride_y, win, (double2 *)T, (double2 *)patch, patch_stride, B, h, w,
                       ph, pw, (hipStream_t)stream, win_stride, staged);
    return HookTemps(stream).finish();
}

int vistaf_ftp_test_dft_inverse(const void *patch, int patch_stride, const void *Gx, const void *Gy, size_t tab_stride_x, size_t tab_stride_y, void *Q, void *field,
                                float *amp, const void *cref, const float *amp_ref, size_t ref_stride, float *prod, float *wrapped, const int32_t *gi_or_null,
                                int B, int h, int w, int ph, int pw, void *stream)
{
    return vistaf_ftp_test_dft_inverse_v(patch, patch_stride, Gx, Gy, tab_stride_x, tab_stride_y, Q, field, amp, cref, amp_ref, ref_stride, prod, wrapped,
                                         gi_or_null, B, h, w, ph, pw, 0, stream);
}

int vistaf_ftp_test_dft_staged_fits(int h, int w, int ph, int pw, int per_frame_tables)
{
    if (h < 1 || w < 1 || ph < 1 || pw < 1) return refuse("bad argument");
    return dft_staged_fits(h, w, ph, pw, per_frame_tables != 0);
}

int vistaf_ftp_test_dft_inverse_v(const void *patch, int patch_stride, const void *Gx, const void *Gy, size_t tab_stride_x, size_t tab_stride_y, void *Q,
                                  void *field, float *amp, const void *cref, const float *amp_ref, size_t ref_stride, float *prod, float *wrapped,
                                  const int32_t *gi_or_null, int B, int h, int w, int ph, int pw, int variant, void *stream)
{
    if (!patch || !Gx || !Gy || !Q || !amp || (cref && (!amp_ref || !prod || !wrapped)) || !batch_ok(B, h, w) || ph < 1 || pw < 1 || ph > 4096 ||
        pw > 4096 || (size_t)B * ph * w > 0x7fffffffull)
        return refuse("bad argument");
    if (!table_strides_ok(tab_stride_x, tab_stride_y, h, w, ph, pw) || patch_stride < ph * pw || (ref_stride != 0 && ref_stride < (size_t)h * w))
        return refuse(kStrideRefusal);
    bool staged;
    TRY(dft_hook_variant(variant, DFT_STAGED_INV2, h, w, ph, pw, tab_stride_x != 0, &staged));
    HookTemps tmp(stream);
    CarrierGeom *geom = nullptr;
    if (gi_or_null) {
        const double zeros[7] = {0, 0, 0, 0, 0, 0, 0};
        std::vector<CarrierGeom> g((size_t)B);
        for (int b = 0; b < B; b++) g[b] = geom_pack(zeros, gi_or_null + 10 * (size_t)b);
        TRY(tmp.upload(&geom, g));
    }
    launch_dft_inverse((const double2 *)patch, patch_stride, (const double2 *)Gx, (const double2 *)Gy, tab_stride_x, tab_stride_y, (double2 *)Q, (double2 *)field, amp,
                       (const double2 *)cref, amp_ref, ref_stride, prod, wrapped, B, h, w, ph, pw, tmp.st, geom, staged);
    return tmp.finish();
}

// ---- csrc/test_hooks_post.h: the back end of post_demod (smoothing, sign flip, hole glue, composition and mm curve, blob filter, force tail,
// output copy).  The three stages with tiers are the session's own functions; `variant` 0 passes them the default of the tier's flag, 1 and 2
// switch it off and on.
int vistaf_ftp_test_smooth_reliable(const float *detr, const float *bg_med, const uint8_t *reliable, double sigma, float *hmap, int B, int h, int w,
                                    int variant, void *stream)
{
    if (!detr || !bg_med || !reliable || !hmap || !frame_ok(B, h, w) || !sigma_ok(sigma)) return refuse("bad argument");
    if (!variant_012(variant)) return refuse(kVariant012);
    const std::vector<float> f = taps_of(sigma);
    const int k = (int)f.size();
    if (variant == 2 && !fuses(true, k)) return refuse("variant 2: the tile kernel takes 1..15 taps");
    const size_t n = (size_t)B * h * w;
    HookTemps tmp(stream);
    float *taps = nullptr;
    SmoothScratch ws{};
    if (k) {
        TRY(tmp.upload(&taps, f));
        for (float **p : {&ws.z0, &ws.mplane, &ws.num, &ws.den, &ws.tmp}) TRY(tmp.alloc(p, n));
    }
    return tmp.finish(smooth_stage(detr, bg_med, reliable, taps, k, ws, hmap, variant ? variant == 2 : Tiers().fused_chains != 0, Tiers().gauss_strip != 0, B,
                                   h, w, tmp.st));
}

int vistaf_ftp_test_core_flip(float *hmap_inout, const float *core_med, int32_t *flipped, int B, int P, void *stream)
{
    if (!hmap_inout || !core_med || !flipped || !frame_ok(B, 1, P)) return refuse("bad argument");
    launch_core_flip(hmap_inout, core_med, flipped, B, P, (hipStream_t)stream);
    return HookTemps(stream).finish();
}

int vistaf_ftp_test_hole_candidates(const float *hmap, const uint8_t *reliable, const float *dist, int ksize, float frac_thr, float min_dist, uint8_t *cand,
                                    int B, int h, int w, void *stream)
{
    if (!hmap || !reliable || !dist || !cand || !frame_ok(B, h, w) || h > 65535 || ksize < 3 || ksize > 511 || !(ksize & 1)) return refuse("bad argument");
    launch_hole_candidates(hmap, reliable, dist, ksize, frac_thr, min_dist, cand, B, h, w, (hipStream_t)stream);
    return HookTemps(stream).finish();
}

int vistaf_ftp_test_hole_tmp(const float *hmap, const uint8_t *reliable, const uint8_t *cand, const float *med, float *tmp, int B, int P, void *stream)
{
    if (!hmap || !reliable || !cand || !med || !tmp || !frame_ok(B, 1, P)) return refuse("bad argument");
    launch_hole_tmp(hmap, reliable, cand, med, tmp, B, P, (hipStream_t)stream);
    return HookTemps(stream).finish();
}
int vistaf_ftp_test_hole_zin(float *tmp_zin, const float *fill, int B, int P, void *stream)
{
    if (!tmp_zin || !fill || !frame_ok(B, 1, P)) return refuse("bad argument");
    launch_hole_zin(tmp_zin, fill, B, P, (hipStream_t)stream);
    return HookTemps(stream).finish();
}
int vistaf_ftp_test_hole_merge(float *hmap_inout, const uint8_t *reliable, const uint8_t *cand, const float *zin, uint8_t *out_rel, int B, int P,
                               void *stream)
{
    if (!hmap_inout || !reliable || !cand || !zin || !out_rel || !frame_ok(B, 1, P)) return refuse("bad argument");
    launch_hole_merge(hmap_inout, reliable, cand, zin, out_rel, B, P, (hipStream_t)stream);
    return HookTemps(stream).finish();
}

int vistaf_ftp_test_height_finish(const float *hmap, const uint8_t *reliable, const uint8_t *roi, const float *dist_in, const float *dist_out,
                                  const float *roi_den, float band, int use_band, double sigma_unrel, int curve_type, double curve_a, double curve_b,
                                  double curve_c, int use_neg, float *unitless, float *depth, uint8_t *cand, float *gmax, int B, int h, int w, int variant,
                                  void *stream)
{
    if (!hmap || !reliable || !roi || !dist_in || !dist_out || !roi_den || !unitless || !depth || !cand || !gmax || !frame_ok(B, h, w) ||
        !sigma_ok(sigma_unrel) || (use_band != 0 && use_band != 1) || (use_band && !(band > 0.f)) || !curve_ok(curve_type, curve_a, curve_b, curve_c))
        return refuse("bad argument");
    if (!variant_012(variant)) return refuse(kVariant012);
    const std::vector<float> f = taps_of(sigma_unrel);
    const int k = (int)f.size();
    if (variant == 2 && !fuses(true, k)) return refuse("variant 2: the tile kernel takes 1..15 taps");
    const size_t n = (size_t)B * h * w;
    HookTemps tmp(stream);
    float *taps = nullptr;
    HeightScratch ws{};
    TRY(tmp.alloc(&ws.z0f, n));
    if (k) { TRY(tmp.upload(&taps, f)); TRY(tmp.alloc(&ws.snum, n)); TRY(tmp.alloc(&ws.tmp, n)); }
    return tmp.finish(height_finish_stage(hmap, reliable, roi, dist_in, use_band ? band : 1.0f, roi_den, dist_out, band, use_band,
                                          Curve{curve_type, curve_a, curve_b, curve_c}, use_neg != 0, taps, k, ws, unitless, depth, cand, (unsigned int *)gmax,
                                          variant ? variant == 2 : Tiers().fused_chains != 0, Tiers().gauss_strip != 0, nullptr, B, h, w, tmp.st));
}

int vistaf_ftp_test_to_mm(const float *unitless, const uint8_t *roi, int curve_type, double curve_a, double curve_b, double curve_c, int use_neg, float *depth,
                          uint8_t *cand, float *gmax, int B, int P, void *stream)
{
    if (!unitless || !roi || !depth || !cand || !gmax || !frame_ok(B, 1, P) || !curve_ok(curve_type, curve_a, curve_b, curve_c)) return refuse("bad argument");
    launch_to_mm(unitless, roi, Curve{curve_type, curve_a, curve_b, curve_c}, use_neg != 0, depth, cand, (unsigned int *)gmax, B, P, (hipStream_t)stream);
    return HookTemps(stream).finish();
}

int vistaf_ftp_test_tail(const float *height, const uint8_t *roi_frame, const float *unitless, const uint8_t *roi_static, double mm_per_px,
                         double depth_eps_mm, double period_px, int force_type, double force_a, double force_b, double force_c, double *scalars, int nscal,
                         double *out3, int B, int P, int variant, void *stream)
{
    if (!height || (!scalars && !out3) || (scalars && (!roi_static || nscal < 9)) || !frame_ok(B, 1, P) || !curve_ok(force_type, force_a, force_b, force_c))
        return refuse("bad argument");
    if (!variant_012(variant)) return refuse(kVariant012);
    HookTemps tmp(stream);
    unsigned long long *scratch = nullptr;      // the chain scratch as a session of frames of P pixels holds it: none below large_frame
    const size_t bytes = variant == 2 || (variant == 0 && large_frame((size_t)P)) ? tail_scratch_bytes(B, P) : 0;
    if (bytes) TRY(tmp.alloc(&scratch, bytes / sizeof(unsigned long long)));
    const int force = variant == 0 ? 0 : variant == 1 ? TAIL_FRAME : TAIL_BLOCKS;
    launch_tail(height, roi_frame, unitless, roi_static, hook_post_params(mm_per_px, depth_eps_mm, period_px, Curve{force_type, force_a, force_b, force_c}),
                scalars, nscal, out3, B, P, tmp.st, scratch, bytes, force);
    return tmp.finish(tail_tier(B, P, scratch != nullptr, bytes, force));
}

int vistaf_ftp_test_backend_fits(int h, int w)
{
    if (!plane_ok(1, h, w)) return refuse("bad argument");
    return backend_fused_fits(h, w) ? 1 : 0;
}

int vistaf_ftp_test_backend(float *depth_inout, const uint8_t *cand, const float *gmax, const float *unitless, const uint8_t *roi_static,
                            const uint8_t *reliable, const int32_t *status, double min_peak_mm, double rel_frac, double mm_per_px, double depth_eps_mm,
                            double period_px, int force_type, double force_a, double force_b, double force_c, int32_t *labels, uint32_t *peak_bits,
                            uint8_t *kept, double *scalars, int nscal, float *out_h, uint8_t *out_r, int B, int h, int w, int variant, void *stream)
{
    if (!depth_inout || !cand || !gmax || !roi_static || !reliable || !status || !labels || !peak_bits || !scalars || nscal < 9 || !frame_ok(B, h, w) ||
        !curve_ok(force_type, force_a, force_b, force_c))
        return refuse("bad argument");
    if (!variant_012(variant)) return refuse(kVariant012);
    if (variant == 2 && !backend_fused_fits(h, w)) return refuse("variant 2: the fused back end does not take this frame size");
    HookTemps tmp(stream);
    unsigned long long *scratch = nullptr;      // of the separate tail, as a session of frames of this size holds it
    const size_t bytes = large_frame((size_t)h * w) ? tail_scratch_bytes(B, h * w) : 0;
    if (bytes) TRY(tmp.alloc(&scratch, bytes / sizeof(unsigned long long)));
    return tmp.finish(backend_stage(depth_inout, cand, (const unsigned int *)gmax, unitless, roi_static, reliable, status, min_peak_mm, rel_frac,
                                    hook_post_params(mm_per_px, depth_eps_mm, period_px, Curve{force_type, force_a, force_b, force_c}), labels, peak_bits, kept,
                                    scalars, nscal, out_h, out_r, scratch, bytes, variant ? variant == 2 : Tiers().fused_backend != 0, nullptr, nullptr, B, h, w,
                                    tmp.st));
}

int vistaf_ftp_test_frame_records(const int *rel_count, const int *flipped, const float *amp_thr, const float *contact_thr, const float *bg_med,
                                  const int *bad_count, double *scalars, int nscal, int32_t *status, int B, void *stream)
{
    if (!rel_count || (!scalars && !status) || (scalars && nscal < 16) || B < 1) return refuse("bad argument");
    if (scalars) launch_fill_scalars(scalars, nscal, rel_count, flipped, amp_thr, contact_thr, bg_med, bad_count, B, (hipStream_t)stream);
    if (status) launch_mark_empty(rel_count, status, B, (hipStream_t)stream);
    return HookTemps(stream).finish();
}

}  // extern "C"
