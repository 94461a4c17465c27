// Per-pixel expressions of the element-wise passes around the short Gaussian blurs and of the binary-mask chains.  Each one is called by its
// own streaming kernel (k_basic.hip, k_cc_dist.hip, k_post.hip) and by the fused kernels (k_blurchain.hip, k_maskchain.hip), so both paths
// execute the same operations in the same order.
// The explicit __f*_rn keep every rounding where the reference has it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "common.hpp"

namespace vf {

// float32: img / (blur + 1e-6) - 1.0
__device__ inline float illum_norm_px(float img, float blur) { return __fsub_rn(__fdiv_rn(img, __fadd_rn(blur, 1e-6f)), 1.0f); }

__device__ inline float mul_static_px(float a, float stat) { return __fmul_rn(a, stat); }

// zeroed = src - scalar; z0 = zeroed on (mask & finite) else 0; m = that mask as float   (shape_ftp.py:1750, :1756, :1142-1144)
__device__ inline void sub_scalar_mask_px(float src, float scalar, uint8_t mask, float &z0, float &m)
{
    float v = __fsub_rn(src, scalar);
    bool ok = mask && finitef(v);
    z0 = ok ? v : 0.f;
    m = ok ? 1.f : 0.f;
}

// num / (den + 1e-6)   (shape_ftp.py:1146-1147)
__device__ inline float div_planes_px(float num, float den) { return __fdiv_rn(num, __fadd_rn(den, 1e-6f)); }

// frontier taper inside reliable (shape_ftp.py:1287-1318): the smoothstep weight of the distance to the outside; 0 off the reliable ROI
// pixels, where hgt and dist_in do not matter (computed and discarded: no branch, so a caller's loads of them need not wait for the mask)
__device__ inline float frontier_compose_px(bool rel_roi, float hgt, float dist_in, float band)
{
    // hgt finite where it counts: `reliable` is output_reliable = reliable & isfinite(height) (:1801)
    float de = fmaxf(__fsub_rn(dist_in, 1.0f), 0.0f);
    float t = __fdiv_rn(de, fmaxf(1e-6f, band));
    t = fminf(fmaxf(t, 0.0f), 1.0f);
    float wgt = __fmul_rn(__fmul_rn(t, t), __fsub_rn(3.0f, __fmul_rn(2.0f, t)));
    float v = __fmul_rn(hgt, wgt);
    return rel_roi ? v : 0.f;
}

// unreliable ROI <- masked blur, outside band <- 0, clamp positives, NaN outside ROI (shape_ftp.py:1820-1841).  smooth_num / roi_den are
// only looked at on unreliable ROI pixels with have_smooth, dist_out only on those with use_band.
__device__ inline float finalize_unitless_px(bool roi, bool rel, float z0, bool have_smooth, float smooth_num, float roi_den, bool use_band,
                                             float dist_out, float band)
{
    float v = nanf32();
    if (roi) {
        v = z0;
        if (!rel) {
            if (have_smooth) v = __fdiv_rn(smooth_num, roi_den);
            if (use_band) {
                float de = fmaxf(__fsub_rn(dist_out, 1.0f), 0.0f);
                if (de <= band) v = 0.f;
            }
        }
        // np.minimum(v, 0.0) hands back its second operand when the two are equal: a zero of either sign becomes +0.0 (the taper leaves -0.0
        // at the mask's edge, a negative height times weight 0)
        if (finitef(v)) v = __fadd_rn(fminf(v, 0.0f), 0.0f);
    }
    return v;
}

// unitless -> mm (shape_ftp.py:682-705) and the blob candidate flag (:1232-1236); returns the candidate flag
__device__ inline bool to_mm_px(float hgt, bool roi, const Curve &curve, int use_neg, float &depth)
{
    float d = hgt;   // NaN stays NaN
    if (hgt == hgt) {
        double x = use_neg ? -(double)hgt : (double)hgt;
        x = fmax(x, 0.0);
        d = (float)curve_eval(curve, x);
    }
    depth = d;
    return roi && finitef(d) && d > 0.0f;
}

// ---- the binary-mask chains (k_maskchain.hip and the streaming kernels it replaces) ------------------------------------------------------
// bad pixel (shape_ftp.py:638-639)
__device__ inline bool bad_flag_px(uint8_t valid, float img, float grad, float thr_hi, float thr_g) { return valid && ((img >= thr_hi) || (grad >= thr_g)); }

// quality threshold (shape_ftp.py:753); a NaN threshold leaves no pixel
__device__ inline bool quality_mask_px(uint8_t roi, float q, float thr) { return roi && finitef(q) && q >= thr; }

// contact pixel (shape_ftp.py:1719-1732)
__device__ inline bool contact_px(uint8_t reliable, float res, float thr)
{
    const float v = fabsf(res);
    return reliable && finitef(v) && v >= thr;
}
// the threshold the contact count is taken with: the first percentile, the second when the first is not finite.  t3: the frame's three.
__device__ inline float contact_first_thr(const float *__restrict__ t3)
{
    float thr = t3[0];
    if (!finitef(thr)) thr = t3[1];
    return thr;
}
// the threshold the mask is formed with: float64 fraction against the float64 constants, as upstream's NumPy compares them (a bound narrowed
// to float32 moves the boundary)
__device__ inline float contact_used_thr(const float *__restrict__ t3, int contact_count, int rel_count, double min_frac, double max_frac)
{
    float thr = contact_first_thr(t3);
    const double frac = (double)contact_count / (double)(rel_count > 1 ? rel_count : 1);
    if (frac < min_frac) { const float t2 = t3[1]; if (finitef(t2)) thr = t2; }
    else if (frac > max_frac) { const float t2 = t3[2]; if (finitef(t2)) thr = t2; }
    return thr;
}
// background = reliable & ~contact_d falls back to reliable below 15 % of it (shape_ftp.py:1738-1741)
__device__ inline bool background_falls_back(int bg_count, int rel_count) { return bg_count < (int)(0.15 * (double)rel_count); }
// frames whose reliable mask is empty produce the upstream "return None" status, unless they carry a status already
__device__ inline bool marks_empty(int rel_count, int32_t status) { return rel_count == 0 && status == 0; }

}  // namespace vf
