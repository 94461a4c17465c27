// Device code that k_backend.hip shares with the kernels it replaces (k_cc_label_lds in k_cc_dist.hip, k_blob_apply and k_tail in k_post.hip):
// one definition, so the fused back end and the separate kernels execute the same operations in the same order.  Included by those three
// files only; the mask family's rules it builds on are in mask_rules.hpp.
#pragma once
#include "kernels.hpp"
#include "mask_rules.hpp"
#include "pixel_ops.hpp"

namespace vf {

// LDS-resident label forest for frames of at most 65535 pixels: one uint16 per pixel, so finds and unions are LDS round trips instead of
// L2 round trips.  LDS has no 16-bit atomics: the "hang root b under a" step is a 32-bit CAS on the word holding the label.
__device__ inline uint32_t cc16_min(uint16_t *L, int i, uint32_t val)
{
    uint32_t *wp = (uint32_t *)L + (i >> 1);
    const int sh = (i & 1) * 16;
    uint32_t old = *(volatile uint32_t *)wp;
    for (;;) {
        uint32_t cur = (old >> sh) & 0xffffu;
        if (cur <= val) return cur;
        uint32_t nw = (old & ~(0xffffu << sh)) | (val << sh);
        uint32_t prev = atomicCAS(wp, old, nw);
        if (prev == old) return cur;
        old = prev;
    }
}
__device__ inline int cc16_find(uint16_t *L, int i)
{
    volatile uint16_t *V = L;
    for (;;) {
        int p = V[i];
        if (p == i) return i;
        int g = V[p];
        if (g == p) return p;
        V[i] = (uint16_t)g;      // path halving (benign race: g is an ancestor of i)
        i = g;
    }
}
__device__ inline void cc16_unite(uint16_t *L, int a, int b)
{
    for (;;) {
        a = cc16_find(L, a);
        b = cc16_find(L, b);
        if (a == b) return;
        if (a > b) { int t = a; a = b; b = t; }
        uint32_t old = cc16_min(L, b, (uint32_t)a);
        if ((int)old == b) return;
        b = (int)old;
    }
}
// Builds the forest of one frame's mask m in L16 (all threads of a 1024-thread workgroup call it): on return every union is done and
// visible (the last statement is a barrier), cc16_find(L16, p) is the root -- the smallest pixel index -- of mask pixel p's 8-connected
// component, and non-mask pixels hold 0xffff.  m is indexed by pixel: a byte plane (in LDS or in memory), or the BitMask of a bit plane
// in LDS.  m must be visible to the workgroup on entry.
template <typename Mask>
__device__ inline void cc_lds_forest(Mask m, int h, int w, uint16_t *L16)
{
    const int P = h * w;
    // Every pixel starts at the left end of its horizontal run (row_last_zero: 16 waves, one row at a time each), so a run is one tree
    // from the start and only the contacts between runs of adjacent rows are left to unite -- a few hundred unions per frame instead of
    // four per pixel.  Roots are minimum pixel indices either way: same labels.
    {
        const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nwv = blockDim.x >> 6;
        for (int y = wid; y < h; y += nwv) {
            int carry = -1;                                     // position of the last zero pixel seen in the row
            for (int x0 = 0; x0 < w; x0 += 64) {
                const int x = x0 + lane;
                const bool on = x < w && m[y * w + x];
                const int lz = row_last_zero(x < w && !on, x, carry);
                if (x < w) L16[y * w + x] = on ? (uint16_t)(y * w + lz + 1) : (uint16_t)0xffffu;
            }
        }
    }
    if ((P & 1) && threadIdx.x == 0) L16[P] = 0xffffu;
    __syncthreads();
    for (int p = threadIdx.x; p < P; p += blockDim.x) {
        if (!m[p]) continue;
        const int y = p / w, x = p - y * w;
        cc_row_contacts(m, p, x, y, w, x > 0 && m[p - 1], [L16](int a, int b) { cc16_unite(L16, a, b); });
    }
    __syncthreads();
}
// The forest of the byte plane mg.  Returns the mask to test pixels with: for MLDS the LDS copy staged behind the forest (every neighbour
// test is an LDS read), else mg.
template <bool MLDS>
__device__ inline const uint8_t *cc_lds_build(const uint8_t *__restrict__ mg, int h, int w, uint16_t *L16)
{
    const int P = h * w;
    uint8_t *ml = (uint8_t *)(L16 + ((P + 2 + 7) & ~7));
    if (MLDS) {
        for (int p = threadIdx.x * 4; p < P; p += blockDim.x * 4) {
            if (p + 3 < P && ((((uintptr_t)mg) & 3) == 0)) *(uint32_t *)(ml + p) = *(const uint32_t *)(mg + p);
            else for (int k = 0; k < 4 && p + k < P; k++) ml[p + k] = mg[p + k];
        }
        __syncthreads();
    }
    const uint8_t *m = MLDS ? (const uint8_t *)ml : mg;
    cc_lds_forest(m, h, w, L16);
    return m;
}
// Pixel p of the mask points at its root for good: a walk that writes nothing on its way, so when every thread of the workgroup does this
// for its pixels between two barriers the only stores are roots -- no path-halving store of another thread's find can land on L16[p]
// afterwards and leave an inner node there (a walk through p meanwhile reads its old parent or the root).  Returns the root.  This is the
// walk of k_backend_fused's first step, which keeps its own three lines: routed through this function the compiler rotated that kernel's
// loop differently and the kernel measured 210.2 us against 205.0 us (profiles/README.md, the mask chains).
__device__ inline int cc16_settle(uint16_t *L16, int p)
{
    int r = p;
    for (int q = ((volatile uint16_t *)L16)[r]; q != r; q = ((volatile uint16_t *)L16)[r]) r = q;
    L16[p] = (uint16_t)r;
    return r;
}

// blob filter (shape_ftp.py:1247-1250): the threshold is formed in float64 (Python floats); `peaks >= thr` then compares a float32 array with
// a Python float, which NumPy 2 rounds to float32 first: the comparison is float32 against float32(thr)
__device__ inline float blob_keep_threshold(unsigned int gmax_bits, double min_peak_mm, double rel_frac)
{
    double gmax = (double)__uint_as_float(gmax_bits);
    double thr = min_peak_mm;
    if (rel_frac >= 0.0) thr = fmax(thr, rel_frac * gmax);
    return (float)thr;
}

// Force tail + arg-extrema of frame b, all 1024 threads of its workgroup (k_tail's body; see k_post.hip for what it computes).
// height(p) yields the height of pixel p in mm; it is called exactly once for every p < P, by thread p % blockDim.x, in ascending p.
// R (the frame's own roi, or null: isfinite(height)), U (the frame's unitless plane, or null) are the frame's planes; roi_static is shared.
constexpr int TAIL_STATIC_LDS = 16 * 8 * 2;     // the reduction scratch below
template <typename HeightFn>
__device__ inline void tail_frame(HeightFn height, const uint8_t *__restrict__ R, const float *__restrict__ U, const uint8_t *__restrict__ roi_static,
                                  const PostParams &pp, double *__restrict__ scalars, int nscal, double *__restrict__ out3, int b, int P)
{
    __shared__ double sd[16];
    __shared__ unsigned long long s64[16];
    // ONE pass over the planes, four pixels per thread in flight: the dominant sign (nansum(neg) > nansum(pos); float32 sums upstream,
    // double here) is only known at the end, so the volume / area / maximum are accumulated for both signs and the right set is kept.
    // Per thread the pixels come in the same order as in separate passes: the sums are the same bits.
    const bool want_arg = scalars != nullptr;
    const float eps = (float)pp.depth_eps_mm;
    double sp = 0, sn = 0, volp = 0, voln = 0;
    int cntp = 0, cntn = 0;
    unsigned long long mxp = 0, mxn = 0, am = 0, an = ~0ull;
    constexpr int TU = 4;
    const int T = blockDim.x;
    for (int p0 = threadIdx.x; p0 < P; p0 += TU * T) {
        float v[TU], u[TU];
        uint8_t rf[TU], rs[TU];
#pragma unroll
        for (int k = 0; k < TU; k++) {
            const int p = p0 + k * T;
            const bool inb = p < P;
            v[k] = inb ? height(p) : nanf32();
            rf[k] = (inb && R) ? R[p] : (uint8_t)0;
            rs[k] = (inb && want_arg) ? roi_static[p] : (uint8_t)0;
            u[k] = (inb && U) ? U[p] : nanf32();
        }
#pragma unroll
        for (int k = 0; k < TU; k++) {
            const int p = p0 + k * T;
            if (p >= P) break;
            const float vv = v[k];
            if (vv == vv) { if (vv > 0.f) sp += vv; else sn += -vv; }
            const bool in = R ? rf[k] != 0 : finitef(vv);
            float dp = fmaxf(vv, 0.f), dn = fmaxf(-vv, 0.f);
            if (!in || !finitef(dp)) dp = 0.f;
            if (!in || !finitef(dn)) dn = 0.f;
            if (dp > eps) { volp += dp; cntp++; const unsigned long long key = (unsigned long long)__float_as_uint(dp) << 32; if (key > mxp) mxp = key; }
            if (dn > eps) { voln += dn; cntn++; const unsigned long long key = (unsigned long long)__float_as_uint(dn) << 32; if (key > mxn) mxn = key; }
            if (rs[k] && finitef(vv)) {            // arg-max of depth (mm) over roi & finite: first occurrence of the maximum
                const unsigned long long key = argmax_key(vv, (unsigned int)p);
                if (key > am) am = key;
            }
            if (rs[k] && finitef(u[k])) {          // arg-min of unitless height over roi & finite: first occurrence of the minimum
                const unsigned long long key = argmin_key(u[k], (unsigned int)p);
                if (key < an) an = key;
            }
        }
    }
    sp = block_sum<double>(sp, sd);
    sn = block_sum<double>(sn, sd);
    const bool use_neg = (float)sn > (float)sp;
    double vol = block_sum<double>(use_neg ? voln : volp, sd);
    double cntd = block_sum<double>((double)(use_neg ? cntn : cntp), sd);
    unsigned long long mx = block_max_u64(use_neg ? mxn : mxp, s64);
    double period_px = pp.period_px, mm_per_px = pp.mm_per_px;
    if (pp.pair_geom) { period_px = pp.pair_geom[b].period; mm_per_px = period_px > 1e-12 ? pp.grating_pitch_mm / period_px : 0.0; }
    double area_px = mm_per_px * mm_per_px;
    double volume_cm3 = cntd > 0 ? (double)(float)vol * area_px / 1000.0 : 0.0;
    double area_mm2 = cntd * area_px;
    double maxd = cntd > 0 ? (double)__uint_as_float((unsigned int)(mx >> 32)) : 0.0;
    if (out3 && threadIdx.x == 0) { out3[b * 3] = volume_cm3; out3[b * 3 + 1] = area_mm2; out3[b * 3 + 2] = maxd; }
    if (!scalars) return;
    am = block_max_u64(am, s64);
    if (U) an = block_min_u64(an, s64);
    if (threadIdx.x == 0) {
        double *S = scalars + b * (size_t)nscal;
        S[0] = volume_cm3; S[1] = area_mm2; S[2] = maxd;
        S[3] = curve_eval(pp.force_curve, volume_cm3);
        S[4] = am ? (double)(0xffffffffu - (unsigned int)(am & 0xffffffffu)) : -1.0;
        S[5] = period_px; S[6] = mm_per_px;
        if (U && an != ~0ull) { S[7] = (double)key2f((unsigned int)(an >> 32)); S[8] = (double)(unsigned int)(an & 0xffffffffu); }
        else { S[7] = (double)nanf32(); S[8] = -1.0; }
    }
}

}  // namespace vf
