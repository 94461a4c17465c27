// The rules of the Telea inpaint family (k_inpaint*.hip), each stated once: the flag byte and its two state sets, the magic row division, the
// window of a hole box, the window build's taps and its hole / band / ring classification, the FMM quadrant solve and the quad minimum, the
// outside pass's per-pop body, the estimator's arithmetic, the ordered sums, and the two-run stable priority queue of the single-wave marches.
// Private to the family.  Pure arithmetic is __host__ __device__ so that tests/diag/telea_host_check.hip can hold it against brute force.
#pragma once
#include <type_traits>
#include "common.hpp"
#include "kernels.hpp"

namespace vf {

// ---- the family's inner launcher (the public ones and the capacities are in kernels.hpp) --------------------------------------------------------
// k_inpaint_win.hip: every cluster of the list on its own LDS window, one wave each; big[root] = 1 for those whose queue overflowed
void launch_telea_clusters2(float *img, const uint8_t *bad, const int32_t *labels, const int32_t *list, const int32_t *count, const int32_t *xmin,
                            const int32_t *ymin, const int32_t *xmax, const int32_t *ymax, uint8_t *big, int range, int B, int h, int w, hipStream_t st);

// flag byte: bits 0-1 state, bit 4 outside the image, bit 5 scratch (hole in row range), bit 6 hole pixel,
// bit 7 seed (initial band)
constexpr uint8_t W_KNOWN = 0, W_BAND = 1, W_INSIDE = 2, W_CHANGE = 3, W_ST = 3, W_BORDER = 0x10, W_ROW = 0x20, W_HOLE = 0x40, W_SEED = 0x80;

// cell / ww == umulhi(cell, magic) for every cell with cell * ww < 2^32
__host__ __device__ inline uint32_t telea_magic_ww(int ww) { return (uint32_t)(0x100000000ull / (unsigned)ww) + 1u; }
// the multiplier of a plane of `rows` rows of ww cells, 0 where the split is not exact for every cell of it (the convention of unwrap.hpp)
__host__ __device__ inline uint32_t telea_magic_plane(int ww, int rows)
{
    return (unsigned long long)ww * (unsigned long long)ww * (unsigned long long)rows < 0x100000000ull ? telea_magic_ww(ww) : 0u;
}

// The window of a box of hole pixels (frame coordinates, inclusive): the box grown by range + 1, NOT clipped to the frame.  Cell (r, cc) is
// pixel (i0 + r - 1, j0 + cc - 1): i0 / j0 are coordinates of the frame padded by one cell, cells beyond the image carry W_BORDER.
struct TeleaBoxWin {
    int i0, j0, wh, ww;
    __host__ __device__ int cells() const { return wh * ww; }
    // cell (r, cc) of a window of `ncell` cells (li = its index): inside the image?  gp = its pixel index there, else 0
    __host__ __device__ __attribute__((always_inline)) bool locate(int li, int ncell, int r, int cc, int h, int w, size_t &gp) const
    {
        const int gi = i0 + r, gj = j0 + cc;
        const bool in = li < ncell && gi >= 1 && gi <= h && gj >= 1 && gj <= w;
        gp = in ? (size_t)(gi - 1) * w + (gj - 1) : 0;
        return in;
    }
    __host__ __device__ __attribute__((always_inline)) size_t pixel(int r, int cc, int w) const { return (size_t)(i0 + r - 1) * w + (j0 + cc - 1); }
};
__host__ __device__ inline TeleaBoxWin telea_window_of_box(int xmin, int ymin, int xmax, int ymax, int range)
{
    const int M = range + 1;
    const int i0 = ymin + 1 - M, i1 = ymax + 1 + M, j0 = xmin + 1 - M, j1 = xmax + 1 + M;      // [i0, i1] x [j0, j1] in padded frame coordinates
    return {i0, j0, i1 - i0 + 1, j1 - j0 + 1};
}

// ---- window build: ring = within Chebyshev `range` of the hole, separable (rows into W_ROW, then columns); band = 4-neighbours of the hole.
// Per-cell pieces; the kernels keep their own loops.  Every tap of a cell is an independent load (clamped index + select: a loop over
// [-range, range] or a short-circuit test would be one dependent LDS round trip per tap); ranges above TELEA_RING_U loop.
constexpr int TELEA_RING_U = 6;
// OR of the flag bytes within `range` columns of cell li = (r, cc) in its row
__host__ __device__ __attribute__((always_inline)) inline uint8_t telea_ring_row_tap(const uint8_t *f, int li, int r, int cc, int ww, int range)
{
    uint8_t a = 0;
    if (range <= TELEA_RING_U) {
#pragma unroll
        for (int d = -TELEA_RING_U; d <= TELEA_RING_U; d++) {
            const int c2 = cc + d;
            const bool in = d >= -range && d <= range && c2 >= 0 && c2 < ww;
            const uint8_t v = f[in ? li + d : li];
            a |= in ? v : (uint8_t)0;
        }
    } else {
        const int lo = cc - range > 0 ? cc - range : 0, hi = cc + range < ww - 1 ? cc + range : ww - 1;
        for (int c2 = lo; c2 <= hi; c2++) a |= f[r * ww + c2];
    }
    return a;
}
// OR of the flag bytes within `range` rows of cell li = (r, cc) in its column
__host__ __device__ __attribute__((always_inline)) inline uint8_t telea_ring_col_tap(const uint8_t *f, int li, int r, int cc, int wh, int ww, int range)
{
    uint8_t a = 0;
    if (range <= TELEA_RING_U) {
#pragma unroll
        for (int d = -TELEA_RING_U; d <= TELEA_RING_U; d++) {
            const int r2 = r + d;
            const bool in = d >= -range && d <= range && r2 >= 0 && r2 < wh;
            const uint8_t v = f[in ? li + d * ww : li];
            a |= in ? v : (uint8_t)0;
        }
    } else {
        const int lo = r - range > 0 ? r - range : 0, hi = r + range < wh - 1 ? r + range : wh - 1;
        for (int r2 = lo; r2 <= hi; r2++) a |= f[r2 * ww + cc];
    }
    return a;
}
// OR of the flag bytes of the four 4-neighbours.  Window edge cells are at distance range + 1 from the hole: never band, their neighbours are
// not needed (a clamped index reads the cell itself, which only matters when it is not a hole pixel)
__host__ __device__ __attribute__((always_inline)) inline uint8_t telea_nb4_tap(const uint8_t *f, int li, int r, int cc, int wh, int ww)
{
    return f[cc > 0 ? li - 1 : li] | f[cc < ww - 1 ? li + 1 : li] | f[r > 0 ? li - ww : li] | f[r < wh - 1 ? li + ww : li];
}
// what the outside pass makes of a cell: nothing (a hole pixel -- KNOWN for that pass --, a cell beyond the image, or out of reach), a band
// pixel (seed of both passes, T = 0) or a ring cell (INSIDE for the outside pass)
enum TeleaCellKind { TC_NONE = 0, TC_BAND = 1, TC_RING = 2 };
// me = the cell's flag byte, nb4 = telea_nb4_tap, col = telea_ring_col_tap over bytes that carry W_ROW
__host__ __device__ __attribute__((always_inline)) inline int telea_cell_kind(uint8_t me, uint8_t nb4, uint8_t col)
{
    if (me & (W_BORDER | W_HOLE)) return TC_NONE;
    if (nb4 & W_HOLE) return TC_BAND;
    return (col & W_ROW) ? TC_RING : TC_NONE;
}
// the same classification of a known pixel (y, x) inside the image straight from a hole predicate (the prep kernels: one thread per cell)
template <class Hole>
__host__ __device__ __attribute__((always_inline)) inline int telea_known_pixel_kind(Hole hole, int y, int x, int range)
{
    if (hole(y, x - 1) || hole(y, x + 1) || hole(y - 1, x) || hole(y + 1, x)) return TC_BAND;
    for (int a = -range; a <= range; a++)
        for (int c = -range; c <= range; c++)
            if (hole(y + a, x + c)) return TC_RING;
    return TC_NONE;
}
// After the outside pass: the flag byte with the march's state (hole = INSIDE, rest KNOWN); neg = the outside pass ran here (CHANGE), T is negated
__host__ __device__ __attribute__((always_inline)) inline uint8_t telea_to_march_state(uint8_t v, bool &neg)
{
    neg = (v & W_ST) == W_CHANGE;
    return (uint8_t)((v & (W_SEED | W_HOLE | W_BORDER)) | ((v & W_HOLE) ? W_INSIDE : W_KNOWN));
}

__device__ inline float wn_lane_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// Sum over lanes [0, N) in LANE ORDER from `init`: ((init + x0) + x1) + ... + x(N-1), every addition rounded to float.  That is the order
// in which cv::inpaint's k / l loops accumulate Ia, Jx, Jy and s (inpaint.cpp icvTeleaInpaintFMM), so the
// filled pixels carry the same roundings bit for bit -- they feed the illumination blur, the demodulation and, through the amplitude, the
// quality >= p25 threshold of the reliable mask.  After step t lanes 0..t hold their final prefix (lane l takes lane l-1's value through
// wave_shr:1 and adds its own term; a lane that is already final recomputes the same value), so N-1 dependent DPP adds give the total.
// A tree reduction is ~6 steps instead of N-1 but rounds differently (up to 1e-6 relative on a filled pixel).
template <int N>
__device__ __attribute__((always_inline)) inline float wn_seq_sum(float x, float init, int lane)
{
    const float xi = lane == 0 ? __fadd_rn(init, x) : x;
    float S = xi;
#pragma unroll
    for (int t = 1; t < N; t++)
        S = __fadd_rn(__int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(S), 0x138, 0xf, 0xf, true)), xi);     // lane 0: 0 + xi
    return wn_lane_f(S, N - 1);
}
// the four estimator sums side by side: four independent chains, so a step issues back to back instead of waiting out the DPP hazard
template <int N>
__device__ __attribute__((always_inline)) inline void wn_seq_sum4(float &a, float &b, float &c, float &d, float init_d, int lane)
{
    const float xd = lane == 0 ? __fadd_rn(init_d, d) : d;      // a, b, c start at +0: 0 + x = x
    float Sa = a, Sb = b, Sc = c, Sd = xd;
#pragma unroll
    for (int t = 1; t < N; t++) {
        const float pa = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(Sa), 0x138, 0xf, 0xf, true));
        const float pb = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(Sb), 0x138, 0xf, 0xf, true));
        const float pc = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(Sc), 0x138, 0xf, 0xf, true));
        const float pd = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(Sd), 0x138, 0xf, 0xf, true));
        Sa = __fadd_rn(pa, a); Sb = __fadd_rn(pb, b); Sc = __fadd_rn(pc, c); Sd = __fadd_rn(pd, xd);
    }
    a = wn_lane_f(Sa, N - 1); b = wn_lane_f(Sb, N - 1); c = wn_lane_f(Sc, N - 1); d = wn_lane_f(Sd, N - 1);
}
// runtime length (n uniform, 1 <= n <= 64): the general estimator path and the whole-frame kernel
__device__ inline float wn_seq_sum_n(float x, float init, int n, int lane)
{
    const float xi = lane == 0 ? __fadd_rn(init, x) : x;
    float S = xi;
    for (int t = 1; t < n; t++)
        S = __fadd_rn(__int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(S), 0x138, 0xf, 0xf, true)), xi);
    return wn_lane_f(S, n - 1);
}
// Ia / s + (Jx + Jy) / (sqrt(Jx^2 + Jy^2) + 1e-20): the float quotient and sums promoted to double for the second term and the final
// addition (inpaint.cpp's expression with its double-precision sqrt)
__device__ inline double telea_estimate_d(float Ia, float Jx, float Jy, float s)
{
    return (double)__fdiv_rn(Ia, s) + (double)__fadd_rn(Jx, Jy) / (sqrt((double)__fadd_rn(__fmul_rn(Jx, Jx), __fmul_rn(Jy, Jy))) + (double)1.0e-20f);
}
__device__ inline float telea_estimate(float Ia, float Jx, float Jy, float s) { return (float)telea_estimate_d(Ia, Jx, Jy, s); }
// the uchar branch of icvTeleaInpaintFMM (8-bit images, here as floats holding 0..255): + 0.5f, cvRound, saturate_cast<uchar>
__device__ inline float telea_estimate_u8(float Ia, float Jx, float Jy, float s)
{
    const float sat = (float)(telea_estimate_d(Ia, Jx, Jy, s) + (double)0.5f);
    return fminf(fmaxf(rintf(sat), 0.f), 255.f);
}
// 1 / (1 + |T - Tc|) formed in double and rounded to float (inpaint.cpp: lev = (float)(1./(1+fabs(...))))
__device__ inline float telea_lev(float tk, float tc) { return (float)(1.0 / (1.0 + (double)fabsf(__fsub_rn(tk, tc)))); }
// 1 / |r|^3 of the offset r = (rx, ry) from a window position to the pixel (dst = 1 / (|r|^2 * |r|), the product in float, the quotient in
// double); 0 at the centre, which never contributes
__device__ inline float telea_dstw(float rx, float ry)
{
    const float len2 = __fadd_rn(__fmul_rn(rx, rx), __fmul_rn(ry, ry));
    return len2 > 0.f ? (float)(1. / (double)__fmul_rn(len2, sqrtf(len2))) : 0.f;
}
// r . grad T, replaced by 1e-6 where |.| <= 0.01 (float(0.01) < 0.01: the same set of floats as OpenCV's double compare)
__device__ inline float telea_dir(float rx, float ry, float gtx, float gty)
{
    const float dir = __fadd_rn(__fmul_rn(rx, gtx), __fmul_rn(ry, gty));
    return fabsf(dir) <= 0.01f ? 0.000001f : dir;
}
__device__ inline float telea_weight(float dstw, float lev, float dir) { return fabsf(__fmul_rn(__fmul_rn(dstw, lev), dir)); }
// OpenCV's gradient along one axis from the states of the two neighbours: kp / km = the neighbour at +1 / -1 is not INSIDE; both usable:
// the central difference, one: the one-sided difference, none: 0.  All three differences come evaluated and are SELECTED (two levels):
// nested conditional expressions would come back as branches, and a taken branch costs a lone wave tens of cycles.
__device__ __attribute__((always_inline)) inline float telea_grad_select(bool kp, bool km, float both, float fwd, float bwd)
{
    const float g_p = km ? both : fwd, g_n = km ? bwd : 0.f;
    return kp ? g_p : g_n;
}
// grad T at the pixel being filled (tc: its own T just solved; tp / tm: its neighbours at +1 / -1)
__device__ __attribute__((always_inline)) inline float telea_grad_T(bool kp, bool km, float tp, float tm, float tc)
{
    return telea_grad_select(kp, km, __fmul_rn(__fsub_rn(tp, tm), 0.5f), __fsub_rn(tp, tc), __fsub_rn(tc, tm));
}
// gradient of the image at a window position along one axis: vP / vM = the values at +1 / -1, vC = the position's own, vS = the value the
// backward difference starts from (vC unless OpenCV's index shift at the image border moves it); kp / km as above
__device__ __attribute__((always_inline)) inline float telea_grad_I(bool kp, bool km, float vP, float vM, float vC, float vS)
{
    return telea_grad_select(kp, km, __fmul_rn(__fsub_rn(vP, vM), 2.0f), __fsub_rn(vP, vC), __fsub_rn(vS, vM));
}
// terms of Ia += w * I, Jx -= w * (gix * rx), Jy -= w * (giy * ry), s += w of one window position; a position that is not used adds 0
struct TeleaTerms { float Ia, Jx, Jy, s; };
__device__ __attribute__((always_inline)) inline TeleaTerms telea_terms(bool use, float wgt, float vC, float gix, float giy, float rx, float ry)
{
    const float z = 0.f;
    TeleaTerms a;
    a.Ia = use ? __fmul_rn(wgt, vC) : z;
    a.Jx = use ? -__fmul_rn(wgt, __fmul_rn(gix, rx)) : z;
    a.Jy = use ? -__fmul_rn(wgt, __fmul_rn(giy, ry)) : z;
    a.s = use ? wgt : z;
    return a;
}

// Stable priority queue (T, push order), the semantics of OpenCV's CvPriorityQueueFloat.  Two sorted runs:
//   * COLD: a sorted array of (T bits << 32 | cell) words in LDS, popped at its head;
//   * HOT: the newest <= 64 pushes, sorted, one per lane in registers.  A push is a branch-free insertion
//     (one DPP shift of the lanes holding larger keys); nothing in LDS moves.
// Every hot entry is younger than every cold entry, so "cold first on equal T" is FIFO.  When the hot run is full
// it is merged into the cold array: each hot lane binary-searches its slot (after the cold entries with
// T' <= T), each cold entry above the smallest hot key binary-searches how many hot keys precede it, and every
// word moves once.  A FMM push lands ~100 entries below the tail of a single sorted array; with the buffer the
// amortised cost of a push is a handful of VALU ops plus ~1/64 of a merge.
struct WQ {
    unsigned long long *e;      // cold run, LDS [cap]
    uint32_t *hotL;             // LDS [64]: hot keys during a merge
    int head, tail, ovf;        // uniform
    int cap;                    // capacity of e (power of two)
    int nh;                     // uniform: hot entries (lanes [0, nh), ascending)
    uint32_t h0;                // uniform: smallest hot key, 0xFFFFFFFF if none
    uint32_t hk, hv;            // per lane: hot key (0xFFFFFFFF = empty) / cell
    uint32_t preT, preI;        // per lane copy of the cold head entry (valid while head < tail)
};
__device__ __attribute__((always_inline)) inline void wq_init(WQ &q)
{
    q.head = q.tail = 0; q.nh = 0; q.h0 = 0xFFFFFFFFu; q.hk = 0xFFFFFFFFu; q.hv = 0; q.preT = 0xFFFFFFFFu; q.preI = 0;
}
__device__ __attribute__((always_inline)) inline void wq_prefetch(WQ &q)
{
    // unconditional (a stale word is read when the run is empty; wq_pop checks head < tail before using it)
    unsigned long long v = q.e[q.head & (q.cap - 1)];
    q.preT = (uint32_t)(v >> 32); q.preI = (uint32_t)v;
}
// PRE: keep a prefetched copy of the cold head for wq_pop (false: the caller reads the run itself)
template <bool PRE = true>
__device__ __attribute__((always_inline)) inline void wq_merge(WQ &q, int lane)
{
    int n = q.tail - q.head;
    if (q.tail + 64 > q.cap) {
        if (q.head == 0) { q.ovf = 1; q.nh = 0; q.hk = 0xFFFFFFFFu; q.h0 = 0xFFFFFFFFu; return; }
        for (int j0 = 0; j0 < n; j0 += 64) {                // slide the cold run back to 0 (ascending chunks never clobber unread words)
            int j = j0 + lane;
            unsigned long long v = 0;
            if (j < n) v = q.e[j + q.head];
            __builtin_amdgcn_wave_barrier();
            if (j < n) q.e[j] = v;
            __builtin_amdgcn_wave_barrier();
        }
        q.head = 0; q.tail = n;
    }
    const unsigned long long *ce = q.e + q.head;
    q.hotL[lane] = q.hk;
    // slot of hot lane i: after the c cold entries with T' <= key
    int lo = 0, hi = n;
    const int it1 = n > 0 ? 32 - __builtin_clz((unsigned)n) : 0;     // ceil(log2(n + 1))
    for (int it = 0; it < it1; it++) {
        int mid = (lo + hi) >> 1;
        bool act = lo < hi;
        uint32_t tm = act ? (uint32_t)(ce[mid] >> 32) : 0u;
        if (act) { if (tm <= q.hk) lo = mid + 1; else hi = mid; }
    }
    const int c = lo;
    const int c0 = __builtin_amdgcn_readfirstlane(c);        // cold entries below c0 stay where they are
    __builtin_amdgcn_wave_barrier();
    for (int jt = n - 1; jt >= c0; jt -= 64) {               // top-down: an entry moves up by <= 64
        const int j = jt - lane;
        const bool act = j >= c0;
        const unsigned long long v = act ? ce[j] : 0ull;
        const uint32_t tj = (uint32_t)(v >> 32);
        int l2 = 0, h2 = 64;                                  // s = hot keys < tj
#pragma unroll
        for (int it = 0; it < 7; it++) {
            int mid = (l2 + h2) >> 1;
            bool a2 = l2 < h2;
            uint32_t km = q.hotL[a2 ? mid : 0];
            if (a2) { if (km < tj) l2 = mid + 1; else h2 = mid; }
        }
        __builtin_amdgcn_wave_barrier();
        if (act) q.e[q.head + j + l2] = v;
        __builtin_amdgcn_wave_barrier();
    }
    if (lane < q.nh) q.e[q.head + c + lane] = ((unsigned long long)q.hk << 32) | q.hv;      // lanes >= nh are empty (key 0xFFFFFFFF sorts last)
    __builtin_amdgcn_wave_barrier();
    q.tail += q.nh;
    q.nh = 0; q.hk = 0xFFFFFFFFu; q.h0 = 0xFFFFFFFFu;
    if (PRE) wq_prefetch(q);
}
template <bool PRE = true>
__device__ __attribute__((always_inline)) inline void wq_push(WQ &q, float Tf, int idx, int lane)
{
    if (q.nh == 64) { wq_merge<PRE>(q, lane); if (q.ovf) return; }
    const uint32_t tb = __float_as_uint(Tf);
    const uint32_t pk = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)q.hk, 0x138, 0xf, 0xf, false);    // wave_shr1: lane l <- l-1, lane 0 <- 0
    const uint32_t pv = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)q.hv, 0x138, 0xf, 0xf, false);
    const bool gt = q.hk > tb, pgt = pk > tb;
    q.hk = gt ? (pgt ? pk : tb) : q.hk;
    q.hv = gt ? (pgt ? pv : (uint32_t)idx) : q.hv;
    q.nh++;
    q.h0 = tb < q.h0 ? tb : q.h0;
}
// pop the smallest (T, then oldest); -1 when empty (uniform)
__device__ __attribute__((always_inline)) inline int wq_pop(WQ &q)
{
    const bool cold = q.head < q.tail;
    if (!cold && q.nh == 0) return -1;
    const uint32_t cT = cold ? (uint32_t)__builtin_amdgcn_readfirstlane((int)q.preT) : 0xFFFFFFFFu;
    if (cold && cT <= q.h0) {
        int idx = __builtin_amdgcn_readfirstlane((int)q.preI);
        q.head++;
        wq_prefetch(q);
        return idx;
    }
    int idx = __builtin_amdgcn_readlane((int)q.hv, 0);
    q.hk = (uint32_t)__builtin_amdgcn_update_dpp((int)0xFFFFFFFF, (int)q.hk, 0x130, 0xf, 0xf, false);              // wave_shl1: lane l <- l+1
    q.hv = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)q.hv, 0x130, 0xf, 0xf, false);
    q.nh--;
    q.h0 = (uint32_t)__builtin_amdgcn_readlane((int)q.hk, 0);
    return idx;
}

// FMM quadrant solve (inpaint.cpp FastMarching_solve): a11 / a22 = T of the vertical / horizontal neighbour,
// k1 / k2 = that neighbour is not INSIDE
__device__ inline float wn_solve(double a11, double a22, bool k1, bool k2)
{
    // Branch-free: on a lone wave every divergent branch costs more than the arithmetic it skips.  sqrt(2 - d^2) is only used for
    // |d| < 1, i.e. an argument in (1, 2]: v_rsq_f64 and the two correction steps of the compiler's own f64 sqrt expansion, without
    // its denormal scaling -- bit-identical to sqrt() on that range.
    const double d = a11 - a22, m12 = a11 < a22 ? a11 : a22;
    const bool wide = fabs(d) >= 1.0;
    const double x = wide ? 2.0 : 2.0 - d * d;
    const double y = __builtin_amdgcn_rsq(x);
    double g = x * y, hh = 0.5 * y;
    const double r = fma(-hh, g, 0.5);
    g = fma(g, r, g);
    hh = fma(hh, r, hh);
    double e = fma(-g, g, x);
    g = fma(e, hh, g);
    e = fma(-g, g, x);
    g = fma(e, hh, g);
    const double both = wide ? 1.0 + m12 : (a11 + a22 + g) * 0.5;
    const double sol = k1 ? (k2 ? both : 1.0 + a11) : (k2 ? 1.0 + a22 : 1.0 + m12);
    return (float)sol;
}

// minimum over the four lanes of a quad (the four quadrant solves of one pixel), in each of them
__device__ __attribute__((always_inline)) inline float quad_min(float v)
{
    float o = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xf, 0xf, false)); v = o < v ? o : v;       // quad_perm [1,0,3,2]
    o = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xf, 0xf, false)); return o < v ? o : v;           // quad_perm [2,3,0,1]
}

// next seed (initial band pixel) in raster order, -1 when exhausted; (base, pend) is the scan state.  LDS = false: the flag plane is in
// global memory (the whole-frame kernel)
template <bool LDS = true>
__device__ inline int wn_next_seed(const uint8_t *f, int cells, int &base, unsigned long long &pend, int lane)
{
    while (!pend && base < cells) {
        int li = base + lane;
        pend = __ballot(li < cells && ((LDS ? f[li] : ld_relaxed<__HIP_MEMORY_SCOPE_WAVEFRONT>(f + li)) & W_SEED));
        if (!pend) base += 64;
    }
    if (!pend) return -1;
    int l = __ffsll((long long)pend) - 1;
    pend &= pend - 1;
    int p = base + l;
    if (!pend) base += 64;
    return p;
}

// ---- the per-pop bodies of the two passes, shared by every tier whose planes are padded (windows in LDS, padded planes in global memory) ----
struct TeleaWin {
    float *t, *im;          // LDS planes of the window: T field, image
    uint8_t *f;             // flag bytes
    int ww;                 // row pitch of the window
};
struct TeleaOutsideConsts { int dn, d1, d2; };       // lanes 0..15 = 4 neighbours x 4 quadrants
__device__ inline TeleaOutsideConsts telea_outside_consts(int lane, int ww)
{
    const int nb = (lane >> 2) & 3, qd = lane & 3;
    TeleaOutsideConsts c;
    c.dn = nb == 0 ? -ww : nb == 1 ? -1 : nb == 2 ? ww : 1;
    c.d1 = (qd & 1) ? ww : -ww;
    c.d2 = (qd & 2) ? 1 : -1;
    return c;
}
// this lane's neighbour offsets of the first two 64-neighbour chunks of the (2*range+1)^2 estimator window
struct TeleaMarchConsts {
    int off[2], d4, range, nn, side, r2;
    int ndisc;                  // window positions inside the disc dk^2 + dl^2 <= range^2
    float rx[2], ry[2], dstw[2];
    bool on[2];
};
// The disc enumeration: which position (dk, dl) of the (2 range + 1)^2 estimator window lane `lane` takes in chunk c2 (0 or 1), and whether
// it is inside the disc dk^2 + dl^2 <= range^2.  When the disc has at most 64 positions (range <= 4) lane i takes the i-th of them in
// row-major order: positions outside the disc never contribute, and the sequential sums then need ndisc - 1 steps instead of side^2 - 1.
// Larger ranges: all side^2 positions, row-major, 64 per chunk.
struct TeleaDisc {
    int nn, ndisc;              // positions enumerated (ndisc when compact, else side^2), positions inside the disc
    int dk[2], dl[2];
    bool on[2];
};
__host__ __device__ inline TeleaDisc telea_disc(int lane, int range)
{
    TeleaDisc c;
    const int side = 2 * range + 1, r2 = range * range;
    c.nn = side * side;
    int nd = 0, mine = -1;
    for (int i = 0; i < c.nn; i++) {
        const int dk = i / side - range, dl = i % side - range;
        if (dl * dl + dk * dk <= r2) { if (nd == lane) mine = i; nd++; }
    }
    c.ndisc = nd;
    const bool compact = nd <= 64;
    if (compact) c.nn = nd;                 // one chunk
#pragma unroll
    for (int c2 = 0; c2 < 2; c2++) {
        int nidx = c2 * 64 + lane;
        bool valid = nidx < c.nn;
        if (compact) { valid = c2 == 0 && mine >= 0; nidx = valid ? mine : 0; }
        c.dk[c2] = nidx / side - range; c.dl[c2] = nidx % side - range;
        c.on[c2] = valid && (c.dl[c2] * c.dl[c2] + c.dk[c2] * c.dk[c2] <= r2);
    }
    return c;
}
__device__ inline TeleaMarchConsts telea_march_consts(int lane, int ww, int range)
{
    TeleaMarchConsts c;
    c.range = range; c.r2 = range * range; c.side = 2 * range + 1;
    const TeleaDisc d = telea_disc(lane, range);
    c.nn = d.nn; c.ndisc = d.ndisc;
#pragma unroll
    for (int c2 = 0; c2 < 2; c2++) {
        c.on[c2] = d.on[c2];
        c.off[c2] = c.on[c2] ? d.dk[c2] * ww + d.dl[c2] : 0;              // lanes that are off may read, unused, the centre pixel
        float ry = (float)(-d.dk[c2]), rx = (float)(-d.dl[c2]);
        c.rx[c2] = rx; c.ry[c2] = ry;
        c.dstw[c2] = telea_dstw(rx, ry);
    }
    c.d4 = (lane & 3) == 0 ? -ww : (lane & 3) == 1 ? -1 : (lane & 3) == 2 ? ww : 1;    // up, left, down, right
    return c;
}

// fn(std::integral_constant<int, NS>) with NS = the disc's positions for the inpaint ranges 1..4 (5, 13, 29, 49: the straight-line estimator
// with that many lanes), anything else NS = OTHER (0: the chunk loop)
template <int OTHER = 0, class F>
__device__ __attribute__((always_inline)) inline void telea_dispatch_ndisc(int ndisc, F fn)
{
    switch (ndisc) {
    case 5: fn(std::integral_constant<int, 5>{}); break;
    case 13: fn(std::integral_constant<int, 13>{}); break;
    case 29: fn(std::integral_constant<int, 29>{}); break;
    case 49:
        if constexpr (OTHER != 49) { fn(std::integral_constant<int, 49>{}); break; }
        [[fallthrough]];
    default: fn(std::integral_constant<int, OTHER>{}); break;
    }
}

// Outside T field (icvCalcFMM with `negate`): a pop p (a seed of the initial band or a queue entry) gives every ring neighbour its T and
// pushes it.  States are those of OpenCV's `out` mask: ring = INSIDE, hole and everything else KNOWN.
// Up to FOUR pops of the outside pass at once.  A pop of this pass only uses 16 lanes (4 neighbours x 4 quadrants), so lane
// group g = lane >> 4 takes the g-th of the next entries IN QUEUE ORDER, as long as the one-at-a-time loop would have popped
// exactly these entries one after the other with the same data:
//  * a pop writes within Manhattan distance 1 of its pixel and reads within 2, so two entries at distance >= 4 do not see
//    each other's writes (telea_outside_prefix cuts the candidate list at the first pair that is closer);
//  * an entry pushed by an earlier member of the batch must not sort before a later member (T_new < T_member would put the new
//    entry first; T_new == T_member keeps the member first, FIFO): the batch is cut there before anything is written.
// Pushes go group by group, neighbour by neighbour -- the push order of the sequential loop -- so the queue contents, the FIFO
// order among equal T and every later pop are those of the sequential march: results are bit-identical.
// the longest prefix of n <= 4 candidates at (r, c) in which every pair is at Manhattan distance >= 4
__host__ __device__ inline int telea_prefix_by_distance(const int (&r)[4], const int (&c)[4], int n)
{
    int m = 1;
#pragma unroll
    for (int j = 1; j < 4; j++) {
        bool clash = false;
#pragma unroll
        for (int i = 0; i < j; i++) { int dr = r[i] - r[j], dc = c[i] - c[j]; clash = clash || (abs(dr) + abs(dc) < 4); }
        if (m == j && j < n && !clash) m = j + 1;
    }
    return m;
}
// `cells` = the candidate cells (wave-uniform), n = how many are valid; returns the longest admissible prefix by distance.  magic_ww == 0
// (telea_magic_plane: no exact row / column split on this plane): 1, one pop per step
__host__ __device__ inline int telea_outside_prefix(const int (&cells)[4], int n, int ww, uint32_t magic_ww)
{
    int r[4], c[4];
#pragma unroll
    for (int i = 0; i < 4; i++) { r[i] = (int)(((unsigned long long)(uint32_t)cells[i] * magic_ww) >> 32); c[i] = cells[i] - r[i] * ww; }     // multiply-high
    return magic_ww ? telea_prefix_by_distance(r, c, n) : 1;
}
// Where the FMM pass keeps its states: OpenCV's `out` flags in the window's flag bytes (outside pass: ring = INSIDE, hole and everything
// else KNOWN).  (A policy rather than plain code so that the pass reads the same whichever plane holds the states.)
struct FmmFlagState {
    float *t;
    uint8_t *f;
    __device__ __attribute__((always_inline)) bool inside(int c) const { return (f[c] & W_ST) == W_INSIDE; }
    __device__ __attribute__((always_inline)) void popped(int p, bool seed) const { f[p] = (uint8_t)(seed ? (W_SEED | W_CHANGE) : W_CHANGE); }   // ring pixels carry no other bit that matters
    __device__ __attribute__((always_inline)) void filled(int pn, float T, int) const { t[pn] = T; f[pn] = W_BAND; }
    __device__ __attribute__((always_inline)) void advance(int) {}
};

// cellT = the float bits of the candidates' T (all 0 for the seeds, which never wait for a push); commit(k) removes the k entries
// from the queue.  Returns the number of entries popped (1..m).
template <class State, class Commit, class Push>
__device__ __attribute__((always_inline)) inline int telea_pop_outside4(State &st, const TeleaOutsideConsts &oc, const int (&cells)[4],
                                                                        const uint32_t (&cellT)[4], int m, bool seed, int lane, Commit commit, Push push)
{
    float *t = st.t;
    const int dn = oc.dn, d1 = oc.d1, d2 = oc.d2;
    const int g = lane >> 4;
    const int p = g == 0 ? cells[0] : g == 1 ? cells[1] : g == 2 ? cells[2] : cells[3];
    const int pn = p + dn;
    const bool ok = g < m && st.inside(pn);
    unsigned long long okb = __ballot(ok);
    if (okb) {
        float dist = 0.f;
        if (ok) {
            const int p1 = pn + d1, p2 = pn + d2;
            float a11 = t[p1], a22 = t[p2];
            const bool k1 = !st.inside(p1), k2 = !st.inside(p2);           // p itself may be among them: BAND now, CHANGE after the pop -- not INSIDE either way
            dist = wn_solve(a11, a22, k1, k2);
        }
        dist = quad_min(dist);
        if (m > 1) {
            // smallest T pushed by each group (row = 16 lanes = one group); T >= 0, so the float bits order like the values
            uint32_t gm = ok ? __float_as_uint(dist) : 0x7f800000u, og;
            og = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)gm, 0x141, 0xf, 0xf, false); gm = og < gm ? og : gm;      // row_half_mirror
            og = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)gm, 0x140, 0xf, 0xf, false); gm = og < gm ? og : gm;      // row_mirror
            uint32_t run = (uint32_t)__builtin_amdgcn_readlane((int)gm, 0);
            int mc = 1;
            if (cellT[1] <= run) {
                mc = 2;
                const uint32_t g1 = (uint32_t)__builtin_amdgcn_readlane((int)gm, 16);
                run = g1 < run ? g1 : run;
                if (m > 2 && cellT[2] <= run) {
                    mc = 3;
                    const uint32_t g2 = (uint32_t)__builtin_amdgcn_readlane((int)gm, 32);
                    run = g2 < run ? g2 : run;
                    if (m > 3 && cellT[3] <= run) mc = 4;
                }
            }
            m = mc;
            okb &= m >= 4 ? ~0ull : (1ull << (16 * m)) - 1ull;
        }
        commit(m);                            // the m entries leave the queue before their pushes enter it
        if (g < m && (lane & 15) == 0) st.popped(p, seed);
        // the new band pixels are distinct cells (four neighbours of a pop; pops of a batch are >= 4 apart): their quad leaders store
        // T and the state together; only the queue insertions are ordered
        unsigned long long pb = okb & 0x1111111111111111ull;
        if ((pb >> lane) & 1ull) st.filled(pn, dist, __popcll(pb & ((1ull << lane) - 1ull)));     // numbered in push order
        st.advance(__popcll(pb));
        // pushes in the order of the sequential loop: pop by pop, neighbour by neighbour = ascending lane among the quad leaders
        while (pb) {
            const int l = __ffsll((long long)pb) - 1;
            pb &= pb - 1ull;
            push(wn_lane_f(dist, l), __builtin_amdgcn_readlane(pn, l));
        }
    } else {
        commit(m);
        if (g < m && (lane & 15) == 0) st.popped(p, seed);
    }
    return m;
}

// One whole FMM pass on a window: the seeds (cells with W_SEED in the flag bytes, T = 0) pop first in raster order, up to four per step out
// of the current 64-cell chunk, then the queue -- the next <= 4 entries in order are the first words of the cold run once no hot key
// precedes them.  np / ns count pops / steps (diagnostics).
// the seeds of one 64-cell chunk starting at cell `base` (pend = its lanes that hold a seed), up to four per step
template <class State>
__device__ __attribute__((always_inline)) inline void telea_fmm_seed_chunk(State &st, WQ &q, const TeleaOutsideConsts &oc, int base, unsigned long long pend,
                                                                           int ww, uint32_t magic_ww, int lane, unsigned long long &np, unsigned long long &ns)
{
    while (pend && !q.ovf) {
        int cand[4];
        unsigned long long rest = pend;
#pragma unroll
        for (int k = 0; k < 4; k++) { cand[k] = base + (int)(__ffsll((long long)rest) - 1); rest &= rest - 1ull; }    // ffs(0) - 1 = -1: masked by n
        const int npend = __popcll(pend);
        const uint32_t candT[4] = {0u, 0u, 0u, 0u};
        const int m = telea_pop_outside4(st, oc, cand, candT, telea_outside_prefix(cand, npend < 4 ? npend : 4, ww, magic_ww), true, lane,
                                         [](int) {}, [&](float T_, int idx_) { wq_push<false>(q, T_, idx_, lane); });
        pend &= pend - 1ull;
        if (m > 1) pend &= pend - 1ull;
        if (m > 2) pend &= pend - 1ull;
        if (m > 3) pend &= pend - 1ull;
        np += m;
        ns++;
    }
}
// the queue of an FMM pass until it is empty: the next <= 4 entries in order are the first words of the cold run once no hot key precedes them
template <class State>
__device__ __attribute__((always_inline)) inline void telea_fmm_queue(State &st, WQ &q, const TeleaOutsideConsts &oc, int ww, uint32_t magic_ww, int lane,
                                                                      unsigned long long &np, unsigned long long &ns)
{
    while (!q.ovf) {
        int cold_n = q.tail - q.head;
        if (cold_n == 0 && q.nh == 0) break;
        const int g = lane >> 4;
        unsigned long long wv = g < cold_n ? q.e[q.head + g] : 0ull;
        const uint32_t t3 = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(wv >> 32), 48);
        if (q.nh > 0 && (cold_n < 4 || q.h0 < t3)) {
            wq_merge<false>(q, lane);
            cold_n = q.tail - q.head;
            wv = g < cold_n ? q.e[q.head + g] : 0ull;
        }
        if (q.ovf) break;
        const int n = cold_n < 4 ? cold_n : 4;
        int cand[4];
#pragma unroll
        for (int k = 0; k < 4; k++) cand[k] = __builtin_amdgcn_readlane((int)(uint32_t)wv, 16 * k);
        uint32_t candT[4];
#pragma unroll
        for (int k = 0; k < 4; k++) candT[k] = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(wv >> 32), 16 * k);
        const int m = telea_pop_outside4(st, oc, cand, candT, telea_outside_prefix(cand, n, ww, magic_ww), false, lane,
                                         [&](int mc) { q.head += mc; }, [&](float T_, int idx_) { wq_push<false>(q, T_, idx_, lane); });
        np += m;
        ns++;
    }
}
// a whole pass over a window of `cells` cells (an LDS window: far below the magic's limit)
template <class State>
__device__ __attribute__((always_inline)) inline void telea_fmm_pass(State &st, WQ &q, const uint8_t *f, int cells, int ww, int lane,
                                                                     unsigned long long &np, unsigned long long &ns)
{
    const TeleaOutsideConsts oc = telea_outside_consts(lane, ww);
    const uint32_t magic_ww = telea_magic_ww(ww);
    __builtin_assume(magic_ww != 0u);
    for (int base = 0; base < cells && !q.ovf; base += 64) {
        const int li = base + lane;
        telea_fmm_seed_chunk(st, q, oc, base, __ballot(li < cells && (f[li] & W_SEED)), ww, magic_ww, lane, np, ns);
    }
    telea_fmm_queue(st, q, oc, ww, magic_ww, lane, np, ns);
}

// cycle sums of the fill's phases (frame 0 only): diagnostics of builds with -DVISTAF_DEBUG.  FSTART() starts a clock `fclk` that the fill
// block takes along; a fill that is not timed (the 16-wave kernel's) hands in a stopped one
#ifdef VISTAF_DEBUG
__device__ unsigned long long g_fill_dbg[8];
struct FillClock {
    unsigned long long t;
    bool on;
    __device__ explicit FillClock(bool on_) : t(__builtin_amdgcn_s_memtime()), on(on_) {}
    __device__ __attribute__((always_inline)) void stamp(int k, int lane)
    {
        if (on && blockIdx.x == 0 && lane == 0) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); g_fill_dbg[k] += t_ - t; t = t_; }
    }
};
#else
struct FillClock {
    __device__ explicit FillClock(bool) {}
    __device__ __attribute__((always_inline)) void stamp(int, int) {}
};
#endif
#define FSTART() FillClock fclk(true)
#define FSTAMP(k) fclk.stamp(k, lane)

// The image values of window position pk with OpenCV's index shifts at the first / last image row / column (km, kp, lm, lp; all 0 away
// from the image border); sk / sK / sl / sL = 1 where the neighbour above / below / left / right is a BORDER cell (bit 4 of its flag byte):
// vC the position's own value, vA / vB right / left, vE / vF below / above, vD / vG where the backward differences start (vC unless shifted)
struct TeleaImg { float vC, vA, vB, vD, vE, vF, vG; };
__device__ __attribute__((always_inline)) inline TeleaImg telea_img_taps(const float *im, int pk, int ww, int sk, int sK, int sl, int sL)
{
    const int rowm = pk + (sk ? ww : 0);
    TeleaImg v;
    v.vC = im[rowm + sl]; v.vA = im[rowm + 1 - sL]; v.vB = im[rowm + sl - 1]; v.vD = im[rowm - sL];
    v.vE = im[pk + (sK ? 0 : ww) + sl]; v.vF = im[rowm - ww + sl]; v.vG = im[pk - (sK ? ww : 0) + sl];
    return v;
}

// THE straight-line fill block: the estimate of pixel pi when the disc has NS <= 64 positions, one per lane.  ONE basic block: on a lone
// wave a taken branch costs tens of cycles and a dependent instruction ~9, so every LDS read is issued up front (the T word read at pi
// itself may be stale, but pi is INSIDE and never enters the sums), every condition is a per-lane select with all alternatives evaluated,
// and whatever centre() computes (the march: the quadrant solve, an f64 chain) overlaps the image-gradient terms.  Lanes that are off read,
// unused, around pi itself.
// centre(tu, tl, td, tr, ku, kl, kd, kr) returns the pixel's own T from T of its up / left / down / right neighbours and whether each is
// not INSIDE (per-lane values: as scalar conditions every select would become a branch); the block returns the estimate and leaves T in tc.
template <int NS, class Centre>
__device__ __attribute__((always_inline)) inline float telea_fill_block(const TeleaWin &win, const TeleaMarchConsts &mc, int pi, int lane, FillClock &fclk,
                                                                        float &tc, Centre centre)
{
    static_assert(NS > 0 && NS <= 64, "one estimator chunk");
    const float *t = win.t, *im = win.im;
    const uint8_t *f = win.f;
    const int ww = win.ww;
    const uint8_t f4 = f[pi + mc.d4];
    const float t4 = t[pi + mc.d4];
    const int pk = pi + mc.off[0];
    const uint8_t f0 = f[pk], fr = f[pk + 1], fl = f[pk - 1], fd = f[pk + ww], fu = f[pk - ww];
    const float tk = t[pk];
    const int sk = (fu >> 4) & 1, sK = (fd >> 4) & 1, sl = (fl >> 4) & 1, sL = (fr >> 4) & 1;
    const TeleaImg v = telea_img_taps(im, pk, ww, sk, sK, sl, sL);
    const float tu = wn_lane_f(t4, 0), tl = wn_lane_f(t4, 1), td = wn_lane_f(t4, 2), tr = wn_lane_f(t4, 3);
    unsigned kv = (unsigned)__ballot((f4 & W_ST) != W_INSIDE) & 0xf;
    asm volatile("" : "+v"(kv));
    const bool ku = kv & 1, kl = kv & 2, kd = kv & 4, kr = kv & 8;
    tc = centre(tu, tl, td, tr, ku, kl, kd, kr);
    FSTAMP(0);                     // LDS reads + the centre's T
    const float gtx = telea_grad_T(kr, kl, tr, tl, tc), gty = telea_grad_T(kd, ku, td, tu, tc);
    const float rx = mc.rx[0], ry = mc.ry[0];
    const bool use = (int)mc.on[0] & (int)((f0 & W_BORDER) == 0) & (int)((f0 & W_ST) != W_INSIDE);
    const float wgt = telea_weight(mc.dstw[0], telea_lev(tk, tc), telea_dir(rx, ry, gtx, gty));
    const bool nr = (fr & W_ST) != W_INSIDE, nl = (fl & W_ST) != W_INSIDE, nd = (fd & W_ST) != W_INSIDE, nu = (fu & W_ST) != W_INSIDE;
    TeleaTerms s = telea_terms(use, wgt, v.vC, telea_grad_I(nr, nl, v.vA, v.vB, v.vC, v.vD), telea_grad_I(nd, nu, v.vE, v.vF, v.vC, v.vG), rx, ry);
    FSTAMP(1);                     // weights and terms
    wn_seq_sum4<NS>(s.Ia, s.Jx, s.Jy, s.s, 1.0e-20f, lane);        // s starts at 1e-20f
    FSTAMP(2);                     // ordered sums
    return telea_estimate(s.Ia, s.Jx, s.Jy, s.s);
}

// Telea march (icvTeleaInpaintFMM): pop p, fill every 4-neighbour that is still INSIDE and push it.  Returns the number of
// pixels filled.
// NS > 0: the disc of the estimator window has NS <= 64 positions, one per lane (telea_march_consts), the case of every shipped
// configuration (range 3: 29); NS == 0: general chunk loop.
template <int NS, class Push>
__device__ __attribute__((always_inline)) inline int telea_pop_march(const TeleaWin &win, const TeleaMarchConsts &mc, int p, bool from_queue, int lane,
                                                                     Push push)
{
    float *t = win.t, *im = win.im;
    uint8_t *f = win.f;
    const int ww = win.ww, d4 = mc.d4, range = mc.range, nn = mc.nn, side = mc.side, r2 = mc.r2;
    int nfill = 0;
    if (from_queue && lane == 0) f[p] = (uint8_t)(W_HOLE | W_KNOWN);
    // the four 4-neighbours, one per lane: still INSIDE?  (a neighbour's fill never changes another's flag)
    unsigned todo = (unsigned)(__ballot(lane < 4 && (f[p + d4] & W_ST) == W_INSIDE) & 0xf);
    while (todo) {
        const int qn = __ffs((int)todo) - 1;
        todo &= todo - 1;
        const int pi = p + (qn == 0 ? -ww : qn == 1 ? -1 : qn == 2 ? ww : 1);
        nfill++;
        // T of pi: the minimum over the quadrants (i-1,j-1) (i+1,j-1) (i-1,j+1) (i+1,j+1), one per lane of a quad
        auto solve = [&](float tu, float tl, float td, float tr, bool ku, bool kl, bool kd, bool kr) -> float {
            const int qd = lane & 3;
            const float T = wn_lane_f(quad_min(wn_solve((qd & 1) ? td : tu, (qd & 2) ? tr : tl, (qd & 1) ? kd : ku, (qd & 2) ? kr : kl)), 0);
            if (lane == 0) t[pi] = T;
            return T;
        };
        if constexpr (NS > 0) {
            FSTART();
            float tc;
            const float val = telea_fill_block<NS>(win, mc, pi, lane, fclk, tc, solve);
            if (lane == 0) { im[pi] = val; f[pi] = (uint8_t)(W_HOLE | W_BAND); }
            FSTAMP(3);                     // final estimate + stores
            push(tc, pi);
            FSTAMP(4);                     // queue push
            continue;
        }
        // (flag, T) of pi's up / left / down / right neighbours on lanes 0..3, shared by all lanes
        const uint8_t f4 = f[pi + d4];
        const float t4 = t[pi + d4];
        const float tu = wn_lane_f(t4, 0), tl = wn_lane_f(t4, 1), td = wn_lane_f(t4, 2), tr = wn_lane_f(t4, 3);
        const unsigned kk = (unsigned)__ballot((f4 & W_ST) != W_INSIDE) & 0xf;
        const bool ku = kk & 1, kl = kk & 2, kd = kk & 4, kr = kk & 8;
        const float tc = solve(tu, tl, td, tr, ku, kl, kd, kr);
        __builtin_amdgcn_wave_barrier();
        const float gtx = telea_grad_T(kr, kl, tr, tl, tc), gty = telea_grad_T(kd, ku, td, tu, tc);
        float Ia = 0.f, Jx = 0.f, Jy = 0.f, s = 1.0e-20f;       // running sums in OpenCV's order: chunk after chunk, lane after lane
        for (int n0 = 0; n0 < nn; n0 += 64) {
            TeleaTerms a = {0.f, 0.f, 0.f, 0.f};
            int off;
            float dstw, rx, ry;
            bool on;
            if (n0 < 128) { int c2 = n0 >> 6; off = mc.off[c2]; dstw = mc.dstw[c2]; on = mc.on[c2]; rx = mc.rx[c2]; ry = mc.ry[c2]; }
            else {
                int nidx = n0 + lane;
                int dk = nidx / side - range, dl = nidx % side - range;
                off = dk * ww + dl;
                on = nidx < nn && (dl * dl + dk * dk <= r2);
                ry = (float)(-dk); rx = (float)(-dl);
                dstw = telea_dstw(rx, ry);
            }
            if (on) {
                const int pk = pi + off;                      // inside the window: margin range+1
                const uint8_t f0 = f[pk], fr = f[pk + 1], fl = f[pk - 1], fd = f[pk + ww], fu = f[pk - ww];
                const float tk = t[pk];
                TeleaImg v;
                v.vC = im[pk]; v.vA = im[pk + 1]; v.vB = im[pk - 1]; v.vE = im[pk + ww]; v.vF = im[pk - ww];
                if (!(f0 & W_BORDER) && (f0 & W_ST) != W_INSIDE) {
                    v.vD = v.vC; v.vG = v.vC;
                    if ((fr | fl | fd | fu) & W_BORDER)
                        v = telea_img_taps(im, pk, ww, (fu >> 4) & 1, (fd >> 4) & 1, (fl >> 4) & 1, (fr >> 4) & 1);      // shifted at the image border: read again
                    const float wgt = telea_weight(dstw, telea_lev(tk, tc), telea_dir(rx, ry, gtx, gty));
                    const bool nr = (fr & W_ST) != W_INSIDE, nl = (fl & W_ST) != W_INSIDE, nd = (fd & W_ST) != W_INSIDE, nu = (fu & W_ST) != W_INSIDE;
                    a = telea_terms(true, wgt, v.vC, telea_grad_I(nr, nl, v.vA, v.vB, v.vC, v.vD), telea_grad_I(nd, nu, v.vE, v.vF, v.vC, v.vG), rx, ry);
                }
            }
            const int nl = nn - n0 < 64 ? nn - n0 : 64;
            Ia = wn_seq_sum_n(a.Ia, Ia, nl, lane); Jx = wn_seq_sum_n(a.Jx, Jx, nl, lane); Jy = wn_seq_sum_n(a.Jy, Jy, nl, lane); s = wn_seq_sum_n(a.s, s, nl, lane);
        }
        const float val = telea_estimate(Ia, Jx, Jy, s);
        if (lane == 0) { im[pi] = val; f[pi] = (uint8_t)(W_HOLE | W_BAND); }
        push(tc, pi);
    }
    return nfill;
}

// The estimate of ONE hole pixel pi whose T the ordering pass (k_inpaint_mw.hip) has already fixed: the fill block of telea_pop_march without
// the quadrant solve and the push (so the value carries the same bits).  The caller guarantees that
// every fill within Chebyshev distance range + 1 of pi runs in march order (the block reads flags, T and image values that far out):
// then "flag != INSIDE" in the live flag bytes is exactly the flag history cv::inpaint's march would have seen at this fill.
// (T of cells that are still INSIDE already holds its final value instead of 1e6; every use of it is masked by the cell's flag.)
template <int NS>
__device__ __attribute__((always_inline)) inline void telea_fill_known_T(const TeleaWin &win, const TeleaMarchConsts &mc, int pi, int lane)
{
    const float tcl = win.t[pi];
    FillClock fclk(false);
    float tc;
    const float val = telea_fill_block<NS>(win, mc, pi, lane, fclk, tc, [&](float, float, float, float, bool, bool, bool, bool) { return wn_lane_f(tcl, 0); });
    if (lane == 0) { win.im[pi] = val; win.f[pi] = (uint8_t)(W_HOLE | W_BAND); }
}

}  // namespace vf
