// Exact order statistics per frame (one 1024-thread workgroup per frame).
//
// Replaces np.percentile / np.nanpercentile / np.median / np.nanmedian on the masked, finite values
// of a plane (shape_ftp.py:343-354, :618-622, :1124-1125).  The two neighbouring order statistics
// are found EXACTLY (range-adaptive 2048-bucket histogram refinement over order-preserving uint32
// keys, then rank-by-counting of <=1024 candidates in LDS); the interpolation then follows NumPy
// 2.x's float32 arithmetic (numpy/lib/_function_base_impl.py `_quantile`, `_lerp`) so thresholds
// equal the CPU path's to the last bit whenever the inputs do.
#pragma once
#include "common.hpp"

namespace vf {

#ifndef SEL_STAMP
#define SEL_STAMP(i) do { } while (0)      // diagnostics hook (k_fit.hip, -DVISTAF_DEBUG)
#endif

constexpr int SEL_T = 1024;
constexpr int SEL_BITS = 13;          // histogram digits: 8192 buckets, 8 per thread in the bucket search
constexpr int SEL_NB = 1 << SEL_BITS;
constexpr int SEL_CAND = 1024;

struct SelShared {
    uint32_t hist[SEL_NB];
    uint32_t cand[SEL_CAND];
    unsigned long long red64[16];
    uint32_t wsum[16];
    uint32_t s_bucket, s_before, s_cnt, s_ncand, s_a, s_b, s_found;
};

// ---- the rules every dataflow shares (k_select.hip, k_fit.hip, k_big.hip); tests/diag/fit_select_host_check.hip runs the host-callable ones
#define SEL_RULE __device__ __attribute__((always_inline)) inline
#define SEL_HRULE __host__ __device__ __attribute__((always_inline)) inline

// Element rule: is the plane element (mask byte mk, value x) part of the selection, and its key.  le: the frame's threshold, or null.
SEL_RULE bool sel_element(uint8_t mk, float x, bool use_abs, const float *le, uint32_t &key)
{
    bool ok = mk != 0 && finitef(x);
    if (use_abs) x = fabsf(x);
    if (le && !(x <= *le)) ok = false;
    key = f2key(x);
    return ok;
}

// Key range: count, smallest and largest key of the valid elements.  add() per element and thread; reduce() over the workgroup (blockDim.x
// <= 1024, s32 / s64: 16 entries each), result in all threads.  All threads must have passed a barrier since s32 / s64 were last read,
// and must pass one before they are written again.  with_extra: a second per-thread count is summed in between (the fit's mask pixels).
struct SelRange {
    uint32_t c = 0;
    unsigned long long mn = ~0ull, mx = 0;          // smallest key; largest key + 1 (0: none)
    SEL_RULE void add(uint32_t key) { c++; if (key < mn) mn = key; if (key + 1ull > mx) mx = key + 1ull; }
    SEL_RULE void reduce(uint32_t *s32, unsigned long long *s64, uint32_t &n, uint32_t &kmin, uint32_t &kmax, bool with_extra, uint32_t &extra) const
    {
        n = block_sum<uint32_t>(c, s32);
        if (with_extra) extra = block_sum<uint32_t>(extra, s32);
        const unsigned long long bmn = block_min_u64(mn, s64), bmx = block_max_u64(mx, s64);
        kmin = (uint32_t)bmn; kmax = bmx ? (uint32_t)(bmx - 1) : 0;
    }
    SEL_RULE void reduce(uint32_t *s32, unsigned long long *s64, uint32_t &n, uint32_t &kmin, uint32_t &kmax) const
    {
        uint32_t none = 0;
        reduce(s32, s64, n, kmin, kmax, false, none);
    }
};

// NumPy 2.x percentile (method 'linear') of float32 data, float32 arithmetic.  The linear method has its own virtual index,
// (n - 1) * q (numpy/lib/_function_base_impl.py: _QuantileMethods['linear']), not the general n*q + (alpha + q*(1 - alpha - beta)) - 1:
//   vi = (n-1)*q ; prev = floor(vi) ; gamma = vi - prev
//   res = a + (b-a)*gamma  [ b - (b-a)*(1-gamma) when gamma >= 0.5 ]
// (The general form rounds differently in float32 and moved the result by a few ulps: [-2.5, 7] at q = 8 gave 0xbfdeb84e for 0xbfdeb852.)
__host__ __device__ inline void np_percentile_index(uint32_t n, float q32, uint32_t &k, float &gamma, bool &top)
{
    const float vi = rn_mul((float)(n - 1), q32);
    top = vi >= (float)(n - 1);
    if (vi < 0.0f) { k = 0; gamma = 0.0f; return; }
    float pf = floorf(vi);
    k = (uint32_t)pf;
    gamma = rn_sub(vi, pf);
    if (top) { k = n - 1; gamma = 0.0f; }
}
__host__ __device__ inline float np_lerp(float a, float b, float t)
{
    float d = rn_sub(b, a);
    float r = rn_add(a, rn_mul(d, t));
    if (t >= 0.5f) r = rn_sub(b, rn_mul(d, rn_sub(1.0f, t)));
    return r;
}

// Plan of one request over n valid elements with keys in [kmin, kmax]; q = float32(percent) / float32(100), q < 0: np.median.  Either the
// result is known (no element: the quiet NaN; a median of one element; a rank at the top: the maximum) or the keys of rank k and k + 1 are
// wanted and sel_result turns them into the float: the lower one alone (median, odd n), their float32 mean (median, even n), np_lerp.
// The kind is worked out from (n, q) where it is needed: held as a value of its own across a selection it cost the resident kernels a
// register per thread (k_select_resident<64>: two more spilled).
enum : uint32_t { SEL_ONE = 0, SEL_MEAN2 = 1, SEL_LERP = 2 };
struct SelPlan {
    bool done; float result; uint32_t k; float gamma; uint32_t n; float q;
    __host__ __device__ uint32_t kind() const { return q < 0.f ? ((n & 1u) ? SEL_ONE : SEL_MEAN2) : SEL_LERP; }
};
SEL_HRULE SelPlan sel_plan(uint32_t n, float q, uint32_t kmin, uint32_t kmax)
{
    SelPlan p = {true, 0.f, 0u, 0.f, n, q};
    if (n == 0) p.result = nanf32();
    else if (q < 0.f) {
        if (n == 1) p.result = key2f(kmin);
        else { p.done = false; p.k = (n & 1u) ? (n - 1) / 2 : n / 2 - 1; p.gamma = 0.5f; }
    } else {
        bool top;
        np_percentile_index(n, q, p.k, p.gamma, top);
        if (p.k + 1 >= n) p.result = key2f(kmax);          // last element: both neighbours are the maximum
        else p.done = false;
    }
    return p;
}
SEL_HRULE float sel_result_kind(uint32_t kind, float gamma, uint32_t key_a, uint32_t key_b)
{
    const float a = key2f(key_a), b = key2f(key_b);
    if (kind == SEL_LERP) return np_lerp(a, b, gamma);
    return kind == SEL_MEAN2 ? rn_div(rn_add(a, b), 2.0f) : a;
}
SEL_HRULE float sel_result(const SelPlan p, uint32_t key_a, uint32_t key_b) { return sel_result_kind(p.kind(), p.gamma, key_a, key_b); }

// Level rules of the histogram refinement over the keys in [lo, hi], BITS digits per level: a key falls into bucket (key - lo) >> sel_shift
SEL_HRULE int sel_shift(uint32_t lo, uint32_t hi, int BITS)
{
    const uint32_t range = hi - lo;
    const int bits = range ? 32 - __builtin_clz(range) : 0;
    return bits > BITS ? bits - BITS : 0;
}
// [lo, hi] narrowed to the chosen bucket.  The last bucket of a level is clipped at hi; `nhi < nlo` is the bucket that wraps past 2^32.
struct SelSpan { uint32_t lo, hi; };
SEL_HRULE SelSpan sel_narrow(uint32_t lo, uint32_t hi, uint32_t bucket, uint32_t shift)
{
    const uint32_t nlo = lo + (bucket << shift);
    uint32_t nhi = shift ? nlo + ((1u << shift) - 1u) : nlo;
    if (nhi > hi || nhi < nlo) nhi = hi;
    return {nlo, nhi};
}
// The next level's width is NOT shared.  The per-frame code (block_select2_each) calls sel_shift on the narrowed range again; the chain
// (k_big.hip: k_sb_pick) takes BITS digits off the previous width, so that its three launches per selection are fixed in advance.  The two
// differ when the last bucket was clipped at hi (the narrowed range is then shorter than a bucket); both end at one key within three levels.
SEL_HRULE uint32_t sel_shift_chain_next(uint32_t shift, int BITS) { return shift > (uint32_t)BITS ? shift - (uint32_t)BITS : 0u; }
// The next order statistic after the key a of rank k: a again if it is duplicated (k + 1 < cnt_le, the number of keys <= a) or nothing lies
// above (min_gt, the smallest key above a, is all ones: no valid key is), else min_gt.
template <class K>
SEL_HRULE uint32_t sel_next(uint32_t k, uint32_t cnt_le, K min_gt, uint32_t a) { return (k + 1 < cnt_le || min_gt == (K) ~(K)0) ? a : (uint32_t)min_gt; }

// Visit every valid element (get(i, key) -> bool valid), SEL_U elements per thread at a time: the SEL_U loads of a
// batch are issued together, so a pass costs P / (SEL_T * SEL_U) memory round trips per thread instead of P / SEL_T.
constexpr int SEL_U = 8;
template <class F, class B>
__device__ inline void sel_foreach(F get, int P, B body)
{
    int i = threadIdx.x;
    for (; i + (SEL_U - 1) * SEL_T < P; i += SEL_U * SEL_T) {
        uint32_t key[SEL_U];
        bool ok[SEL_U];
#pragma unroll
        for (int u = 0; u < SEL_U; u++) ok[u] = get(i + u * SEL_T, key[u]);
#pragma unroll
        for (int u = 0; u < SEL_U; u++)
            if (ok[u]) body(key[u]);
    }
    for (; i < P; i += SEL_T) {
        uint32_t key;
        if (get(i, key)) body(key);
    }
}

// Finds keys of rank k and k+1 (ascending, 0-based) among the n valid elements.
// each(body) calls body(key) for every valid element of this thread (the same elements on every call).
// n must be > 0 and k < n.  Result in all threads.
// NT: threads of the workgroup (a power of two, 256 <= NT <= 1024; the candidate list is limited to NT entries, one per thread of the sort).
template <int NT = SEL_T, class Each>
__device__ __attribute__((always_inline)) inline void block_select2_each(Each each, uint32_t n, uint32_t k, SelShared &sh, uint32_t kmin, uint32_t kmax,
                                                                         uint32_t &key_a, uint32_t &key_b)
{
    static_assert(NT >= 256 && NT <= SEL_T && (NT & (NT - 1)) == 0, "workgroup size");
    constexpr uint32_t CAND = NT < SEL_CAND ? NT : SEL_CAND;
    const int tid = threadIdx.x;
    uint32_t lo = kmin, hi = kmax, below = 0;
    uint32_t a = 0, b = 0;
    for (;;) {
        if (hi == lo) { a = lo; break; }
        const int shift = sel_shift(lo, hi, SEL_BITS);
        for (int i = tid; i < SEL_NB; i += NT) sh.hist[i] = 0;
        __syncthreads();
        SEL_STAMP(0);
        each([&](uint32_t key) { if (key >= lo && key <= hi) atomicAdd(&sh.hist[(key - lo) >> shift], 1u); });
        __syncthreads();
        SEL_STAMP(1);
        // locate the bucket holding rank (k - below): each thread owns SEL_NB / SEL_T consecutive buckets
        uint32_t want = k - below;
        constexpr int NBT = SEL_NB / NT;
        uint32_t cb[NBT];
        uint32_t mine = 0;
#pragma unroll
        for (int j = 0; j < NBT; j++) { cb[j] = sh.hist[NBT * tid + j]; mine += cb[j]; }
        // exclusive prefix over threads: wave scan + wave totals
        int lane = tid & 63, wid = tid >> 6;
        uint32_t incl = wave_scan_add(mine);
        if (lane == 63) sh.wsum[wid] = incl;
        __syncthreads();
        uint32_t wbase = 0;
        for (int i = 0; i < wid; i++) wbase += sh.wsum[i];
        uint32_t excl = wbase + incl - mine;
        if (want >= excl && want < excl + mine) {
            uint32_t run = excl;
#pragma unroll
            for (int j = 0; j < NBT; j++) {
                if (want >= run && want < run + cb[j]) { sh.s_bucket = NBT * tid + j; sh.s_before = run; sh.s_cnt = cb[j]; }
                run += cb[j];
            }
        }
        __syncthreads();
        uint32_t bsel = sh.s_bucket, cnt = sh.s_cnt;
        below += sh.s_before;
        const SelSpan nx = sel_narrow(lo, hi, bsel, (uint32_t)shift);
        lo = nx.lo; hi = nx.hi;
        __syncthreads();
        SEL_STAMP(2);
        if (shift == 0) { a = lo; break; }
        if (cnt <= CAND) {
            // collect candidates of this bucket, rank by counting
            if (tid == 0) sh.s_ncand = 0;
            __syncthreads();
            each([&](uint32_t key) {
                // one counter update per wave and visit: the lanes holding a candidate take consecutive slots
                const bool in = key >= lo && key <= hi;
                const unsigned long long mk = __ballot(in);
                if (in) {
                    const int ln = threadIdx.x & 63, leader = __ffsll((long long)mk) - 1;
                    uint32_t base = 0;
                    if (ln == leader) base = atomicAdd(&sh.s_ncand, (uint32_t)__popcll(mk));
                    base = (uint32_t)__builtin_amdgcn_readlane((int)base, leader);
                    const uint32_t pos = base + (uint32_t)__popcll(mk & ((1ull << ln) - 1ull));
                    if (pos < CAND) sh.cand[pos] = key;
                }
            });
            __syncthreads();
            SEL_STAMP(3);
            uint32_t m = sh.s_ncand;
            const uint32_t want2 = k - below;
            if (tid == 0) { sh.s_found = 0; }
            __syncthreads();
            if (m > CAND) m = CAND;                                  // cannot happen (cnt <= SEL_CAND); keeps the indices in range
            // sort the candidates (bitonic network in LDS, padded with the largest key to a power of two >= 64): the two order
            // statistics are then read off by index.  Partners closer than 64 live in the same wave, whose LDS operations execute
            // in order, so only the wider exchanges and the start of a new merge round need a workgroup barrier.
            const uint32_t np2 = m <= 64u ? 64u : 1u << (32 - __clz(m - 1u));
            if ((uint32_t)tid >= m && (uint32_t)tid < np2) sh.cand[tid] = 0xFFFFFFFFu;
            __syncthreads();
            for (uint32_t k2 = 2; k2 <= np2; k2 <<= 1) {
                for (uint32_t j = k2 >> 1; j > 0; j >>= 1) {
                    const uint32_t ixj = (uint32_t)tid ^ j;
                    if ((uint32_t)tid < np2 && ixj > (uint32_t)tid) {
                        const uint32_t x = sh.cand[tid], y = sh.cand[ixj];
                        const bool up = ((uint32_t)tid & k2) == 0u;
                        if ((x > y) == up) { sh.cand[tid] = y; sh.cand[ixj] = x; }
                    }
                    if (j >= 64u || (j == 1u && k2 >= 64u)) __syncthreads();
                    else __builtin_amdgcn_wave_barrier();
                }
            }
            if (tid == 0) {
                sh.s_a = sh.cand[want2];
                if (want2 + 1 < m) { sh.s_b = sh.cand[want2 + 1]; sh.s_found = 1; }
            }
            __syncthreads();
            SEL_STAMP(4);
            a = sh.s_a;
            if (sh.s_found) { key_a = a; key_b = sh.s_b; __syncthreads(); return; }
            break;
        }
    }
    // b = next order statistic: a again if duplicated, else the smallest key above a
    {
        uint32_t le = 0;
        unsigned long long nxt = ~0ull;
        each([&](uint32_t key) { le += key <= a; if (key > a && (unsigned long long)key < nxt) nxt = key; });
        __syncthreads();
        uint32_t tot = block_sum<uint32_t>(le, sh.wsum);
        unsigned long long mn = block_min_u64(nxt, sh.red64);
        b = sel_next(k, tot, mn, a);
        __syncthreads();
        SEL_STAMP(5);
    }
    key_a = a; key_b = b;
}

// get(i, key) -> bool valid over the P elements of a plane
template <class F>
__device__ inline void block_select2(F get, int P, uint32_t n, uint32_t k, SelShared &sh, uint32_t kmin, uint32_t kmax,
                                     uint32_t &key_a, uint32_t &key_b)
{
    block_select2_each<SEL_T>([&](auto body) { sel_foreach(get, P, body); }, n, k, sh, kmin, kmax, key_a, key_b);
}

// count / min / max of valid keys
template <class F>
__device__ inline void block_minmax(F get, int P, SelShared &sh, uint32_t &n, uint32_t &kmin, uint32_t &kmax)
{
    SelRange rg;
    sel_foreach(get, P, [&](uint32_t key) { rg.add(key); });
    __syncthreads();
    rg.reduce(sh.wsum, sh.red64, n, kmin, kmax);
    __syncthreads();
}

// percentile (q32 = float32(q)/float32(100) >= 0) of valid elements; NaN when n == 0
template <class F>
__device__ inline float block_percentile(F get, int P, float q32, SelShared &sh, uint32_t n, uint32_t kmin, uint32_t kmax)
{
    const SelPlan p = sel_plan(n, q32, kmin, kmax);
    if (p.done) return p.result;
    uint32_t ka, kb;
    block_select2(get, P, n, p.k, sh, kmin, kmax, ka, kb);
    return sel_result(p, ka, kb);
}

// np.median of valid elements (mean of the two middle values in float32 for even n)
template <int NT = SEL_T, class Each>
__device__ __attribute__((always_inline)) inline float block_median_each(Each each, SelShared &sh, uint32_t n, uint32_t kmin, uint32_t kmax)
{
    const SelPlan p = sel_plan(n, -1.f, kmin, kmax);
    if (p.done) return p.result;
    uint32_t ka, kb;
    block_select2_each<NT>(each, n, p.k, sh, kmin, kmax, ka, kb);
    return sel_result(p, ka, kb);
}
template <class F>
__device__ inline float block_median(F get, int P, SelShared &sh, uint32_t n, uint32_t kmin, uint32_t kmax)
{
    return block_median_each<SEL_T>([&](auto body) { sel_foreach(get, P, body); }, sh, n, kmin, kmax);
}

#undef SEL_RULE
#undef SEL_HRULE

}  // namespace vf
