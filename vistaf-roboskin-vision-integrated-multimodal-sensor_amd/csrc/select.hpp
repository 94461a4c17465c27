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
#ifndef SEL_COUNT_M
#define SEL_COUNT_M(m) do { } while (0)    // diagnostics hook: the count of a level's chosen bucket (k_fit.hip, -DVISTAF_DEBUG)
#endif

constexpr int SEL_T = 1024;
constexpr int SEL_BITS = 13;          // histogram digits: 8192 buckets, 8 per thread in the bucket search
constexpr int SEL_NB = 1 << SEL_BITS;
constexpr int SEL_CAND = 1024;
// Candidate lists of up to SEL_RANK_MAX keys are finished by counting (sel_rank_vote), longer ones by the bitonic network.  The count costs
// a wave three VALU instructions per candidate (v_readlane, compare, add with carry), about 12 m cycles of its SIMD; up to 256 candidates
// are four waves, one per SIMD, beyond that the waves queue up behind each other and the network's fixed ladder of exchanges and barriers
// is the shorter way
constexpr uint32_t SEL_RANK_MAX = 256;
constexpr uint32_t SEL_PAD = 0xFFFFFFFFu;          // the largest key: pads the candidate list, is no valid element's key

// hist is all zeros whenever no level of a selection is between its sweep and its bucket search: sel_init zeroes it once per kernel, the
// bucket search zeroes what it has read.
struct SelShared {
    alignas(16) uint32_t hist[SEL_NB];
    uint32_t cand[SEL_CAND];              // read four bytes per lane by the count: no alignment of its own (hist is read 16 bytes at a time)
    unsigned long long red64[16];
    uint32_t wsum[16];
    uint32_t s_bucket, s_before, s_cnt, s_ncand, s_a, s_b, s_found;
};
static_assert(SEL_CAND % 64 == 0 && SEL_RANK_MAX % 64 == 0 && SEL_RANK_MAX >= 64 && SEL_RANK_MAX <= 256, "the rank count pads the list to whole waves; NT >= 256 threads hold them");

// Once per kernel, before the first selection; the workgroup must pass a barrier between this and the first selection's sweep.
template <int NT = SEL_T>
__device__ inline void sel_init(SelShared &sh)
{
    for (int i = threadIdx.x; i < SEL_NB; i += NT) sh.hist[i] = 0;
}

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

// Finish by counting: a key x of the candidate list with `less` candidates below it holds the ranks from `less` on, up to the next larger
// key's count.  So the order statistic of rank `want` is the largest key whose count is <= want: every candidate votes its key or nothing
// (0, below or equal to every key), and the maximum of the votes is the statistic.  Equal keys have equal counts and vote alike.  The pads at
// the end of the list (SEL_PAD) are below no key, and have every real candidate below them: m > want, no vote.
SEL_HRULE uint32_t sel_rank_vote(uint32_t x, uint32_t less, uint32_t want) { return less <= want ? x : 0u; }

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
// n must be > 0 and k < n.  Result in all threads.  With SELF, sel_init(sh) and a barrier must have come before the kernel's first call.
// The barriers of a level: A histogram complete, B wave totals, C chosen bucket, D candidates complete, E finish.  Each LDS word, its last
// reader and its next writer (the next level or the next call), and the barriers between them:
//   hist                    read and zeroed before B (search)       atomics of the next sweep                  B, C
//   wsum                    read between B and C                    after the next A                           C, A
//   s_bucket, before, cnt   read after C                            finder thread, after the next A and B      A, B
//   s_ncand, s_found        read after D / after E                  finder thread, after the next A and B      A, B
//   s_a, s_b                read after E                            finder thread, after the next A and B      A, B
//   cand                    read between D and E                    pads and collection, after the next C      A, B, C
//   wsum, red64 of the second statistic's sweep: read behind that block's own barriers, which every thread passes before it returns
// So a call needs no barrier behind it for its own sake; callers that use sh.wsum / sh.red64 themselves keep SelRange's rule.
// A selection decided at its first level executes five barriers up to SEL_RANK_MAX candidates (A .. E); above, D is followed by the pad
// barrier and the network's 10 (up to 512 candidates) or 15 (up to 1024) before E: 16 or 21.
// NT: threads of the workgroup (a power of two, 256 <= NT <= 1024; the candidate list is limited to NT entries, one per thread of the sort).
// SELF: the histogram cleans itself and the level words need no barriers of their own (see the table above).  false: the level keeps the
// bookkeeping it had before -- a clear loop and its barrier in front of the sweep, a barrier behind the reads of the level words, thread 0
// opening the collection behind a barrier, a barrier before a found pair returns -- and needs no sel_init.  The plain column fits take it:
// their register allocation is the better for it (k_fit.hip).
template <int NT = SEL_T, bool SELF = true, class Each>
__device__ __attribute__((always_inline)) inline void block_select2_each(Each each, uint32_t n, uint32_t k, SelShared &sh, uint32_t kmin, uint32_t kmax,
                                                                         uint32_t &key_a, uint32_t &key_b)
{
    static_assert(NT >= 256 && NT <= SEL_T && (NT & (NT - 1)) == 0, "workgroup size");
    static_assert(SEL_RANK_MAX <= (uint32_t)NT, "the padded list is held by whole waves of the workgroup");
    constexpr uint32_t CAND = NT < SEL_CAND ? NT : SEL_CAND;
    const int tid = threadIdx.x;
    uint32_t lo = kmin, hi = kmax, below = 0;
    uint32_t a = 0, b = 0;
    for (;;) {
        if (hi == lo) { a = lo; break; }
        const int shift = sel_shift(lo, hi, SEL_BITS);
        if constexpr (!SELF) {
            for (int i = tid; i < SEL_NB; i += NT) sh.hist[i] = 0;
            __syncthreads();
        }
        SEL_STAMP(0);
        // the histogram is all zeros here (SelShared): no clear, and no barrier in front of the sweep -- whoever last read a word that this
        // level writes has passed a barrier since (the levels' own, the callers' after a selection)
        each([&](uint32_t key) { if (key >= lo && key <= hi) atomicAdd(&sh.hist[(key - lo) >> shift], 1u); });
        __syncthreads();
        SEL_STAMP(1);
        // locate the bucket holding rank (k - below): each thread owns SEL_NB / NT consecutive buckets, and zeroes them once it holds them
        uint32_t want = k - below;
        constexpr int NBT = SEL_NB / NT;
        static_assert(NBT % 4 == 0, "a thread's buckets are read and zeroed 16 bytes at a time");
        uint32_t cb[NBT];
        uint32_t mine = 0;
        {
            uint4 *h4 = reinterpret_cast<uint4 *>(&sh.hist[NBT * tid]);
#pragma unroll
            for (int j = 0; j < NBT / 4; j++) {
                const uint4 c = h4[j];
                cb[4 * j] = c.x; cb[4 * j + 1] = c.y; cb[4 * j + 2] = c.z; cb[4 * j + 3] = c.w;
            }
            if constexpr (SELF) {
#pragma unroll
                for (int j = 0; j < NBT / 4; j++) h4[j] = make_uint4(0u, 0u, 0u, 0u);
            }
#pragma unroll
            for (int j = 0; j < NBT; j++) mine += cb[j];
        }
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
            if constexpr (SELF) { sh.s_ncand = 0; sh.s_found = 0; sh.s_a = 0; sh.s_b = 0; }
        }
        __syncthreads();
        // (wave-uniform, and said so: lo, hi and below then live in scalar registers across the sweeps, not in vector registers next to the samples)
        uint32_t bsel = sh.s_bucket, cnt = sh.s_cnt, before = sh.s_before;
        if constexpr (SELF) {
            bsel = (uint32_t)__builtin_amdgcn_readfirstlane((int)bsel); cnt = (uint32_t)__builtin_amdgcn_readfirstlane((int)cnt);
            before = (uint32_t)__builtin_amdgcn_readfirstlane((int)before);
        }
        below += before;
        const SelSpan nx = sel_narrow(lo, hi, bsel, (uint32_t)shift);
        lo = nx.lo; hi = nx.hi;
        // (no barrier here: the next writer of these words is the next level's search, behind that level's own two barriers)
        if constexpr (!SELF) __syncthreads();
        SEL_STAMP(2);
        SEL_COUNT_M(cnt);
        if (shift == 0) { a = lo; break; }
        if (cnt <= CAND) {
            // collect the candidates of this bucket: exactly cnt of them, the keys the histogram counted.  The threads behind them pad the
            // list with the largest key to a multiple of 64 meanwhile (the rank count walks it a wave's width at a time).
            if ((uint32_t)tid >= cnt && (uint32_t)tid < ((cnt + 63u) & ~63u)) sh.cand[tid] = SEL_PAD;
            if constexpr (!SELF) {
                if (tid == 0) { sh.s_ncand = 0; sh.s_found = 0; sh.s_a = 0; sh.s_b = 0; }
                __syncthreads();
            }
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
            if (m > CAND) m = CAND;                                  // cannot happen (m == cnt <= CAND); keeps the indices in range
            if (m <= SEL_RANK_MAX) {
                // finish by counting (sel_rank_vote), in the whole waves that hold the padded list: a wave reads 64 candidates at a time, one
                // per lane, and every lane counts how many of them lie below its own key -- the candidate comes out of the lane as a scalar
                // (v_readlane), so a lane holds its key, its count and the 64 candidates' register and nothing else
                if ((uint32_t)tid < ((m + 63u) & ~63u)) {
                    const uint32_t x = sh.cand[tid];
                    const uint32_t nch = (uint32_t)__builtin_amdgcn_readfirstlane((int)((m + 63u) >> 6));
                    uint32_t less = 0;
                    for (uint32_t ch = 0; ch < nch; ch++) {
                        const uint32_t c = sh.cand[64u * ch + ((uint32_t)tid & 63u)];
#pragma unroll
                        for (int l = 0; l < 64; l++) less += (uint32_t)((uint32_t)__builtin_amdgcn_readlane((int)c, l) < x);
                    }
                    const bool two = want2 + 1 < m;
                    const uint32_t va = wave_max_u32(sel_rank_vote(x, less, want2)), vb = wave_max_u32(sel_rank_vote(x, less, want2 + 1));
                    if (((uint32_t)tid & 63u) == 0u) {
                        atomicMax(&sh.s_a, va);
                        if (two) atomicMax(&sh.s_b, vb);
                        if (tid == 0 && two) sh.s_found = 1;
                    }
                }
            } else {
                // sort the candidates (bitonic network in LDS, padded with the largest key to a power of two >= 64): the two order
                // statistics are then read off by index.  Partners closer than 64 live in the same wave, whose LDS operations execute
                // in order, so only the wider exchanges and the start of a new merge round need a workgroup barrier.
                const uint32_t np2 = m <= 64u ? 64u : 1u << (32 - __clz(m - 1u));
                if ((uint32_t)tid >= m && (uint32_t)tid < np2) sh.cand[tid] = SEL_PAD;
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
            }
            __syncthreads();
            SEL_STAMP(4);
            a = sh.s_a;
            // (no barrier behind the reads: s_a, s_b and s_found are next written behind the barriers of a later level or selection)
            if (sh.s_found) { key_a = a; key_b = sh.s_b; if constexpr (!SELF) __syncthreads(); return; }
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
template <int NT = SEL_T, bool SELF = true, class Each>
__device__ __attribute__((always_inline)) inline float block_median_each(Each each, SelShared &sh, uint32_t n, uint32_t kmin, uint32_t kmax)
{
    const SelPlan p = sel_plan(n, -1.f, kmin, kmax);
    if (p.done) return p.result;
    uint32_t ka, kb;
    block_select2_each<NT, SELF>(each, n, p.k, sh, kmin, kmax, ka, kb);
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
