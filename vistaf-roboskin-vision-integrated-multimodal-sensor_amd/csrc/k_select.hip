// Per-frame exact percentiles / medians (np.percentile, np.nanpercentile, np.nanmedian call sites:
// shape_ftp.py:347, :354, :622, :846, :1720-1732, :1746, :1760, :1764).  One 1024-thread workgroup
// per frame; see select.hpp for the algorithm.
//
// Two kernels.  k_select_resident<NS> (planes of up to 65536 pixels) loads every element once, keeps its key in one of NS registers per
// thread and runs every sweep of the selection over those registers; k_select (larger planes) streams the plane from memory on every sweep.
#include "kernels.hpp"
#include "select.hpp"

namespace vf {

struct PlaneGetter {
    const float *v; const uint8_t *m; float le; bool use_le, use_abs;
    __device__ bool operator()(int i, uint32_t &key) const
    {
        // both loads unconditional, so that the SEL_U elements of a batch are all in flight together (select.hpp: sel_foreach)
        const uint8_t mk = m[i];
        const float x = v[i];
        return sel_element(mk, x, use_abs, use_le ? &le : nullptr, key);
    }
};

__global__ __launch_bounds__(SEL_T) void k_select(const float *__restrict__ vals, const uint8_t *__restrict__ mask, size_t mask_stride,
                                                  const float *__restrict__ le_thr, int use_abs, const float *__restrict__ reqs,
                                                  int nreq, float *__restrict__ out, int *__restrict__ counts, int P)
{
    __shared__ SelShared sh;
    size_t b = blockIdx.x;
    PlaneGetter g{vals + b * (size_t)P, mask + b * mask_stride, le_thr ? le_thr[b] : 0.f, le_thr != nullptr, use_abs != 0};
    uint32_t n, kmin, kmax;
    sel_init(sh);                                  // block_minmax's barriers stand between this and the first sweep
    block_minmax(g, P, sh, n, kmin, kmax);
    if (threadIdx.x == 0 && counts) counts[b] = (int)n;
    for (int j = 0; j < nreq; j++) {
        float q = reqs[j];
        float r = (q < 0.f) ? block_median(g, P, sh, n, kmin, kmax) : block_percentile(g, P, q, sh, n, kmin, kmax);
        if (threadIdx.x == 0) out[b * (size_t)nreq + j] = r;
        __syncthreads();
    }
}

// ---- the register-resident kernel ---------------------------------------------------------------------------------------------------
// Thread t owns elements t, t + 1024, ... of the plane: slot s holds the key of element t + 1024 s, or SEL_NOKEY where the element is
// invalid (masked out, not finite, above the threshold) or lies beyond the plane.  No finite float has that key (it is f2key of the NaN
// 0x7fffffff), and it is the largest key, so every "key <= bound" test of a sweep drops it without a test of its own.
constexpr uint32_t SEL_NOKEY = 0xFFFFFFFFu;
constexpr int SEL_MAX_CHAIN = 4;
// where the results go: plain, request j of frame b at p[0][b * nreq + j]; chained, at p[j][b]
struct SelOut { float *p[SEL_MAX_CHAIN]; };

// count / min / max of this thread's keys <= cut, reduced over the workgroup: SelRange's rule (select.hpp) in this kernel's own spelling, on
// 32-bit keys with SEL_NOKEY as "none" inside the NS-times unrolled loop; the 64-bit accumulator there would change the kernel's text
template <int NS>
__device__ inline void resident_minmax(const uint32_t (&key)[NS], uint32_t cut, SelShared &sh, uint32_t &n, uint32_t &kmin, uint32_t &kmax)
{
    uint32_t c = 0, mn = SEL_NOKEY, mx = 0;
#pragma unroll
    for (int s = 0; s < NS; s++)
        if (key[s] <= cut) { c++; mn = key[s] < mn ? key[s] : mn; mx = key[s] > mx ? key[s] : mx; }
    __syncthreads();
    n = block_sum<uint32_t>(c, sh.wsum);
    kmin = (uint32_t)block_min_u64(mn, sh.red64);
    kmax = (uint32_t)block_max_u64(mx, sh.red64);
    __syncthreads();
}

// chained != 0: request j > 0 runs over the elements that also satisfy x <= result[j - 1], compared as floats as PlaneGetter does
// (a NaN result leaves no element; -0.0 <= 0.0 holds although the key of -0.0 is the smaller one)
template <int NS>
__global__ __launch_bounds__(SEL_T) void k_select_resident(const float *__restrict__ vals, const uint8_t *__restrict__ mask, size_t mask_stride,
                                                           const float *__restrict__ le_thr, int use_abs, const float *__restrict__ reqs,
                                                           int nreq, int chained, SelOut out, int *__restrict__ counts, int P)
{
    __shared__ SelShared sh;
    const size_t b = blockIdx.x;
    const PlaneGetter g{vals + b * (size_t)P, mask + b * mask_stride, le_thr ? le_thr[b] : 0.f, le_thr != nullptr, use_abs != 0};
    uint32_t key[NS];
    // the one pass over memory: SEL_U elements per thread in flight together; a slot beyond the plane reads the last element and drops it
#pragma unroll
    for (int s0 = 0; s0 < NS; s0 += SEL_U) {
        bool ok[SEL_U];
#pragma unroll
        for (int u = 0; u < SEL_U; u++)
            if (s0 + u < NS) {
                const int i = (int)threadIdx.x + (s0 + u) * SEL_T;
                ok[u] = g(i < P ? i : P - 1, key[s0 + u]) && i < P;
            }
#pragma unroll
        for (int u = 0; u < SEL_U; u++)
            if (s0 + u < NS && !ok[u]) key[s0 + u] = SEL_NOKEY;
    }
    uint32_t cut = SEL_NOKEY - 1u;              // every valid key
    // Every sweep works on opaque copies of the keys.  Whatever a sweep derives from key[s] alone is invariant across the sweeps of a launch,
    // and the compiler hoists it and keeps it live next to the keys: the NS answers of "key[s] <= cut" as exec masks in SGPRs, the 64-bit
    // extension of every key that block_select2_each's last sweep compares (a second VGPR per slot) -- hundreds of spills (k_fit.hip: each)
    const auto each = [&](auto body) {
#pragma unroll
        for (int s = 0; s < NS; s++) {
            uint32_t k = key[s];
            asm volatile("" : "+v"(k));
            if (k <= cut) body(k);
        }
    };
    uint32_t n, kmin, kmax;
    sel_init(sh);                                  // resident_minmax's barriers stand between this and the first sweep
    resident_minmax<NS>(key, cut, sh, n, kmin, kmax);
    if (threadIdx.x == 0 && counts) counts[b] = (int)n;
    float r = 0.f;
    for (int j = 0; j < nreq; j++) {
        if (chained && j > 0 && n > 0) {
            if (r != r) n = 0;
            else {
                const uint32_t c2 = f2key(r == 0.f ? 0.f : r);
                cut = c2 < cut ? c2 : cut;
                resident_minmax<NS>(key, cut, sh, n, kmin, kmax);
            }
        }
        // one block_select2_each for every kind of request (it is inlined, and its sweeps are unrolled NS times: a copy per kind, as
        // block_median_each next to block_percentile would make, doubles the kernel's code)
        const SelPlan p = sel_plan(n, reqs[j], kmin, kmax);
        if (p.done) r = p.result;
        else {
            uint32_t ka, kb;
            block_select2_each<SEL_T>(each, n, p.k, sh, kmin, kmax, ka, kb);
            r = sel_result(p, ka, kb);
        }
        if (threadIdx.x == 0) {
            if (chained) (j == 0 ? out.p[0] : j == 1 ? out.p[1] : j == 2 ? out.p[2] : out.p[3])[b] = r;      // no runtime index into the argument
            else out.p[0][b * (size_t)nreq + j] = r;
        }
        __syncthreads();
    }
}

int select_variant(int B, int P, int nreq, bool big, bool resident)
{
    if (big && nreq <= 4 && big_frames(B, P)) return SELV_BIG;
    if (!resident || P > 64 * SEL_T) return SELV_STREAM;
    return P <= 16 * SEL_T ? SELV_RES16 : P <= 32 * SEL_T ? SELV_RES32 : P <= 49 * SEL_T ? SELV_RES49 : SELV_RES64;
}

static void launch_resident(int variant, const float *vals, const uint8_t *mask, size_t mask_stride, const float *le_thr, bool use_abs,
                            const float *reqs_dev, int nreq, bool chained, const SelOut &out, int *counts, int B, int P, hipStream_t st)
{
#define VF_SEL_RES(NS) hipLaunchKernelGGL(k_select_resident<NS>, dim3(B), dim3(SEL_T), 0, st, vals, mask, mask_stride, le_thr, use_abs ? 1 : 0, \
                                          reqs_dev, nreq, chained ? 1 : 0, out, counts, P)
    switch (variant) {
    case SELV_RES16: VF_SEL_RES(16); break;
    case SELV_RES32: VF_SEL_RES(32); break;
    case SELV_RES49: VF_SEL_RES(49); break;
    default: VF_SEL_RES(64); break;
    }
#undef VF_SEL_RES
}

void launch_select(const float *vals, const uint8_t *mask, size_t mask_stride, const float *le_thr, bool use_abs,
                   const float *reqs_dev, int nreq, float *out, int *counts, int B, int P, hipStream_t st, void *big_scratch, bool resident)
{
    const int variant = select_variant(B, P, nreq, big_scratch != nullptr, resident);
    if (variant == SELV_BIG)                                     // large frames: every sweep over all pixels of the batch (k_big.hip)
        launch_select_big(vals, mask, mask_stride, le_thr, use_abs, reqs_dev, nreq, out, counts, B, P, big_scratch, st);
    else if (variant == SELV_STREAM)
        hipLaunchKernelGGL(k_select, dim3(B), dim3(SEL_T), 0, st, vals, mask, mask_stride, le_thr, use_abs ? 1 : 0, reqs_dev, nreq,
                           out, counts, P);
    else launch_resident(variant, vals, mask, mask_stride, le_thr, use_abs, reqs_dev, nreq, false, SelOut{{out}}, counts, B, P, st);
}

int launch_select_chained(const float *vals, const uint8_t *mask, size_t mask_stride, bool use_abs, const float *reqs_dev, int nreq,
                          float *const *outs, int *counts, int B, int P, hipStream_t st)
{
    const int variant = select_variant(B, P, nreq, false, true);
    if (variant < SELV_RES16 || nreq < 1 || nreq > SEL_MAX_CHAIN) return -1;
    SelOut o{};
    for (int j = 0; j < nreq; j++) o.p[j] = outs[j];
    launch_resident(variant, vals, mask, mask_stride, nullptr, use_abs, reqs_dev, nreq, true, o, counts, B, P, st);
    return variant;
}

}  // namespace vf
