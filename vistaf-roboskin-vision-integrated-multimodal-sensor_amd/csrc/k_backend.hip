// The back end of a predict for frames whose label forest fits LDS, in ONE launch with one 1024-thread workgroup per frame: blob candidates
// -> 8-connected components -> per-component peak -> keep decision -> force tail and arg-extrema -> the caller's buffers.  These were
// k_cc_label_lds<true>, a memset of the peak plane, k_blob_peaks, k_blob_apply, k_tail and k_copy_out: five passes over the depth plane, two of
// them one-thread-per-pixel grids.  Here the labels stay in LDS between the steps and the depth plane is read twice (the second time out
// of the cache of the CU that has just read it) and written only where the filter clears a pixel.
//
// Every step is the code of the kernel it replaces: the labelling is cc_lds_build (backend_device.hpp, shared with k_cc_label_lds), the peak is
// the same wave-aggregated integer atomicMax at the component's root, the keep decision is blob_keep_threshold (shared with k_blob_apply)
// and the tail is tail_frame (shared with k_tail) with the same 1024 threads, the same pixels per thread in the same order and the same
// reductions, so every output has the bits of the separate kernels (tests/test_backend_fused.py).  The planes the contacts read-out needs
// afterwards are written as before: labels, peak_bits at the roots (other entries are never read: k_ct_roots and k_ct_rank index the
// plane by root only), kept, and the filtered depth.
#include "kernels.hpp"
#include "backend_device.hpp"

namespace vf {

__global__ __launch_bounds__(1024) void k_backend_fused(float *__restrict__ depth, const uint8_t *__restrict__ cand, const unsigned int *__restrict__ gmax_bits,
                                                        const float *__restrict__ unitless, const uint8_t *__restrict__ roi_static,
                                                        const uint8_t *__restrict__ reliable, const int32_t *__restrict__ status, double min_peak_mm,
                                                        double rel_frac, PostParams pp, int32_t *__restrict__ labels, unsigned int *__restrict__ peak_bits,
                                                        uint8_t *__restrict__ kept, double *__restrict__ scalars, int nscal, float *__restrict__ out_h,
                                                        uint8_t *__restrict__ out_r, int h, int w)
{
    extern __shared__ __attribute__((aligned(16))) uint16_t L16[];
    const size_t b = blockIdx.x;
    const int P = h * w;
    const size_t off = b * (size_t)P;
    const int lane = threadIdx.x & 63;

    // 1. labels (root = smallest pixel index of the component); the forest stays in LDS with every candidate pointing at its root
    const uint8_t *m = cc_lds_build<true>(cand + off, h, w, L16);
    unsigned int *PB = peak_bits + off;
    for (int p = threadIdx.x; p < P; p += blockDim.x) {
        int r = -1;
        if (m[p]) {
            // a walk that writes nothing on its way: the only stores of this loop are roots, so no path-halving store of another thread's
            // find can land on L16[p] after this one and leave an inner node there (a walk through p meanwhile reads its old parent or r)
            r = p;
            for (int q = ((volatile uint16_t *)L16)[r]; q != r; q = ((volatile uint16_t *)L16)[r]) r = q;
            L16[p] = (uint16_t)r;
            if (r == p) st_relaxed<__HIP_MEMORY_SCOPE_AGENT>(&PB[p], 0u);      // instead of clearing the whole plane
        }
        labels[off + p] = r;
    }
    __threadfence_block();      // one workgroup per frame: the zeros are in L2 before this CU's atomics below (as k_cc_largest)
    __syncthreads();

    // 2. per-component peak: one atomic per wave and root among its 64 consecutive pixels (wave_root_max, as k_blob_peaks)
    float *D = depth + off;
    {
        const int Pr = ((P + 63) / 64) * 64;
        for (int p = threadIdx.x; p < Pr; p += blockDim.x) {
            const int root = (p < P && m[p]) ? (int)L16[p] : -1;
            wave_root_max(root, root >= 0 ? __float_as_uint(D[p]) : 0u, PB, lane);
        }
    }
    __threadfence_block();
    __syncthreads();

    // 3. keep decision, once per component: the root's byte of the LDS mask copy becomes 2 (kept) or 1 (removed) -- still non-zero, so the
    // candidate test of every pixel stays what it was -- and a pixel's decision is two LDS reads instead of a load of its root's peak from L2
    const float thr = blob_keep_threshold(gmax_bits[b], min_peak_mm, rel_frac);
    {
        uint8_t *ml = const_cast<uint8_t *>(m);
        for (int p = threadIdx.x; p < P; p += blockDim.x) {
            if (!m[p] || (int)L16[p] != p) continue;
            const float peak = __uint_as_float(ld_relaxed<__HIP_MEMORY_SCOPE_AGENT>(&PB[p]));
            ml[p] = peak >= thr ? (uint8_t)2 : (uint8_t)1;
        }
    }
    __syncthreads();

    // 4. - 5. tail and outputs: the tail asks for each of its pixels once, in its own order; the answer is the filtered depth
    const int32_t stat = status[b];
    const bool empty = stat == 1 || stat == 3;     // k_copy_out: empty reliable mask (upstream returns None) / no carrier (pair mode)
    uint8_t *K = kept ? kept + off : nullptr;
    float *OH = out_h ? out_h + off : nullptr;
    uint8_t *OR = out_r ? out_r + off : nullptr;
    const uint8_t *REL = reliable + off;
    auto height = [&](int p) -> float {
        float d = D[p];
        bool k = false;
        if (m[p]) {
            k = m[L16[p]] == 2;
            if (!k) { d = 0.f; D[p] = 0.f; }
        }
        if (K) K[p] = (uint8_t)k;
        if (OH) OH[p] = empty ? nanf32() : d;
        if (OR) OR[p] = empty ? (uint8_t)0 : REL[p];
        return d;
    };
    tail_frame(height, (const uint8_t *)nullptr, unitless ? unitless + off : nullptr, roi_static, pp, scalars, nscal, (double *)nullptr, (int)b, P);
}

bool backend_fused_fits(int h, int w)
{
    const size_t P = (size_t)h * w;
    return P <= 65535 && cc_lds_bytes(h * w) + TAIL_STATIC_LDS <= (size_t)LDS_DYN_MAX;
}

void launch_backend_fused(float *depth, const uint8_t *cand, const unsigned int *gmax_bits, const float *unitless, const uint8_t *roi_static,
                          const uint8_t *reliable, const int32_t *status, double min_peak_mm, double rel_frac, PostParams pp, int32_t *labels,
                          unsigned int *peak_bits, uint8_t *kept, double *scalars, int nscal, float *out_h, uint8_t *out_r, int B, int h, int w,
                          hipStream_t st)
{
    static DynLdsOnce lds_once;
    ensure_dyn_lds(lds_once, (const void *)k_backend_fused, LDS_DYN_MAX - TAIL_STATIC_LDS);
    hipLaunchKernelGGL(k_backend_fused, dim3(B), dim3(1024), cc_lds_bytes(h * w), st, depth, cand, gmax_bits, unitless, roi_static, reliable, status,
                       min_peak_mm, rel_frac, pp, labels, peak_bits, kept, scalars, nscal, out_h, out_r, h, w);
}

}  // namespace vf
