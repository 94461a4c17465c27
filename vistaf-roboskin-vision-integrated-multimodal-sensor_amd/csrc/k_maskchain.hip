// The three binary-mask chains of a predict, each in ONE launch with one 1024-thread workgroup per frame, for frames whose bit planes (and,
// for the reliable mask, label forest) fit LDS: mask_chain_fits of mask_bits.hpp, Tiers::fused_masks.  A mask is 64-bit words in LDS from the
// first threshold to the last count; only the planes a later stage or a test reads are written, as bytes.
//
//   k_bad_chain       bad = valid & (img >= hi | grad >= g) -> n dilations -> bad1, bad_count                  (shape_ftp.py:638-646)
//       was k_bad_flags, k_morph_bits per dilation, a memset and k_count_u8; bad0 is not written.
//   k_reliable_chain  rel0 = roi & finite & (q >= thr) -> close -> & roi -> largest 8-connected component -> & roi -> erosion by the
//                     chamfer ball -> reliable, rel_count, status 1 where it is empty                             (shape_ftp.py:739-775)
//       was k_threshold_mask, k_morph_bits, k_cc_label_lds, k_cc_largest, k_morph_bits, a memset, k_count_u8 and k_mark_empty; rel1, rel2 and
//       the label plane are not written, the area plane only at the roots.
//   k_contact_chain   count at the first threshold -> threshold choice -> contact -> n dilations -> & reliable -> contact_d;
//                     background = reliable & ~contact_d, or reliable below 15 % of it                          (shape_ftp.py:1719-1741)
//       was a memset, k_contact_count, k_contact_mask, k_morph_bits, k_and_not, a memset, k_count_u8 and k_background_fix; the contact plane
//       before the dilation is not written.
//
// Every step is the code of the kernel it replaces.  The pixel rules (bad_flag_px, quality_mask_px, contact_px, contact_first_thr,
// contact_used_thr, background_falls_back, marks_empty) are the ones k_bad_flags, k_threshold_mask, k_contact_count, k_contact_mask,
// k_background_fix and k_mark_empty call (pixel_ops.hpp).  Pack, dilate / erode and unpack are k_morph_bits' own steps (mb_pack,
// mb_morph_step, mb_unpack of mask_bits.hpp).  The labelling is cc_lds_forest (backend_device.hpp, the forest of k_cc_label_lds and
// k_backend_fused) reading the bit plane through BitMask; cc16_settle (the walk of k_backend_fused's first step) and the roots-only clear
// follow k_backend_fused.  The areas are
// k_cc_largest's: ccl_run_count over the same 64-pixel tiles in the same order, the same ccl_key / ccl_root choice, the same
// workgroup-scope ordering (one workgroup per frame: a __threadfence_block() between the clear, the atomics and the reads).  Counts are
// popcounts of the plane that is unpacked, so they are the byte counts k_count_u8 took.  tests/test_mask_chains.py pins each chain against
// the separate kernels and against a CPU reference.
#include "kernels.hpp"
#include "backend_device.hpp"
#include "mask_bits.hpp"

namespace vf {

__global__ __launch_bounds__(MB_T) void k_bad_chain(const float *__restrict__ img, const float *__restrict__ grad, const uint8_t *__restrict__ valid,
                                                    const float *__restrict__ thr_hi, const float *__restrict__ thr_g, MorphSeq seq,
                                                    uint8_t *__restrict__ bad1, int *__restrict__ bad_count, int h, int w)
{
    extern __shared__ unsigned long long mc_lds[];
    __shared__ int cnt[16];
    const int W64 = mb_w64(w), nw = h * W64;
    unsigned long long *A = mc_lds, *O = mc_lds + nw;
    const size_t b = blockIdx.x, off = b * (size_t)h * w;
    const float *I = img + off, *G = grad + off;
    const float hi = thr_hi[b], g = thr_g[b];
    mb_pack(A, h, w, [=](int y, int x) { const size_t p = (size_t)y * w + x; return (uint8_t)bad_flag_px(valid[p], I[p], G[p], hi, g); });
    __syncthreads();
    const unsigned long long last_valid = mb_last_valid(w);
    for (int op = 0; op < seq.n; op++) mb_morph_step(A, O, h, W64, seq.se[op], seq.dilate[op] != 0, last_valid);
    mb_unpack(A, bad1 + off, h, w, nullptr, nullptr);
    const int c = mb_count(A, nw, cnt);
    if (threadIdx.x == 0) bad_count[b] = c;
}

__global__ __launch_bounds__(MB_T) void k_reliable_chain(const float *__restrict__ quality, const uint8_t *__restrict__ roi, const float *__restrict__ amp_thr,
                                                         MorphSeq seq, RowSpanSE ball, int has_ball, int32_t *__restrict__ area,
                                                         uint8_t *__restrict__ rel0, uint8_t *__restrict__ reliable, int *__restrict__ rel_count,
                                                         int32_t *__restrict__ status, int h, int w)
{
    extern __shared__ __attribute__((aligned(16))) uint16_t mc_l16[];      // the forest, and behind it three bit planes
    __shared__ unsigned long long s64[16];
    __shared__ int cnt[16];
    const int P = h * w, W64 = mb_w64(w), nw = h * W64;
    uint16_t *L16 = mc_l16;
    unsigned long long *A = (unsigned long long *)((char *)mc_l16 + cc_lds_forest_bytes(P)), *O = A + nw, *R = O + nw;
    const size_t b = blockIdx.x, off = b * (size_t)P;
    const int tid = threadIdx.x, lane = tid & 63;
    const unsigned long long last_valid = mb_last_valid(w);

    // 1. threshold (k_threshold_mask); the static roi as a plane, for the two ANDs below
    const float *Q = quality + off;
    const float thr = amp_thr[b];
    mb_pack(A, h, w, [=](int y, int x) { const size_t p = (size_t)y * w + x; return (uint8_t)quality_mask_px(roi[p], Q[p], thr); });
    mb_pack(R, h, w, [=](int y, int x) { return roi[(size_t)y * w + x]; });
    __syncthreads();
    mb_unpack(A, rel0 + off, h, w, nullptr, nullptr);
    __syncthreads();            // A is changed in place from here on

    // 2. closing, then & roi (k_morph_bits with and_static)
    for (int op = 0; op < seq.n; op++) mb_morph_step(A, O, h, W64, seq.se[op], seq.dilate[op] != 0, last_valid);
    for (int t = tid; t < nw; t += MB_T) A[t] &= R[t];
    __syncthreads();

    // 3. labels (k_cc_label_lds): every mask pixel ends up pointing at its root, and the area plane is cleared at the roots only
    const BitMask m(A, w);
    cc_lds_forest(m, h, w, L16);
    int32_t *AR = area + off;
    for (int p = tid; p < P; p += MB_T) {
        if (!m[p]) continue;
        if (cc16_settle(L16, p) == p) st_relaxed<__HIP_MEMORY_SCOPE_AGENT>(&AR[p], 0);
    }
    __threadfence_block();      // one workgroup per frame: the zeros are in L2 before this CU's atomics below (as k_cc_largest)
    __syncthreads();

    // 4. areas per root, the largest root, its plane & roi (k_cc_largest).  Off the mask the forest holds 0xffff, which no root equals.
    constexpr int U = 4;
    {
        const int Pr = ((P + U * MB_T - 1) / (U * MB_T)) * (U * MB_T);
        int run_root = -1, run_cnt = 0;
        for (int p0 = tid; p0 < Pr; p0 += U * MB_T) {
            int root[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int p = p0 + u * MB_T;
                const int l = p < P ? (int)L16[p] : 0xffff;
                root[u] = l == 0xffff ? -1 : l;
            }
#pragma unroll
            for (int u = 0; u < U; u++) ccl_run_count(root[u], run_root, run_cnt, AR, lane);
        }
        ccl_run_flush(run_root, run_cnt, AR, lane);
    }
    __threadfence_block();
    __syncthreads();
    unsigned long long best = 0;
    for (int p = tid; p < P; p += MB_T) {
        if ((int)L16[p] != p) continue;
        const unsigned long long key = ccl_key(ld_relaxed<__HIP_MEMORY_SCOPE_AGENT>(&AR[p]), p);
        if (key > best) best = key;
    }
    best = block_max_u64(best, s64);
    const int broot = ccl_root(best);
    mb_pack(O, h, w, [=](int y, int x) { return (uint8_t)((int)L16[y * w + x] == broot); });
    __syncthreads();
    for (int t = tid; t < nw; t += MB_T) O[t] &= R[t];
    __syncthreads();
    { unsigned long long *tmp = A; A = O; O = tmp; }

    // 5. erosion by the chamfer ball (k_morph_bits), the byte plane, its count (k_count_u8) and the empty-mask status (k_mark_empty)
    if (has_ball) mb_morph_step(A, O, h, W64, ball, false, last_valid);
    mb_unpack(A, reliable + off, h, w, nullptr, nullptr);
    const int c = mb_count(A, nw, cnt);
    if (tid == 0) {
        rel_count[b] = c;
        if (marks_empty(c, status[b])) status[b] = 1;
    }
}

__global__ __launch_bounds__(MB_T) void k_contact_chain(const float *__restrict__ res, const uint8_t *__restrict__ reliable, const float *__restrict__ thr3,
                                                        const int *__restrict__ rel_count, double min_frac, double max_frac, MorphSeq seq,
                                                        int *__restrict__ contact_count, float *__restrict__ thr_used, uint8_t *__restrict__ contact_d,
                                                        uint8_t *__restrict__ background, int *__restrict__ bg_count, int h, int w)
{
    extern __shared__ unsigned long long mc_lds[];
    __shared__ int cnt[16];
    const int P = h * w, W64 = mb_w64(w), nw = h * W64;
    unsigned long long *A = mc_lds, *O = A + nw, *R = O + nw;
    const size_t b = blockIdx.x, off = b * (size_t)P;
    const int tid = threadIdx.x;
    const float *RES = res + off;
    const uint8_t *REL = reliable + off;
    const float *t3 = thr3 + b * 3;

    // 1. count at the first threshold (k_contact_count): the popcount of the contact plane at that threshold
    const float thr1 = contact_first_thr(t3);
    mb_pack(R, h, w, [=](int y, int x) { return REL[(size_t)y * w + x]; });
    mb_pack(A, h, w, [=](int y, int x) { const size_t p = (size_t)y * w + x; return (uint8_t)contact_px(REL[p], RES[p], thr1); });
    __syncthreads();
    const int cc = mb_count(A, nw, cnt);
    const int rc = rel_count[b];

    // 2. the threshold the mask is formed with (k_contact_mask).  Unchanged (the same bits): A is that mask already; else the residuals are
    // read again, out of the cache of the CU that has just read them
    const float thr = contact_used_thr(t3, cc, rc, min_frac, max_frac);
    if (tid == 0) { contact_count[b] = cc; thr_used[b] = thr; }
    if (__float_as_uint(thr) != __float_as_uint(thr1)) {
        mb_pack(A, h, w, [=](int y, int x) { const size_t p = (size_t)y * w + x; return (uint8_t)contact_px(REL[p], RES[p], thr); });
        __syncthreads();
    }

    // 3. dilations, then & reliable (k_morph_bits with and_frame)
    const unsigned long long last_valid = mb_last_valid(w);
    for (int op = 0; op < seq.n; op++) mb_morph_step(A, O, h, W64, seq.se[op], seq.dilate[op] != 0, last_valid);
    for (int t = tid; t < nw; t += MB_T) { const unsigned long long v = A[t] & R[t]; A[t] = v; O[t] = R[t] & ~v; }      // O: k_and_not
    __syncthreads();
    mb_unpack(A, contact_d + off, h, w, nullptr, nullptr);

    // 4. background: its count (k_count_u8), and the reliable plane itself where the count is below 15 % of it (k_background_fix)
    const int bg = mb_count(O, nw, cnt);
    if (tid == 0) bg_count[b] = bg;
    if (background_falls_back(bg, rc)) {
        for (int p = tid; p < P; p += MB_T) background[off + p] = REL[p];
    } else mb_unpack(O, background + off, h, w, nullptr, nullptr);
}

namespace {
MorphSeq morph_seq_of(const RowSpanSE &se, int ndil, int nero)
{
    MorphSeq seq;
    seq.n = ndil + nero;
    for (int i = 0; i < MB_MAXOPS; i++) { seq.dilate[i] = i < ndil ? 1 : 0; seq.se[i] = se; }
    return seq;
}
}  // namespace

void launch_bad_chain(const float *img, const float *grad, const uint8_t *valid, const float *thr_hi, const float *thr_g, const RowSpanSE &se,
                      int iters, uint8_t *bad1, int *bad_count, int B, int h, int w, hipStream_t st)
{
    static DynLdsOnce lds_once;
    ensure_dyn_lds(lds_once, (const void *)k_bad_chain, LDS_DYN_HEADROOM);      // what mask_chain_fits admits; the kernel's static LDS comes on top
    hipLaunchKernelGGL(k_bad_chain, dim3(B), dim3(MB_T), mask_chain_lds(MCH_BAD, h, w), st, img, grad, valid, thr_hi, thr_g,
                       morph_seq_of(se, iters, 0), bad1, bad_count, h, w);
}

void launch_reliable_chain(const float *quality, const uint8_t *roi, const float *amp_thr, const RowSpanSE &se_close, int close_iters,
                           const RowSpanSE *ball, int32_t *area, uint8_t *rel0, uint8_t *reliable, int *rel_count, int32_t *status, int B, int h,
                           int w, hipStream_t st)
{
    static DynLdsOnce lds_once;
    ensure_dyn_lds(lds_once, (const void *)k_reliable_chain, LDS_DYN_HEADROOM);      // what mask_chain_fits admits; the kernel's static LDS comes on top
    hipLaunchKernelGGL(k_reliable_chain, dim3(B), dim3(MB_T), mask_chain_lds(MCH_RELIABLE, h, w), st, quality, roi, amp_thr,
                       morph_seq_of(se_close, close_iters, close_iters), ball ? *ball : se_close, ball ? 1 : 0, area, rel0, reliable, rel_count,
                       status, h, w);
}

void launch_contact_chain(const float *res, const uint8_t *reliable, const float *thr3, const int *rel_count, double min_frac, double max_frac,
                          const RowSpanSE &se, int iters, int *contact_count, float *thr_used, uint8_t *contact_d, uint8_t *background,
                          int *bg_count, int B, int h, int w, hipStream_t st)
{
    static DynLdsOnce lds_once;
    ensure_dyn_lds(lds_once, (const void *)k_contact_chain, LDS_DYN_HEADROOM);      // what mask_chain_fits admits; the kernel's static LDS comes on top
    hipLaunchKernelGGL(k_contact_chain, dim3(B), dim3(MB_T), mask_chain_lds(MCH_CONTACT, h, w), st, res, reliable, thr3, rel_count, min_frac,
                       max_frac, morph_seq_of(se, iters < 0 ? 0 : iters, 0), contact_count, thr_used, contact_d, background, bg_count, h, w);
}

}  // namespace vf
