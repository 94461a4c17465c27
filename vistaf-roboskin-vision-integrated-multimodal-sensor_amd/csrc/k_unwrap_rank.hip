// Ranks for the growth loop of unwrap_quality_guided (shape_ftp.py:1043-1080).
//
// k_unwrap_rank   (1024 threads / frame) replaces each masked pixel's float quality by its RANK in the
//                 frame's total order (q ascending, ties: larger pixel index first, so that the larger
//                 rank is exactly the reference heap's higher priority "-q, then smaller (y, x)").
//                 Stable LSD radix sort, 11-bit digits (3 passes), wave-contiguous chunks, 4 tiles of loads in flight.  The rank codes are
//                 written into a plane padded by one pixel of zeros on every side, next to the sorted pixel indices.
// Frames whose padded plane (h+2)*(w+2) has at most 65533 pixels get uint16 codes (k_unwrap_rank), which the batched growth loop
// k_unwrap_flood_batch (k_unwrap_batch.hip) holds in LDS; larger frames get uint32 codes (k_unwrap_rank32) for the bitmap flood of
// k_unwrap_big.hip.
#include "unwrap.hpp"
#include "select.hpp"

namespace vf {

constexpr int RK_T = 1024;

// ---- ranks -------------------------------------------------------------------------------------------
// rank plane layout: [(h+2) x (w+2)] uint16 (frame stride padded to 8 elements), border = 0.
// Sort structure: each of the 16 waves owns a contiguous range of the element array and walks it in
// 64-element tiles (coalesced, L1-bypassing loads of data other waves wrote in the previous pass).
// Counting uses a per-wave 2048-bin LDS histogram (16 x 8 KB); the stable scatter ranks a lane among the lanes of its
// tile that share its digit with eleven ballots (peer mask) + mbcnt.
// Every exchange through global memory in this kernel is between waves of ONE workgroup (one frame): workgroup scope is all the
// ordering it needs.  (Agent scope would write back and invalidate the XCD's whole L2 at every fence: buffer_wbl2 / buffer_inv sc1.)

constexpr int RK_BITS = 11, RK_NB = 1 << RK_BITS;   // 3 passes of 11 bits over the 32-bit keys
constexpr int RK_U = 4;        // 64-element tiles in flight per wave (independent loads issued together)

// CodeT = uint16_t: frames of up to 65533 padded pixels (the LDS-resident batch flood); uint32_t: larger frames (k_unwrap_big.hip), which also
// get the number of masked pixels in n_out
template <typename CodeT>
__device__ __attribute__((always_inline)) inline void unwrap_rank_body(const float *__restrict__ quality_all, const uint8_t *__restrict__ mask_all,
                                                                       unsigned long long *A_all, unsigned long long *B_all, size_t gstride,
                                                                       CodeT *__restrict__ rank_all, int32_t *__restrict__ seed_out,
                                                                       int32_t *__restrict__ n_out, int h, int w)
{
    // sort records: key << 32 | padded pixel index (one 8-byte scattered store per element and pass)
    extern __shared__ uint32_t rk_lds[];
    uint32_t (*whist)[RK_NB] = (uint32_t (*)[RK_NB])rk_lds;    // [16 waves][RK_NB digits] counts, then exclusive offsets (128 KB)
    __shared__ uint32_t wcount[16];
    const size_t b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int P = h * w, W2 = w + 2, EN = (int)padded_pixels(h, w);
    const float *q = quality_all + b * (size_t)P;
    const uint8_t *m = mask_all + b * (size_t)P;
    unsigned long long *rA = A_all + b * gstride, *rB = B_all + b * gstride;
    uint32_t *inv = (uint32_t *)rA;             // three passes leave the records in rB: rA is free for the sorted pixel indices
    CodeT *rk = rank_all + b * (size_t)code_stride(EN);
    const unsigned long long lt_mask = (1ull << lane) - 1ull;

    for (int i = tid; i < EN; i += RK_T) rk[i] = 0;
    // 1. compact masked pixels in DESCENDING pixel order; wave `wid` owns reversed positions [r0, r1)
    const int Lw = (((P + 15) / 16) + 63) & ~63;
    const int r0 = min(P, wid * Lw), r1 = min(P, r0 + Lw);
    uint32_t c = 0;
    for (int rb = r0; rb < r1; rb += 64 * RK_U) {
        uint8_t mm[RK_U];
#pragma unroll
        for (int u = 0; u < RK_U; u++) { int r = rb + u * 64 + lane; mm[u] = r < r1 ? m[P - 1 - r] : (uint8_t)0; }
#pragma unroll
        for (int u = 0; u < RK_U; u++) c += (uint32_t)__popcll(__ballot(mm[u] != 0));
    }
    if (lane == 0) wcount[wid] = c;
    __syncthreads();
    uint32_t off = 0, n = 0;
    for (int i = 0; i < 16; i++) { uint32_t x = wcount[i]; if (i < wid) off += x; n += x; }
    for (int rb = r0; rb < r1; rb += 64 * RK_U) {
        uint8_t mm[RK_U];
        float qq[RK_U];
#pragma unroll
        for (int u = 0; u < RK_U; u++) {
            int r = rb + u * 64 + lane;
            bool in = r < r1;
            mm[u] = in ? m[P - 1 - r] : (uint8_t)0;
            qq[u] = in ? q[P - 1 - r] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < RK_U; u++) {
            bool in = mm[u] != 0;
            unsigned long long bm = __ballot(in);
            if (in) {
                int p = P - 1 - (rb + u * 64 + lane);
                int y = p / w, x = p - y * w;
                uint32_t o = off + (uint32_t)__popcll(bm & lt_mask);
                rA[o] = ((unsigned long long)f2key(qq[u]) << 32) | (uint32_t)pad_index(y, x, W2);
            }
            off += (uint32_t)__popcll(bm);
        }
    }
    if (tid == 0 && n == 0) seed_out[b] = -1;
    if (tid == 0 && n_out) n_out[b] = (int32_t)n;
    __threadfence_block();
    __syncthreads();
    if (n == 0) return;

    // 2. stable LSD radix sort, 3 passes of 11 bits; wave `wid` owns elements [e0, e1)
    const int Mw = ((((int)n + 15) / 16) + 63) & ~63;
    const int e0 = min((int)n, wid * Mw), e1 = min((int)n, e0 + Mw);
    unsigned long long *rs = rA, *rd = rB;
    for (int pass = 0; pass < 3; pass++) {
        const int shift = pass * RK_BITS;
        for (int i = lane; i < RK_NB; i += 64) whist[wid][i] = 0;
        for (int eb = e0; eb < e1; eb += 64 * RK_U) {
            uint32_t kk[RK_U];
#pragma unroll
            for (int u = 0; u < RK_U; u++) { int e = eb + u * 64 + lane; kk[u] = e < e1 ? ld_relaxed<__HIP_MEMORY_SCOPE_WORKGROUP>((const uint32_t *)&rs[e] + 1) : 0u; }
#pragma unroll
            for (int u = 0; u < RK_U; u++)
                if (eb + u * 64 + lane < e1) atomicAdd(&whist[wid][(kk[u] >> shift) & (RK_NB - 1)], 1u);
        }
        __syncthreads();
        // exclusive offsets in (digit-major, wave-minor) order: thread t owns digits 2t and 2t + 1 of all 16 waves
        {
            uint32_t mine = 0;
#pragma unroll
            for (int k = 0; k < 32; k++) mine += whist[k & 15][2 * tid + (k >> 4)];
            uint32_t incl = wave_scan_add(mine);
            if (lane == 63) wcount[wid] = incl;
            __syncthreads();
            uint32_t run = incl - mine;
            for (int i = 0; i < wid; i++) run += wcount[i];
#pragma unroll
            for (int k = 0; k < 32; k++) {
                uint32_t v = whist[k & 15][2 * tid + (k >> 4)];
                whist[k & 15][2 * tid + (k >> 4)] = run;
                run += v;
            }
        }
        __syncthreads();
        for (int eb = e0; eb < e1; eb += 64 * RK_U) {
            unsigned long long rr[RK_U];
#pragma unroll
            for (int u = 0; u < RK_U; u++) {
                int e = eb + u * 64 + lane;
                rr[u] = e < e1 ? ld_relaxed<__HIP_MEMORY_SCOPE_WORKGROUP>(&rs[e]) : 0ull;
            }
#pragma unroll
            for (int u = 0; u < RK_U; u++) {
                const bool ok = eb + u * 64 + lane < e1;
                const uint32_t dgt = (uint32_t)(rr[u] >> (32 + shift)) & (RK_NB - 1);
                unsigned long long peers = __ballot(ok);
#pragma unroll
                for (int bit = 0; bit < RK_BITS; bit++) {
                    unsigned long long bm = __ballot(ok && ((dgt >> bit) & 1u));
                    peers &= ((dgt >> bit) & 1u) ? bm : ~bm;
                }
                const uint32_t base = whist[wid][dgt];
                const uint32_t rnk = (uint32_t)__popcll(peers & lt_mask);
                if (ok) rd[base + rnk] = rr[u];
                __builtin_amdgcn_wave_barrier();
                if (ok && rnk == 0) whist[wid][dgt] = base + (uint32_t)__popcll(peers);
                __builtin_amdgcn_wave_barrier();
            }
        }
        __threadfence_block();
        __syncthreads();
        unsigned long long *t = rs; rs = rd; rd = t;
    }
    // 3. rank = sorted position (ascending priority); uint16 code = rank + 3; inv[rank] = padded pixel index
    for (int e = tid; e < (int)n; e += RK_T) {
        uint32_t ix = (uint32_t)ld_relaxed<__HIP_MEMORY_SCOPE_WORKGROUP>(&rs[e]);
        rk[ix] = (CodeT)(e + 3);
        inv[e] = ix;
        if (e == (int)n - 1) seed_out[b] = (int32_t)ix;
    }
}
__global__ __launch_bounds__(RK_T) void k_unwrap_rank(const float *__restrict__ quality_all, const uint8_t *__restrict__ mask_all,
                                                      unsigned long long *A_all, unsigned long long *B_all, size_t gstride,
                                                      uint16_t *__restrict__ rank_all, int32_t *__restrict__ seed_out, int h, int w, const int32_t *__restrict__ need_frame)
{
    if (need_frame && !need_frame[blockIdx.x]) return;        // the consistency check settled this frame (k_unwrap_fast.hip)
    unwrap_rank_body<uint16_t>(quality_all, mask_all, A_all, B_all, gstride, rank_all, seed_out, nullptr, h, w);
}
__global__ __launch_bounds__(RK_T) void k_unwrap_rank32(const float *__restrict__ quality_all, const uint8_t *__restrict__ mask_all,
                                                        unsigned long long *A_all, unsigned long long *B_all, size_t gstride,
                                                        uint32_t *__restrict__ rank_all, int32_t *__restrict__ seed_out, int32_t *__restrict__ n_out,
                                                        int h, int w, const int32_t *__restrict__ need_frame)
{
    if (need_frame && !need_frame[blockIdx.x]) return;        // the consistency check settled this frame (k_unwrap_fast.hip)
    unwrap_rank_body<uint32_t>(quality_all, mask_all, A_all, B_all, gstride, rank_all, seed_out, n_out, h, w);
}
// ranks of frames too large for uint16 codes: 32-bit codes in a padded plane, sorted pixel indices in A (uint32, stride 2 * gstride)
void launch_unwrap_rank32(const float *quality, const uint8_t *mask, uint32_t *gA, uint32_t *gB, size_t gstride, uint32_t *rank32, int32_t *seed,
                          int32_t *n_out, int B, int h, int w, hipStream_t st, const int32_t *need)
{
    static DynLdsOnce rank_once;
    ensure_dyn_lds(rank_once, (const void *)k_unwrap_rank32, 16 * RK_NB * (int)sizeof(uint32_t));
    hipLaunchKernelGGL(k_unwrap_rank32, dim3(B), dim3(RK_T), (size_t)16 * RK_NB * sizeof(uint32_t), st, quality, mask, (unsigned long long *)gA,
                       (unsigned long long *)gB, gstride, rank32, seed, n_out, h, w, need);
}

// Frames of the uint16 rank range: uint16 ranks, then the batched growth loop (k_unwrap_batch.hip).  g0|g1 and g2|g3 (k_unwrap.hip:
// contiguous uint32 planes of gstride elements per frame) take the two planes of 8-byte sort records; the sorted pixel indices end up in g0
// (stride 2 * gstride), and the growth loop logs its pops in g2 (stride 2 * gstride), dead once the ranks are out, for launch_unwrap_replay.
// ppar: int32 plane of gstride elements.
void launch_unwrap_ranked(const float *quality, const uint8_t *mask, uint32_t *g0, uint32_t *g2, int32_t *ppar, size_t gstride, uint16_t *rank16,
                          int32_t *seed, int B, int h, int w, hipStream_t st, hipEvent_t ev_flood, const int32_t *need)
{
    static DynLdsOnce rank_once;
    ensure_dyn_lds(rank_once, (const void *)k_unwrap_rank, 16 * RK_NB * (int)sizeof(uint32_t));   // + 64 B static
    hipLaunchKernelGGL(k_unwrap_rank, dim3(B), dim3(RK_T), (size_t)16 * RK_NB * sizeof(uint32_t), st, quality, mask, (unsigned long long *)g0,
                       (unsigned long long *)g2, gstride, rank16, seed, h, w, need);
    if (ev_flood) hipEventRecord(ev_flood, st);
    launch_unwrap_flood_batch(rank16, seed, g0, 2 * gstride, ppar, gstride, g2, 2 * gstride, B, h, w, st, need);
}

}  // namespace vf
