// unwrap_quality_guided on the GPU (shape_ftp.py:1043-1080).
//
// The reference grows a region from the best-quality pixel with a max-heap of tuples
// (-q, y, x, py, px).  That is Prim-style growth with a total order: the next pixel is the frontier
// pixel with the largest (q, then smallest (y, x)), and its parent is the lexicographically smallest
// (py, px) among its neighbours visited so far.  The growth order is inherently sequential; launch_unwrap picks the flood by the
// size of the padded frame, EN = (h+2)*(w+2):
//   EN <= 65533      uint16 ranks and the batched flood in LDS (k_unwrap_rank.hip, k_unwrap_batch.hip), whose pop log
//                    k_unwrap_replay turns into wrap counts;
//   EN < 2^26        32-bit ranks and the bitmap flood (k_unwrap_big.hip); the frames whose mask outgrows its bitmap go to
//                    k_unwrap_flood, then every frame to k_unwrap_tree;
//   larger           k_unwrap_flood, then k_unwrap_tree.
// The last two kernels live here:
//   k_unwrap_flood  one wavefront per frame replays exactly that order (frontier keys and pixel states in global memory,
//                   64-lane arg-max per step, the 8 neighbours examined by 8 lanes) and records only the spanning tree
//                   (parent index per pixel);
//   k_unwrap_tree   (parallel) turns the tree into integer wrap counts by pointer jumping (integer sums are associative,
//                   so any evaluation order gives the tree's exact counts) and writes u = w + 2*pi*k.
// In exact arithmetic u[p] - w[p] is the same multiple of 2*pi as in the reference's
// u[p] = u[parent] + angle(exp(1j*(w[p]-w[parent]))) chain; only float32 rounding along the chain differs.
#include "unwrap.hpp"

namespace vf {

// fq / fi / st: the frontier keys and indices (cap entries per frame) and the pixel states, in global memory
__global__ __launch_bounds__(64) void k_unwrap_flood(const float *__restrict__ quality_all, const uint8_t *__restrict__ mask_all,
                                                     int32_t *__restrict__ parent_all, uint8_t *gst, uint32_t *gfq, uint32_t *gfi,
                                                     int cap, int32_t *status, int h, int w, const int32_t *__restrict__ only, const int32_t *__restrict__ need_frame)
{
    if (need_frame && !need_frame[blockIdx.x]) return;        // the consistency check settled this frame (k_unwrap_fast.hip)
    const int lane = threadIdx.x;
    const size_t b = blockIdx.x;
    if (only && !only[b]) return;                    // big-frame path: only the frames the bitmap flood handed back
    const int P = h * w;
    const float *quality = quality_all + b * (size_t)P;
    const uint8_t *mask = mask_all + b * (size_t)P;
    int32_t *parent = parent_all + b * (size_t)P;
    uint32_t *fq = gfq + b * (size_t)cap, *fi = gfi + b * (size_t)cap;
    uint8_t *st = gst + b * (size_t)P;

    // st: 0 untouched, 1 in frontier, 2 visited.  Seed = first arg-max of q over the mask.
    unsigned long long best = 0;
    for (int p = lane; p < P; p += 64) {
        st[p] = 0;
        parent[p] = -1;
        if (mask[p]) {
            unsigned long long k = argmax_key(quality[p], (unsigned)p);
            if (k > best) best = k;
        }
    }
    best = wave_max_u64(best);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __syncthreads();
    if (best == 0) return;   // empty mask: everything stays NaN (shape_ftp.py:1047-1048)
    int F = 0;
    bool overflow = false;
    int cur = (int)(0xffffffffu - (uint32_t)(best & 0xffffffffu));
    bool is_seed = true;

    for (;;) {
        // ---- visit `cur`: parent = lexicographically smallest visited neighbour; push new neighbours
        int y = cur / w, x = cur - y * w;
        int np = -1;
        uint8_t s = 255;
        if (lane < 8) {
            int dy, dx;
            neighbour_slot(lane, dy, dx);
            int ny = y + dy, nx = x + dx;
            if (ny >= 0 && ny < h && nx >= 0 && nx < w) { np = ny * w + nx; s = ld_relaxed<__HIP_MEMORY_SCOPE_AGENT>(st + np); }
        }
        unsigned long long vis = __ballot(s == 2);
        int par = cur;
        if (!is_seed) {
            int pl = __ffsll((long long)vis) - 1;      // always >= 0: cur entered the frontier from a visited pixel
            par = __shfl(np, pl, 64);
        }
        bool fresh = (s == 0) && mask[np < 0 ? 0 : np] && np >= 0;
        uint32_t nk = fresh ? f2key(quality[np]) : 0u;
        unsigned long long nb = __ballot(fresh);
        int cnt = (int)__popcll(nb);
        if (F + cnt > cap) { overflow = true; break; }
        if (fresh) {
            int pos = F + (int)__popcll(nb & ((1ull << lane) - 1ull));
            fq[pos] = nk;
            fi[pos] = (uint32_t)np;
            st[np] = 1;
        }
        if (lane == 0) { parent[cur] = par; st[cur] = 2; }
        F += cnt;
        is_seed = false;
        if (F == 0) break;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");

        // ---- pop the frontier maximum: (q desc, index asc)
        uint32_t bq = 0, bi = 0xffffffffu;
        int bslot = -1;
        for (int j = lane; j < F; j += 64) {
            uint32_t kq = fq[j], ki = fi[j];
            if (kq > bq || (kq == bq && ki < bi)) { bq = kq; bi = ki; bslot = j; }
        }
        uint32_t mq = wave_max_u32(bq);
        unsigned long long tie = __ballot(bq == mq && bslot >= 0);
        int leader;
        if (__popcll(tie) == 1) leader = __ffsll((long long)tie) - 1;
        else {
            uint32_t mi = ~wave_max_u32((bq == mq && bslot >= 0) ? ~bi : 0u);
            unsigned long long who = __ballot(bq == mq && bslot >= 0 && bi == mi);
            leader = __ffsll((long long)who) - 1;
        }
        int slot = __shfl(bslot, leader, 64);
        cur = (int)__shfl(bi, leader, 64);
        int last = F - 1;
        if (lane == 0 && slot != last) { fq[slot] = fq[last]; fi[slot] = fi[last]; }
        F = last;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    }
    if (overflow && lane == 0) status[b] = 2;
}

// Tree -> wrap counts -> unwrapped phase, one 1024-thread workgroup per frame.
// Each pixel carries one 64-bit word (parent index | wrap-count increment relative to that parent), where
// inc = the integer n with (w[p]-w[par]) + 2*pi*n in (-pi, pi].  Pointer jumping replaces
// (par, inc) by (par[par], inc + inc[par]) IN PLACE and asynchronously: every word always states a true
// relation "k[p] = k[par] + inc" (the k are fixed by the tree), and a parent's word is read with one 64-bit
// load, so any interleaving is consistent; rounds repeat until every pixel points at the seed.
// ppar_all (optional): parents in PADDED (h+2)x(w+2) index space as written by the bitmap flood (k_unwrap_big.hip);
// they are converted here and stored to parent_all (the plane the parity tests read back).
__global__ __launch_bounds__(1024) void k_unwrap_tree(const float *__restrict__ wrapped_all, int32_t *parent_all,
                                                      const int32_t *__restrict__ ppar_in, size_t gstride, unsigned long long *words_all,
                                                      float *__restrict__ unwrapped_all, int h, int w, const int32_t *__restrict__ plain_parents, const int32_t *__restrict__ need_frame)
{
    if (need_frame && !need_frame[blockIdx.x]) return;        // the consistency check settled this frame (k_unwrap_fast.hip)
    __shared__ int s_changed;
    const size_t b = blockIdx.x;
    // plain_parents[b] != 0: this frame's parents were written to parent_all directly (generic flood), not to the padded plane
    const int32_t *ppar_all = (plain_parents && plain_parents[b]) ? nullptr : ppar_in;
    const int P = h * w;
    const float *wrapped = wrapped_all + b * (size_t)P;
    int32_t *tree = parent_all + b * (size_t)P;
    unsigned long long *word = words_all + b * gstride;
    for (int p = threadIdx.x; p < P; p += blockDim.x) {
        int par;
        if (ppar_all) {
            const int W2 = w + 2;
            int y = p / w, x = p - y * w;
            int pp = ppar_all[b * gstride + (size_t)pad_index(y, x, W2)];
            par = pp < 0 ? -1 : unpad_index(pp, 0u, W2);
            tree[p] = par;
        } else par = tree[p];
        int v = 0;
        if (par >= 0 && par != p) v = wrap_count((double)wrapped[p] - (double)wrapped[par]);
        word[p] = (unsigned long long)(uint32_t)par | ((unsigned long long)(uint32_t)v << 32);
    }
    __threadfence();
    __syncthreads();
    for (int round = 0; round < 64; round++) {
        if (threadIdx.x == 0) s_changed = 0;
        __syncthreads();
        int changed = 0;
        for (int p0 = threadIdx.x; p0 < P; p0 += 4 * blockDim.x) {
            unsigned long long wv[4], wq[4];
            int pp[4];
#pragma unroll
            for (int u = 0; u < 4; u++) { pp[u] = p0 + u * blockDim.x; wv[u] = pp[u] < P ? ld_relaxed<__HIP_MEMORY_SCOPE_AGENT>(word + pp[u]) : ~0ull; }
#pragma unroll
            for (int u = 0; u < 4; u++) { int par = (int)(uint32_t)wv[u]; wq[u] = (par >= 0 && par != pp[u]) ? ld_relaxed<__HIP_MEMORY_SCOPE_AGENT>(word + par) : ~0ull; }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                int par = (int)(uint32_t)wv[u];
                if (par < 0 || par == pp[u]) continue;
                int pq = (int)(uint32_t)wq[u];
                if (pq != par && pq >= 0) {
                    int v = (int)(uint32_t)(wv[u] >> 32) + (int)(uint32_t)(wq[u] >> 32);
                    st_relaxed<__HIP_MEMORY_SCOPE_AGENT>(word + pp[u], (unsigned long long)(uint32_t)pq | ((unsigned long long)(uint32_t)v << 32));
                    changed = 1;
                }
            }
        }
        if (changed) s_changed = 1;
        __threadfence();
        __syncthreads();
        int any = s_changed;
        __syncthreads();
        if (!any) break;
    }
    float *unwrapped = unwrapped_all + b * (size_t)P;
    for (int p = threadIdx.x; p < P; p += blockDim.x) {
        unsigned long long wv = ld_relaxed<__HIP_MEMORY_SCOPE_AGENT>(word + p);
        unwrapped[p] = (int)(uint32_t)wv >= 0 ? unwrap_value(wrapped[p], (int)(uint32_t)(wv >> 32)) : nanf32();
    }
}

// The flood's planes, then the check's.  EN = (h + 2)(w + 2) is the per-frame stride of the uint32 planes; sort_a and sort_b are two of them
// each (2 EN per frame), and what they hold changes along a path:
struct UnwrapScratch {
    uint8_t *state;                     // [B, P] pixel states of the generic flood
    uint32_t *sort_a, *sort_b;          // [B, 2 EN] the rank kernels' 8-byte sort records; sort_a then holds the sorted pixel indices (stride 2 EN)
    int32_t *ppar;                      // [B, EN] parents in padded index space (batched and bitmap floods)
    void *rank;                         // [B, code_stride(EN)] rank codes: uint16 in the uint16 rank range, else uint32
    int32_t *seed, *nmask, *need_generic;   // [B]
    uint32_t *pop_log;                  // = sort_b: the batched flood's pop log (stride 2 EN), written once the ranks are out
    uint32_t *frontier_q, *frontier_i;  // = sort_a, sort_a + B EN: the generic flood's frontier (stride P), the sorted indices being dead by then
    unsigned long long *tree_words;     // = sort_a: k_unwrap_tree's 64-bit words (stride EN), after the floods
    UfPlanes check;
    size_t EN;
};
static UnwrapScratch unwrap_scratch(ScratchLayout &L, int B, int h, int w)
{
    UnwrapScratch S;
    S.EN = (size_t)padded_pixels(h, w);
    const size_t nb = (size_t)B, gn = nb * S.EN;
    S.state = L.take<uint8_t>(nb * h * w, 256, "state");
    S.sort_a = L.take<uint32_t>(2 * gn, 256, "sort_a");
    S.sort_b = L.take<uint32_t>(2 * gn, 256, "sort_b");
    S.ppar = L.take<int32_t>(gn, 256, "ppar");
    const size_t codes = nb * (size_t)code_stride((long)S.EN);
    if (unwrap_ranked_supported(h, w)) S.rank = L.take<uint16_t>(codes, 256, "rank");
    else S.rank = L.take<uint32_t>(codes, 256, "rank");
    S.seed = L.take<int32_t>(nb, 256, "seed");
    S.nmask = L.take<int32_t>(nb, 256, "nmask");
    S.need_generic = L.take<int32_t>(nb, 256, "need_generic");
    S.pop_log = S.sort_b;
    S.frontier_q = S.sort_a;
    S.frontier_i = S.sort_a ? S.sort_a + gn : nullptr;
    S.tree_words = (unsigned long long *)S.sort_a;
    S.check = unwrap_fast_planes(L, B, h, w);
    return S;
}
size_t unwrap_scratch_bytes(int B, int h, int w, ScratchRec *rec) { ScratchLayout L(nullptr, rec); unwrap_scratch(L, B, h, w); return L.bytes(); }

// the flood of an h x w frame (UnwrapTier); with big_handback the frames of the bitmap range still get their 32-bit ranks, and the generic flood grows them
int unwrap_tier(int h, int w, bool big_handback)
{
    return unwrap_tier_of(h, w, big_handback);
}

void launch_unwrap(const float *wrapped, const float *quality, const uint8_t *mask, float *unwrapped, int32_t *parent,
                   void *scratch, int32_t *status, int B, int h, int w, hipStream_t st, hipEvent_t ev_mid, hipEvent_t ev_flood, bool big_handback,
                   int32_t *need_buf)
{
    const int tier = unwrap_tier(h, w);      // by shape: big_handback acts inside the bitmap branch, frame by frame
    const int P = h * w;
    ScratchLayout L(scratch);
    const UnwrapScratch S = unwrap_scratch(L, B, h, w);
    const size_t EN = S.EN;
    // First the consistency check (k_unwrap_fast.hip): frames whose wrapped field is path-independent on the seed's component get their
    // plane from a parallel integration, and every kernel of the priority flood below skips them (need[b] = 0).  The parent plane of
    // such a frame is not produced (it is a by-product of the flood; the parity tests that compare trees switch the check off).
    const int32_t *need = nullptr;
    if (need_buf && unwrap_fast_supported(h, w)) {
        launch_unwrap_fast(wrapped, quality, mask, unwrapped, need_buf, S.check, B, h, w, st);
        need = need_buf;
    }
    // the generic flood (frontier and pixel states in global memory) and the tree kernel; only: the frames that take it, null for all of
    // them; ppar: padded parents of the other frames, from the bitmap flood
    auto flood_and_tree = [&](const int32_t *only, const int32_t *ppar) {
        hipLaunchKernelGGL(k_unwrap_flood, dim3(B), dim3(64), 0, st, quality, mask, parent, S.state, S.frontier_q, S.frontier_i, P, status, h, w, only, need);
        if (ev_mid) hipEventRecord(ev_mid, st);
        hipLaunchKernelGGL(k_unwrap_tree, dim3(B), dim3(1024), 0, st, wrapped, parent, ppar, EN, S.tree_words, unwrapped, h, w, only, need);
    };
    if (tier == UWT_RANK16) {
        // frames of the uint16 rank range: uint16 ranks, the batched flood in LDS, then the replay of its pop log
        launch_unwrap_ranked(quality, mask, S.sort_a, S.sort_b, S.ppar, EN, (uint16_t *)S.rank, S.seed, B, h, w, st, ev_flood, need);
        if (ev_mid) hipEventRecord(ev_mid, st);
        launch_unwrap_replay(wrapped, S.pop_log, 2 * EN, S.ppar, EN, parent, unwrapped, B, h, w, st, need);
    } else if (tier == UWT_BITMAP) {
        // frames beyond the uint16 rank range (native crops): 32-bit ranks, bitmap priority queue in LDS, plane in global memory
        // (k_unwrap_big.hip); masks too large for the bitmap (big_handback: every mask) go through the generic kernel, frame by frame
        launch_unwrap_rank32(quality, mask, S.sort_a, S.sort_b, EN, (uint32_t *)S.rank, S.seed, S.nmask, B, h, w, st, need);
        if (ev_flood) hipEventRecord(ev_flood, st);
        launch_unwrap_flood_big((uint32_t *)S.rank, S.seed, S.nmask, S.sort_a, 2 * EN, S.ppar, EN, S.need_generic, big_handback, B, h, w, st, need);
        flood_and_tree(S.need_generic, S.ppar);
    } else {
        // frames of 2^26 padded pixels and more: the generic kernel for every frame
        if (ev_flood) hipEventRecord(ev_flood, st);
        flood_and_tree(nullptr, nullptr);
    }
}

}  // namespace vf
