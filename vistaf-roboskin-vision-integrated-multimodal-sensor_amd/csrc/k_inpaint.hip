// cv2.inpaint(img_f32, mask, radius, INPAINT_TELEA) on the GPU (shape_ftp.py:652-666, :1199) -- the whole-frame kernel: any frame, any mask.
//
// Telea's fast-marching inpaint is ordered by a stable priority queue keyed on (T, push sequence)
// [OpenCV photo/inpaint.cpp CvPriorityQueueFloat], so the march itself is sequential per frame.  One
// wavefront owns one frame: the queue is a sorted array whose head is the next pop, the four quadrant
// solves of a pixel run on four lanes (the outside pass: four neighbours x four quadrants on sixteen), and
// the (2r+1)^2 terms of Telea's estimator are formed one window position per lane and summed in OpenCV's
// order, lane after lane (telea_common.hpp: wn_seq_sum_n).  Frames are independent, so a batch fills the
// chip with one wave per frame.  The arithmetic is the family's (telea_common.hpp); what is this kernel's
// own is the addressing: planes over the frame padded by ONE cell, so positions are tested against the
// frame by coordinates and OpenCV's index shifts at the image border are computed, not read off flags.
//
// Mutable per-frame state: flag planes (LDS when (h+2)*(w+2) fits, else global), T field and image in
// global memory.  Global mutable words are read with relaxed atomic loads (never merged or hoisted over
// a store) and every store is drained (workgroup fence) before the next dependent read.
#include <cstdio>
#include "host_util.hpp"
#include "telea_common.hpp"

namespace vf {

constexpr int TQ_CAP = 6144;                 // LDS queue capacity (entries): frames with more ring cells or hole pixels queue in global memory

// a mutable word in global memory; LF: a flag byte in LDS (plain read)
template <typename T>
__device__ inline T ldg(const T *p) { return ld_relaxed<__HIP_MEMORY_SCOPE_WAVEFRONT>(p); }
template <bool LF>
__device__ inline uint8_t ldf(const uint8_t *f, int i) { return LF ? f[i] : ldg(f + i); }
__device__ inline void drain() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); }

// Diagnostic shader-clock stamps / pop counts of frame 0: only in builds with -DVISTAF_DEBUG (the stamps are process-wide globals that
// concurrent sessions would race on, and s_memtime + a global store per phase is not free on a lone latency-bound wave).
#ifdef VISTAF_DEBUG
__device__ unsigned long long g_telea_dbg[16];
#define TSTAMP(i) do { if (b == 0 && lane == 0) g_telea_dbg[i] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define TSTAMP(i) do { } while (0)
#endif

// Stable priority queue kept as a SORTED array (the structure of OpenCV's CvPriorityQueueFloat), in LDS (LQ) or in the frame's slice of
// global memory -- which is why it is not the two-run WQ of the window marches.  FMM pushes are nearly monotone in T, so an insertion shifts
// only the few trailing entries with a larger T (found and moved by the 64 lanes at once) and lands AFTER every entry with T' <= T (FIFO
// among ties); pop is the head.  [head, tail) slides up; it is moved back to 0 when the array end is reached.
struct TQueue {
    uint32_t *T;       // float bits of T (>= 0), ascending in [head, tail)
    uint32_t *idx;
    int head, tail, cap;
    int overflow;
};

template <bool LQ>
__device__ inline void tq_push(TQueue &q, float Tf, int idx, int lane)
{
    if (!LQ) drain();
    if (q.tail >= q.cap) {
        if (q.head == 0) { q.overflow = 1; return; }
        int n = q.tail - q.head;
        for (int j0 = 0; j0 < n; j0 += 64) {
            int j = j0 + lane;
            uint32_t tv = 0, iv = 0;
            if (j < n) { tv = LQ ? q.T[j + q.head] : ldg(q.T + j + q.head); iv = LQ ? q.idx[j + q.head] : ldg(q.idx + j + q.head); }
            if (!LQ) drain();
            if (j < n) { q.T[j] = tv; q.idx[j] = iv; }
            if (!LQ) drain();
        }
        q.head = 0; q.tail = n;
    }
    const uint32_t tb = __float_as_uint(Tf);
    int k = 0;
    for (;;) {
        int j = q.tail - 1 - k - lane;
        bool in = j >= q.head;
        uint32_t tv = in ? (LQ ? q.T[j] : ldg(q.T + j)) : 0u;
        uint32_t iv = in ? (LQ ? q.idx[j] : ldg(q.idx + j)) : 0u;
        unsigned long long g = __ballot(in && tv > tb);
        int c = (g == ~0ull) ? 64 : (int)(__ffsll((long long)~g) - 1);     // leading run of "greater" entries
        if (!LQ) drain();
        if (lane < c) { q.T[j + 1] = tv; q.idx[j + 1] = iv; }
        if (!LQ) drain();
        k += c;
        if (c < 64) break;
    }
    if (lane == 0) { q.T[q.tail - k] = tb; q.idx[q.tail - k] = (uint32_t)idx; }
    q.tail++;
}

// pop the smallest (T, then oldest); -1 when empty (uniform)
template <bool LQ>
__device__ inline int tq_pop(TQueue &q)
{
    if (q.head == q.tail) return -1;
    if (!LQ) drain();
    int idx = (int)(LQ ? q.idx[q.head] : ldg(q.idx + q.head));
    q.head++;
    return __builtin_amdgcn_readfirstlane(idx);
}

// one quadrant of FastMarching_solve at the cells p1 (vertical neighbour) and p2 (horizontal neighbour)
template <bool LF>
__device__ inline float fmm_quadrant(const uint8_t *f, const float *t, int p1, int p2)
{
    return wn_solve(ldg(t + p1), ldg(t + p2), ldf<LF>(f, p1) != W_INSIDE, ldf<LF>(f, p2) != W_INSIDE);
}

// Parallel preparation (one thread per padded cell): Telea flags f (INSIDE on the hole), outside-pass flags fo
// (ring = within Chebyshev `range` of the hole, seeds = 4-neighbour band), T = 1e6 / 0 on the band, hole and ring cell counts.
__global__ void k_telea_prep(const uint8_t *__restrict__ bad_all, uint8_t *__restrict__ gflags, float *__restrict__ gT,
                             int32_t *__restrict__ nbad_all, int32_t *__restrict__ nring_all, const int32_t *__restrict__ only, int range, int h, int w)
{
    const int er = h + 2, ec = w + 2, en = er * ec;
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    size_t b = blockIdx.y;
    if (i >= en) return;
    if (only && !only[b]) return;      // frame already inpainted by the window kernel: its hole count stays 0
    const uint8_t *bad = bad_all + b * (size_t)h * w;
    int y = i / ec, x = i - y * ec;
    auto hole = [&](int yy, int xx) -> bool { return yy >= 1 && yy <= h && xx >= 1 && xx <= w && bad[(size_t)(yy - 1) * w + (xx - 1)] != 0; };
    bool interior = (y >= 1 && y <= h && x >= 1 && x <= w);
    bool in = hole(y, x);
    uint8_t fv = in ? W_INSIDE : W_KNOWN, fov = W_KNOWN;
    float tv = 1.0e6f;
    if (interior && !in) {
        const int kind = telea_known_pixel_kind(hole, y, x, range);
        if (kind == TC_BAND) { fov = W_KNOWN | W_SEED; tv = 0.f; }   // seeds: known, T = 0 (Heap->Add(band) / Out->Add(band))
        else if (kind == TC_RING) fov = W_INSIDE;
    }
    gflags[b * (size_t)en * 2 + i] = fv;
    gflags[b * (size_t)en * 2 + en + i] = fov;
    gT[b * (size_t)en + i] = tv;
    if (in) atomicAdd(&nbad_all[b], 1);
    // a dense mask puts most of the frame on the ring: one atomic per wave (the lanes that returned above take no part in the ballot)
    const unsigned long long mr = __ballot(fov == W_INSIDE);
    if (mr && (int)(threadIdx.x & 63) == __ffsll((long long)mr) - 1) atomicAdd(&nring_all[b], __popcll(mr));
}

// Both passes over the whole padded frame.  The two planes hold a state (W_KNOWN .. W_CHANGE) per cell, the outside pass's plane fo also the
// W_SEED bit.  LF: the flag planes are in LDS; LQ: so is the queue (else in global memory, read with relaxed loads and drained stores)
template <bool LF, bool LQ>
__device__ __attribute__((always_inline)) inline void telea_march_global(float *img, int range, uint8_t *f, uint8_t *fo, float *t, TQueue &q, int h, int w,
                                                                         int lane, size_t b, bool round_u8 = false)
{
    const int er = h + 2, ec = w + 2, en = er * ec;
    // the pops of a pass: the seeds (band pixels) in raster order, then the queue until it is empty; -1 at the end
    int phase = 0, base = 0, pass = 0;
    unsigned long long pend = 0;
    auto next_pop = [&]() -> int {
        if (phase == 0) {
            const int p = wn_next_seed<LF>(fo, en, base, pend, lane);
            if (p >= 0) return p;
            phase = 1;
            TSTAMP(pass == 0 ? 2 : 5);
        }
        return tq_pop<LQ>(q);
    };
    TSTAMP(1);
    unsigned long long npop1 = 0, npop2 = 0;
    // ---- pass 1: outside T field
    for (int p; (p = next_pop()) >= 0;) {
        npop1++;
        if (lane == 0) fo[p] = (uint8_t)(W_CHANGE | (phase == 0 ? W_SEED : 0));
        // the four 4-neighbours are independent of one another in this pass: lanes 0..15 = 4 pixels x 4 quadrants
        int nb = lane >> 2;
        int pn = nb == 0 ? p - ec : nb == 1 ? p - 1 : nb == 2 ? p + ec : p + 1;
        bool ok = false;
        float dist = 0.f;
        if (lane < 16) {
            int y = pn / ec, x = pn - y * ec;
            ok = (y > 0 && x > 0 && y < er - 1 && x < ec - 1) && ldf<LF>(fo, pn) == W_INSIDE;
        }
        if (__ballot(ok)) {
            drain();
            if (ok) {
                int qd = lane & 3;
                dist = fmm_quadrant<LF>(fo, t, (qd & 1) ? pn + ec : pn - ec, (qd & 2) ? pn + 1 : pn - 1);
            }
            dist = quad_min(dist);
            for (int k = 0; k < 4; k++) {
                bool okk = __builtin_amdgcn_readlane((int)ok, k * 4) != 0;
                if (!okk) continue;
                float dk = wn_lane_f(dist, k * 4);
                int pk = __builtin_amdgcn_readlane(pn, k * 4);
                if (lane == 0) { t[pk] = dk; fo[pk] = W_BAND; }
                tq_push<LQ>(q, dk, pk, lane);
            }
        }
        if (LF) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    }
    drain();
    __syncthreads();
    TSTAMP(3);
    // negate T where the outside pass ran (CHANGE; the seeds' T = 0 stays zero)
    for (int i = lane; i < en; i += 64)
        if ((ldf<LF>(fo, i) & W_ST) == W_CHANGE) { float v = ldg(t + i); t[i] = -v; }
    drain();
    __syncthreads();

    TSTAMP(4);
    // ---- pass 2: Telea march
    q.head = q.tail = 0;
    phase = 0; base = 0; pend = 0; pass = 1;
    const int r2 = range * range, side = 2 * range + 1, nn = side * side;
    // 1 / |r|^3 of this lane's window position in the first two 64-position chunks, hoisted out of the march
    float pre_dstw[2];
    for (int c2 = 0; c2 < 2; c2++) {
        const int nidx = c2 * 64 + lane;
        pre_dstw[c2] = telea_dstw((float)(range - nidx % side), (float)(range - nidx / side));
    }
    for (int p; (p = next_pop()) >= 0;) {
        npop2++;
        if (phase == 1 && lane == 0) f[p] = W_KNOWN;
        if (LF) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); else drain();
        for (int qn = 0; qn < 4; qn++) {
            int pi = qn == 0 ? p - ec : qn == 1 ? p - 1 : qn == 2 ? p + ec : p + 1;
            int i = pi / ec, j = pi - i * ec;
            if (i <= 0 || j <= 0 || i >= er - 1 || j >= ec - 1) continue;
            if (ldf<LF>(f, pi) != W_INSIDE) continue;
            drain();
            // T of the pixel = min over the four quadrants (i-1,j-1) (i+1,j-1) (i-1,j+1) (i+1,j+1), one per lane of every quad
            const int qd = lane & 3;
            const float tc = wn_lane_f(quad_min(fmm_quadrant<LF>(f, t, (qd & 1) ? pi + ec : pi - ec, (qd & 2) ? pi + 1 : pi - 1)), 0);
            if (lane == 0) t[pi] = tc;
            // gradT at (i,j): uses the T just computed for the centre
            const bool kr = ldf<LF>(f, pi + 1) != W_INSIDE, kl = ldf<LF>(f, pi - 1) != W_INSIDE;
            const bool kd = ldf<LF>(f, pi + ec) != W_INSIDE, ku = ldf<LF>(f, pi - ec) != W_INSIDE;
            const float gtx = telea_grad_T(kr, kl, ldg(t + pi + 1), ldg(t + pi - 1), tc), gty = telea_grad_T(kd, ku, ldg(t + pi + ec), ldg(t + pi - ec), tc);
            float sIa = 0, sJx = 0, sJy = 0, sS = 1.0e-20f;     // running sums in OpenCV's order: chunk after chunk, lane after lane
            for (int n0 = 0; n0 < nn; n0 += 64) {
                int nidx = n0 + lane;
                TeleaTerms a = {0.f, 0.f, 0.f, 0.f};
                if (nidx < nn) {
                    int k = i - range + nidx / side, l = j - range + nidx % side;
                    if (k > 0 && l > 0 && k < er - 1 && l < ec - 1) {
                        int pk = k * ec + l;
                        if (ldf<LF>(f, pk) != W_INSIDE && ((l - j) * (l - j) + (k - i) * (k - i) <= r2)) {
                            // OpenCV's index shifts at the first / last image row / column
                            const int km = k - 1 + (k == 1), kp = k - 1 - (k == er - 2);
                            const int lm = l - 1 + (l == 1), lp = l - 1 - (l == ec - 2);
                            const float ry = (float)(i - k), rx = (float)(j - l);
                            const float dstw = n0 == 0 ? pre_dstw[0] : (n0 == 64 ? pre_dstw[1] : telea_dstw(rx, ry));
                            const float tk = (pk == pi) ? tc : ldg(t + pk);
                            const float wgt = telea_weight(dstw, telea_lev(tk, tc), telea_dir(rx, ry, gtx, gty));
                            const float *rm = img + (size_t)km * w;
                            TeleaImg v;
                            v.vC = ldg(rm + lm); v.vA = ldg(rm + lp + 1); v.vB = ldg(rm + lm - 1); v.vD = ldg(rm + lp);
                            v.vE = ldg(img + (size_t)(kp + 1) * w + lm); v.vF = ldg(img + (size_t)(km - 1) * w + lm); v.vG = ldg(img + (size_t)kp * w + lm);
                            const bool nr = ldf<LF>(f, pk + 1) != W_INSIDE, nl = ldf<LF>(f, pk - 1) != W_INSIDE;
                            const bool nd = ldf<LF>(f, pk + ec) != W_INSIDE, nu = ldf<LF>(f, pk - ec) != W_INSIDE;
                            a = telea_terms(true, wgt, v.vC, telea_grad_I(nr, nl, v.vA, v.vB, v.vC, v.vD), telea_grad_I(nd, nu, v.vE, v.vF, v.vC, v.vG), rx, ry);
                        }
                    }
                }
                const int nl = nn - n0 < 64 ? nn - n0 : 64;
                sIa = wn_seq_sum_n(a.Ia, sIa, nl, lane);
                sJx = wn_seq_sum_n(a.Jx, sJx, nl, lane);
                sJy = wn_seq_sum_n(a.Jy, sJy, nl, lane);
                sS = wn_seq_sum_n(a.s, sS, nl, lane);
            }
            const float val = round_u8 ? telea_estimate_u8(sIa, sJx, sJy, sS) : telea_estimate(sIa, sJx, sJy, sS);
            if (lane == 0) { img[(size_t)(i - 1) * w + (j - 1)] = val; f[pi] = W_BAND; }
            tq_push<LQ>(q, tc, pi, lane);
            if (LF) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        }
    }
    TSTAMP(6);
#ifdef VISTAF_DEBUG
    if (b == 0 && lane == 0) { g_telea_dbg[8] = npop1; g_telea_dbg[9] = npop2; }
#endif
    (void)npop1; (void)npop2; (void)pass;
}

template <bool LF>
__global__ __launch_bounds__(64) void k_telea(float *__restrict__ img_all, int range, uint8_t *gflags, float *gT, uint32_t *gqueue,
                                              const int32_t *__restrict__ nbad_all, const int32_t *__restrict__ nring_all, int32_t *status, int h, int w,
                                              int round_u8)
{
    extern __shared__ unsigned char lds_raw[];
    const int lane = threadIdx.x;
    const size_t b = blockIdx.x;
    const int er = h + 2, ec = w + 2, en = er * ec, P = h * w;
    float *img = img_all + b * (size_t)P;
    float *t = gT + b * (size_t)en;
    TQueue q;
    q.head = q.tail = 0; q.overflow = 0;
    uint8_t *f, *fo;
    if (LF) { f = lds_raw + (size_t)TQ_CAP * 8; fo = f + ((en + 15) & ~15); }
    else { f = gflags + b * (size_t)en * 2; fo = f + en; }
    TSTAMP(0);
    // ---- flags and the initial T field were prepared by k_telea_prep (all CUs); stage the flag planes into LDS
    if (nbad_all[b] == 0) return;
    if (LF) {
        const uint8_t *gsrc = gflags + b * (size_t)en * 2;
        for (int i = lane; i < en; i += 64) { f[i] = gsrc[i]; fo[i] = gsrc[en + i]; }
        __syncthreads();
    }
    // The outside pass pushes every ring cell once and the march every hole pixel once, and a pass starts with an empty queue: a frame
    // with no more of either than TQ_CAP can never have more live entries than the LDS queue holds.  Any other frame -- a checkerboard, a
    // lattice of single pixels, a few per cent of scattered pixels: their band alone is longer -- keeps the same sorted run in its slice of
    // global memory, which holds a cell for every cell of the frame.  Same pushes, same pops, same order either way, so the same bits; and no
    // frame overflows (the check in tq_push stays: status 2 would mean that this argument is broken, not that the mask is dense).
    if (LF && max(nbad_all[b], nring_all[b]) <= TQ_CAP) {
        q.T = (uint32_t *)lds_raw; q.idx = (uint32_t *)(lds_raw + (size_t)TQ_CAP * 4); q.cap = TQ_CAP;
        telea_march_global<LF, true>(img, range, f, fo, t, q, h, w, lane, b, round_u8 != 0);
    } else {
        q.T = gqueue + b * (size_t)en * 2; q.idx = q.T + en; q.cap = en;
        telea_march_global<LF, false>(img, range, f, fo, t, q, h, w, lane, b, round_u8 != 0);
    }
    if (q.overflow && lane == 0) status[b] = 2;
}

#ifdef VISTAF_DEBUG
void telea_debug_dump()
{
    unsigned long long h[16];
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_telea_dbg), sizeof(h)) != hipSuccess) return;
    printf("[telea dbg] cycles: init %llu | pass1 seeds %llu | pass1 queue %llu | negate %llu | pass2 seeds %llu | pass2 queue %llu | pops %llu / %llu | bad %llu\n",
           h[1] - h[0], h[2] - h[1], h[3] - h[2], h[4] - h[3], h[5] - h[4], h[6] - h[5], h[8], h[9], h[10]);
}
#endif

// planes of the whole-frame kernel over the frame padded by one cell, en = (h + 2)(w + 2)
struct TeleaScratch {
    float *T;               // [B, en]
    uint8_t *flags;         // [B, 2 en] the two flag planes of a frame, one behind the other
    uint32_t *queue;        // [B, 2 en] keys, then indices: the queue of the frames whose ring or hole outgrows the LDS queue, or whose flags do not fit LDS
    int32_t *nbad, *nring;  // [B] hole pixels, ring cells; one region (one memset clears both)
};
static TeleaScratch telea_scratch(ScratchLayout &L, int B, int h, int w)
{
    const size_t n = (size_t)B * (h + 2) * (w + 2);
    TeleaScratch S;
    S.T = L.take<float>(n, 256, "T");
    S.flags = L.take<uint8_t>(2 * n, 256, "flags");
    S.queue = L.take<uint32_t>(2 * n, 256, "queue");
    S.nbad = L.take<int32_t>(2 * (size_t)B, 256, "nbad");
    S.nring = S.nbad ? S.nbad + B : nullptr;
    return S;
}
size_t telea_scratch_bytes(int B, int h, int w, ScratchRec *rec) { ScratchLayout L(nullptr, rec); telea_scratch(L, B, h, w); return L.bytes(); }
size_t inpaint_scratch_bytes(int B, int h, int w) { return std::max(telea_scratch_bytes(B, h, w), inpaint_big_scratch_bytes(B, h, w)); }

static size_t telea_lds_bytes(int h, int w)
{
    size_t en = (size_t)(h + 2) * (w + 2);
    return (size_t)TQ_CAP * 8 + 2 * ((en + 15) & ~(size_t)15);
}

void launch_inpaint_telea(float *img, const uint8_t *bad, int range, void *scratch, int32_t *status, const int32_t *only, int B, int h,
                          int w, hipStream_t st, bool round_u8)
{
    const size_t en = (size_t)(h + 2) * (w + 2);
    ScratchLayout L(scratch);
    const TeleaScratch S = telea_scratch(L, B, h, w);
    hipMemsetAsync(S.nbad, 0, sizeof(int32_t) * 2 * B, st);
    hipLaunchKernelGGL(k_telea_prep, dim3((unsigned)((en + 255) / 256), B), dim3(256), 0, st, bad, S.flags, S.T, S.nbad, S.nring, only, range, h, w);
    size_t lds_full = telea_lds_bytes(h, w);
    if (lds_full <= 160 * 1024) {
        static DynLdsOnce lds_once;
        ensure_dyn_lds(lds_once, (const void *)k_telea<true>, 160 * 1024);
        hipLaunchKernelGGL(k_telea<true>, dim3(B), dim3(64), lds_full, st, img, range, S.flags, S.T, S.queue, S.nbad, S.nring, status, h, w, round_u8 ? 1 : 0);
    } else {
        hipLaunchKernelGGL(k_telea<false>, dim3(B), dim3(64), 0, st, img, range, S.flags, S.T, S.queue, S.nbad, S.nring, status, h, w, round_u8 ? 1 : 0);
    }
}

}  // namespace vf
