// Lobe read-out (include_ext/vistaf_lobes.h): the depth maxima inside every contact, their prominence over the saddles that join them, the
// lobes the contact splits into and the table of those lobes in the layout of the contacts table.  An extension, as the other per-contact
// read-outs: the reference has no counterpart.  The definition is in the header; tests/lobes_helpers.py restates it in NumPy.
//
// One workgroup of 1024 threads per (frame, row) on the row's clipped box of n = bw * bh pixels, with tables per pixel (depth key, top, basin)
// and per maximum (at most ceil(bw / 2) * ceil(bh / 2): two maxima are never 8-adjacent).  A box whose tables fit LB_LDS_BUDGET works in
// LDS; a larger one runs the same code over tables in the caller's workspace (lb_box_in_lds; test_hooks_lobes.h tells the tiers apart).
//   k_fill_i8<-1>  (contact_rows.hpp) writes -1 over the lobe plane.
//   k_lobes_rows   packs the order of the header's step 1 into one unsigned key per pixel; finds up(p) in one sweep and top(p) by pointer
//                  jumping; lists the maxima in row-major order with a block scan; builds the maximum spanning forest of the basin graph under
//                  the pass order by Boruvka rounds (every crossing pair offers its packed pass key to both components' best-edge slots with
//                  an integer atomicMax; the order is strict and total, so the forest is unique and is the set of passes at which step 4 joins
//                  two components); sorts those passes (bitonic) and lane 0 replays them in descending order with a union-find for the elder
//                  rule -- the only serial part, RAW_MAXIMA - 1 steps; follows into() to the peaks by pointer jumping; numbers the peaks by a
//                  second sort; writes the lobe plane; then one sweep of the box per written lobe for its sums, each a block reduction in a
//                  fixed order.
//   k_lobes_split  one workgroup per frame: ranks the written lobes of all rows by their peaks and writes the split table, count and parents.
//   k_lobes_plane  writes the split index plane from the contact index plane, the lobe plane and the ranks.
// No memset, no float atomics, no host read-back; the integer atomics (a maximum, a counter whose order a sort removes) do not depend on
// the order of arrival, so a frame gives the same bits wherever it stands.
#include <string>

#include "../../include_ext/vistaf_lobes.h"
#include "contact_rows.hpp"
#include "host_util.hpp"
#include "test_hooks_lobes.h"

using namespace vf;

namespace {

typedef unsigned long long u64;

// 1024 threads for the row kernel: a workgroup's time is sweeps of the box, each a chain of dependent loads, so the threads of a workgroup
// are what hides their latency on a large box (measured: DESIGN.md); the frame kernel has little to do
constexpr int LB_NT = 1024, LB_SPLIT_NT = 256, LB_MAXL = VISTAF_LOBES_MAX;
// The LDS a row's tables may take (contact_rows.hpp).  A 51 x 51 box fits (12 bytes per pixel, 32 per possible maximum, 8 per slot of the
// sort); no occupancy or time has been measured for this kernel.
constexpr int LB_LDS_BUDGET = ROW_LDS_BUDGET;
constexpr int LB_AUX = 4;          // per written lobe, for k_lobes_split: depth sum bits, peak key, x0 | y0 << 32, x1 | y1 << 32

// ---- pure rules -----------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline size_t lb_max_cap(int bw, int bh) { return (size_t)((bw + 1) / 2) * (size_t)((bh + 1) / 2); }
__host__ __device__ inline size_t lb_pow2(size_t v) { size_t p = 1; while (p < v) p <<= 1; return p; }
// the tables of one row, in the order of their alignment: best, sad [MC] and edges [pow2(MC)] u64; mpix, comp, into, ptr [MC] int32;
// dk [n] uint32; top, lab [n] int32
__host__ __device__ inline size_t lb_row_bytes(int bw, int bh)
{
    const size_t n = (size_t)bw * bh, mc = lb_max_cap(bw, bh);
    return 8 * (2 * mc + lb_pow2(mc)) + 4 * (4 * mc) + 12 * n;
}
__host__ __device__ inline bool lb_box_in_lds(int bw, int bh) { return lb_row_bytes(bw, bh) <= (size_t)LB_LDS_BUDGET; }
// the dynamic LDS of a launch over h x w frames: what the largest box that can take the LDS tier needs, never more than the budget
inline size_t lb_launch_lds(int h, int w) { return lb_box_in_lds(w, h) ? lb_row_bytes(w, h) : (size_t)LB_LDS_BUDGET; }

// The workspace.  Per frame: the lobe plane (used when the caller gives none).  Per (frame, row): the ranks of its lobes in the split table
// and LB_AUX words per lobe; the row's tables sized for a box of the whole frame, unless every box of such a frame takes the LDS tier.
struct LobesBufs {
    int8_t *plane;
    int32_t *rank;
    u64 *aux;
    uint8_t *rows;
    size_t row_stride;       // bytes of one row's tables, a multiple of 256 (0: no box leaves LDS)
};

LobesBufs lobes_scratch(ScratchLayout &L, int B, int h, int w, int K)
{
    LobesBufs bf;
    bf.aux = L.take<u64>((size_t)B * K * LB_MAXL * LB_AUX, 256, "lobe_aux");
    bf.rank = L.take<int32_t>((size_t)B * K * LB_MAXL, 256, "lobe_rank");
    bf.plane = L.take<int8_t>((size_t)B * h * w, 256, "lobe_plane");
    bf.row_stride = lb_box_in_lds(w, h) ? 0 : (lb_row_bytes(w, h) + 255) & ~(size_t)255;
    bf.rows = L.take<uint8_t>((size_t)B * K * bf.row_stride, 256, "row_tables");
    return bf;
}

size_t lobes_scratch_bytes(int B, int h, int w, int K, ScratchRec *rec = nullptr)
{
    return scratch_bytes([&](ScratchLayout &L) { return lobes_scratch(L, B, h, w, K); }, rec);
}

struct LbArgs {
    const int8_t *index;
    const double *contacts;
    const int32_t *count;
    const double *mm_per_px;
    const float *depth;
    int h, w, K, max_lobes;
    double min_mm, min_frac;
    float eps;
    double *lobes, *rows;
    int8_t *plane;           // the caller's lobe plane or the workspace's
    LobesBufs bf;
};

// the tables of a row carved from `base` (8-byte aligned), and the rules on them
struct LbTab {
    int bw, bh, n, mc;
    u64 *best, *sad, *edges;
    int32_t *mpix, *comp, *into, *ptr;
    uint32_t *dk;
    int32_t *top, *lab;
    __device__ inline LbTab(uint8_t *base, int bw_, int bh_) : bw(bw_), bh(bh_), n(bw_ * bh_), mc((int)lb_max_cap(bw_, bh_))
    {
        best = (u64 *)base; sad = best + mc; edges = sad + mc;
        mpix = (int32_t *)(edges + lb_pow2((size_t)mc)); comp = mpix + mc; into = comp + mc; ptr = into + mc;
        dk = (uint32_t *)(ptr + mc);
        top = (int32_t *)(dk + n); lab = top + n;
    }
    // the order of step 1 as one unsigned compare: 0 for a position that is no pixel of the row
    __device__ inline u64 key(int p) const { return ((u64)dk[p] << 32) | (u64)(0xffffffffu - (uint32_t)p); }
    __device__ inline u64 key_at(int x, int y) const
    {
        if (x < 0 || x >= bw || y < 0 || y >= bh) return 0ull;
        const int p = y * bw + x;
        return dk[p] ? key(p) : 0ull;
    }
    // the keys of the 8 neighbours of p (0 where there is none) and their box indices
    __device__ inline void ring(int p, u64 nk[8], int np[8]) const
    {
        const int y = p / bw, x = p - y * bw;
        int q = 0;
        for (int dy = -1; dy <= 1; dy++)
            for (int dx = -1; dx <= 1; dx++) {
                if (!dx && !dy) continue;
                nk[q] = key_at(x + dx, y + dy);
                np[q] = (y + dy) * bw + x + dx;
                q++;
            }
    }
    // the pass (lo, hi = neighbour q of lo) as one key: the order of step 3.  The last three bits say how many neighbours of lo hi exceeds.
    __device__ static inline u64 pass_key(uint32_t dk_lo, int lo, const u64 nk[8], int q)
    {
        int code = 0;
        for (int r = 0; r < 8; r++) code += nk[r] && nk[q] > nk[r];
        return ((u64)dk_lo << 32) | ((u64)(0x1fffffffu - (uint32_t)lo) << 3) | (u64)code;
    }
    __device__ static inline int pass_lo(u64 e) { return (int)(0x1fffffffu - (uint32_t)((e >> 3) & 0x1fffffffull)); }
    __device__ inline int pass_hi(u64 e) const
    {
        const int lo = pass_lo(e);
        u64 nk[8];
        int np[8];
        ring(lo, nk, np);
        const u64 kl = key(lo);
        for (int q = 0; q < 8; q++)
            if (nk[q] > kl && pass_key(dk[lo], lo, nk, q) == e) return np[q];
        return lo;       // not reached: e was made from one of these neighbours
    }
    __device__ inline u64 max_key(int i) const { return key(mpix[i]); }
};

// descending bitonic sort of e[0..n2), n2 a power of two; every thread calls it
__device__ inline void lb_sort_desc(u64 *e, int n2)
{
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < n2; i += LB_NT) {
                const int o = i ^ j;
                if (o > i) {
                    const u64 a = e[i], b = e[o];
                    if (((i & k) == 0) ? a < b : a > b) { e[i] = b; e[o] = a; }
                }
            }
            block_sync_fenced();
        }
}

__device__ inline void lb_empty_row(const LbArgs &a, double *row, double *lobes)
{
    empty_row(row, VISTAF_NLOBEROW, VISTAF_LOBEROW_STATUS, VISTAF_LOBEST_NO_PIXELS);
    for (int i = threadIdx.x; i < a.max_lobes * VISTAF_NLOBE; i += LB_NT) lobes[i] = nan64();
}

// The body of k_lobes_rows for a row with a box: base holds the tables, in LDS or in the workspace
__device__ __forceinline__ void lb_row(uint8_t *base, const LbArgs &a, const ContactBox &box, int b, int k)
{
    __shared__ u64 red[16];
    __shared__ double redd[16];
    __shared__ int wtot[LB_NT / 64];
    __shared__ int nedges_s;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const LbTab t(base, box.bw, box.bh);
    const size_t P = (size_t)a.h * a.w;
    const int8_t *index = a.index + b * P;
    const float *depth = a.depth + b * P;
    double *row = a.rows + ((size_t)b * a.K + k) * VISTAF_NLOBEROW;
    double *lobes = a.lobes + ((size_t)b * a.K + k) * a.max_lobes * VISTAF_NLOBE;
    const int n = t.n, bw = t.bw;

    // ---- the keys: a sample that is not finite counts as 0, and -0 as 0
    u64 npix = 0;
    for (int p = tid; p < n; p += LB_NT) {
        const int y = p / bw, x = p - y * bw;
        const size_t f = (size_t)(box.y0 + y) * a.w + box.x0 + x;
        uint32_t key = 0;
        if (index[f] == k) {
            float d = depth[f];
            if (!finitef(d) || d == 0.f) d = 0.f;
            key = f2key(d);
            npix++;
        }
        t.dk[p] = key;
    }
    npix = block_sum(npix, red);
    if (npix == 0) { lb_empty_row(a, row, lobes); return; }
    if (tid == 0) nedges_s = 0;
    block_sync_fenced();

    // ---- up(p), then top(p) by pointer jumping
    for (int p = tid; p < n; p += LB_NT) {
        int up = -1;
        if (t.dk[p]) {
            u64 nk[8], bk = t.key(p);
            int np[8];
            t.ring(p, nk, np);
            up = p;
            for (int q = 0; q < 8; q++)
                if (nk[q] > bk) { bk = nk[q]; up = np[q]; }
        }
        t.top[p] = up;
    }
    block_sync_fenced();
    for (;;) {
        bool moved = false;
        for (int p = tid; p < n; p += LB_NT) {
            const int u = t.top[p];
            if (u < 0) continue;
            const int uu = t.top[u];
            if (uu != u) { t.top[p] = uu; moved = true; }
        }
        if (!block_any_fenced(moved)) break;
    }

    // ---- the maxima in row-major order; lab(p) = the number of top(p) in that list
    int M = 0;
    for (int p0 = 0; p0 < n; p0 += LB_NT) {
        const int p = p0 + tid;
        const int flag = p < n && t.top[p] == p ? 1 : 0;
        int tot;                                 // its own block scan: with common.hpp's block_excl_scan the call measured 0.6 % above the parent's range
        const int ex = wave_excl_scan(flag, tot);
        if (lane == 0) wtot[wid] = tot;
        __syncthreads();
        int off = M, all = 0;
        for (int i = 0; i < LB_NT / 64; i++) { if (i < wid) off += wtot[i]; all += wtot[i]; }
        if (flag) { t.mpix[off + ex] = p; t.lab[p] = off + ex; }
        M += all;
        __syncthreads();
    }
    block_sync_fenced();
    for (int p = tid; p < n; p += LB_NT) {
        const int u = t.top[p];
        if (u >= 0 && u != p) t.lab[p] = t.lab[u];
    }
    for (int i = tid; i < M; i += LB_NT) t.comp[i] = i;
    block_sync_fenced();

    // ---- Boruvka rounds over the basin graph: the passes of the maximum spanning forest go to edges[]
    for (;;) {
        for (int i = tid; i < M; i += LB_NT) t.best[i] = 0ull;
        block_sync_fenced();
        bool offered = false;
        for (int p = tid; p < n; p += LB_NT) {
            if (!t.dk[p]) continue;
            u64 nk[8];
            int np[8];
            t.ring(p, nk, np);
            const u64 kp = t.key(p);
            const int ca = t.comp[t.lab[p]];
            for (int q = 0; q < 8; q++) {
                if (nk[q] <= kp) continue;
                const int cb = t.comp[t.lab[np[q]]];
                if (ca == cb) continue;
                const u64 e = LbTab::pass_key(t.dk[p], p, nk, q);
                atomicMax(&t.best[ca], e);
                atomicMax(&t.best[cb], e);
                offered = true;
            }
        }
        if (!block_any_fenced(offered)) break;
        for (int i = tid; i < M; i += LB_NT) {
            int hook = -1;
            const u64 e = t.best[i];
            if (t.comp[i] == i && e) {
                const int ca = t.comp[t.lab[LbTab::pass_lo(e)]], cb = t.comp[t.lab[t.pass_hi(e)]];
                const int o = ca == i ? cb : ca;
                if (!(t.best[o] == e && i < o)) {          // of two components that chose the same pass the one with the smaller number stays
                    hook = o;
                    t.edges[atomicAdd(&nedges_s, 1)] = e;
                }
            }
            t.into[i] = hook;
        }
        block_sync_fenced();
        for (int i = tid; i < M; i += LB_NT)
            if (t.into[i] >= 0) t.comp[i] = t.into[i];
        block_sync_fenced();
        for (;;) {
            bool moved = false;
            for (int i = tid; i < M; i += LB_NT) {
                const int c = t.comp[i], cc = t.comp[c];
                if (cc != c) { t.comp[i] = cc; moved = true; }
            }
            if (!block_any_fenced(moved)) break;
        }
    }
    const int nedges = nedges_s;
    const int M2 = (int)lb_pow2((size_t)M);

    // ---- the forest's passes in descending order, their two basins decoded by all threads; then lane 0 replays them for the elder rule
    for (int i = nedges + tid; i < M2; i += LB_NT) t.edges[i] = 0ull;
    block_sync_fenced();
    lb_sort_desc(t.edges, M2);
    for (int i = tid; i < M; i += LB_NT) {
        if (i < nedges) {
            const u64 e = t.edges[i];
            t.best[i] = ((u64)(uint32_t)t.lab[LbTab::pass_lo(e)] << 32) | (u64)(uint32_t)t.lab[t.pass_hi(e)];
        }
        t.comp[i] = i;          // the union-find of the replay
        t.ptr[i] = i;           // the elder of a root
        t.sad[i] = 0ull;
        t.into[i] = -1;
    }
    block_sync_fenced();
    if (tid == 0) {
        for (int j = 0; j < nedges; j++) {
            const int ba = (int)(t.best[j] >> 32), bb = (int)(t.best[j] & 0xffffffffull);
            int ra = ba, rb = bb;
            while (t.comp[ra] != ra) { t.comp[ra] = t.comp[t.comp[ra]]; ra = t.comp[ra]; }
            while (t.comp[rb] != rb) { t.comp[rb] = t.comp[t.comp[rb]]; rb = t.comp[rb]; }
            if (ra == rb) continue;          // not reached: a forest has no cycle
            const int ea = t.ptr[ra], eb = t.ptr[rb];
            if (t.max_key(ea) < t.max_key(eb)) { t.sad[ea] = t.edges[j]; t.into[ea] = bb; t.comp[ra] = rb; }
            else { t.sad[eb] = t.edges[j]; t.into[eb] = ba; t.comp[rb] = ra; }
        }
    }
    block_sync_fenced();

    // ---- the threshold, the peaks, the chain of into() down to a peak
    u64 gk = 0;
    for (int i = tid; i < M; i += LB_NT) { const u64 v = t.max_key(i); gk = v > gk ? v : gk; }
    gk = block_max_u64(gk, red);
    const double dmax = (double)key2f((uint32_t)(gk >> 32));
    const double ft = a.min_frac * dmax, tau = a.min_mm > ft ? a.min_mm : ft;
    u64 next = 0, deepest = 0, npeaks = 0;
    for (int i = tid; i < M; i += LB_NT) {
        const u64 sd = t.sad[i];
        bool peak = true;
        if (sd) {
            const double prom = (double)key2f(t.dk[t.mpix[i]]) - (double)key2f((uint32_t)(sd >> 32));
            peak = prom > tau;
            if (peak) { const u64 v = sd >> 32; deepest = v > deepest ? v : deepest; }
            else { const u64 v = (u64)__double_as_longlong(prom) + 1ull; next = v > next ? v : next; }       // prom >= 0: its bits order it
        }
        npeaks += peak ? 1 : 0;
        t.ptr[i] = peak ? i : t.into[i];
    }
    next = block_max_u64(next, red);
    deepest = block_max_u64(deepest, red);
    const int peaks = (int)block_sum(npeaks, red);
    block_sync_fenced();
    for (int round = 0; round < 32; round++) {          // the chain ends (header, step 6); 2^32 exceeds any number of maxima
        bool moved = false;
        for (int i = tid; i < M; i += LB_NT) {
            const int c = t.ptr[i], cc = t.ptr[c];
            if (cc != c) { t.ptr[i] = cc; moved = true; }
        }
        if (!block_any_fenced(moved)) break;
    }

    // ---- the lobes' numbers: the peaks in descending order; comp[] now holds the lobe of every maximum
    for (int i = tid; i < M2; i += LB_NT) t.edges[i] = i < M && t.ptr[i] == i ? t.max_key(i) : 0ull;
    block_sync_fenced();
    lb_sort_desc(t.edges, M2);
    for (int j = tid; j < peaks; j += LB_NT) t.comp[t.lab[(int)(0xffffffffu - (uint32_t)t.edges[j])]] = j;
    block_sync_fenced();
    for (int i = tid; i < M; i += LB_NT)
        if (t.ptr[i] != i) t.comp[i] = t.comp[t.ptr[i]];
    block_sync_fenced();

    // ---- the lobe plane, the depth sum of the whole contact
    const int L = peaks < a.max_lobes ? peaks : a.max_lobes;
    int8_t *plane = a.plane + b * P;
    double all = 0.0;
    for (int p = tid; p < n; p += LB_NT) {
        if (!t.dk[p]) continue;
        const int y = p / bw, x = p - y * bw, l = t.comp[t.lab[p]];
        plane[(size_t)(box.y0 + y) * a.w + box.x0 + x] = (int8_t)(l < a.max_lobes ? l : -2);
        const float d = key2f(t.dk[p]);
        if (d > a.eps) all += (double)d;
    }
    all = block_sum(all, redd);
    const double s = a.mm_per_px[b], s2 = s * s;
    const double force = a.contacts[((size_t)b * a.K + k) * VISTAF_NCONTACT + VISTAF_CONTACT_FORCE_N];

    // ---- one sweep per written lobe
    u64 *aux = a.bf.aux + ((size_t)b * a.K + k) * LB_MAXL * LB_AUX;
    for (int j = 0; j < L; j++) {
        u64 pix = 0, cpix = 0, x0 = ~0ull, y0 = ~0ull, x1 = 0, y1 = 0, basins = 0;
        double S = 0.0, SX = 0.0, SY = 0.0;
        for (int p = tid; p < n; p += LB_NT) {
            if (!t.dk[p] || t.comp[t.lab[p]] != j) continue;
            const int y = box.y0 + p / bw, x = box.x0 + p % bw;
            pix++;
            x0 = (u64)x < x0 ? (u64)x : x0; y0 = (u64)y < y0 ? (u64)y : y0;
            x1 = (u64)x > x1 ? (u64)x : x1; y1 = (u64)y > y1 ? (u64)y : y1;
            const float d = key2f(t.dk[p]);
            if (d > a.eps) { cpix++; S += (double)d; SX += (double)x * (double)d; SY += (double)y * (double)d; }
        }
        for (int i = tid; i < M; i += LB_NT) basins += t.comp[i] == j ? 1 : 0;
        pix = block_sum(pix, red); cpix = block_sum(cpix, red); basins = block_sum(basins, red);
        x0 = block_min_u64(x0, red); y0 = block_min_u64(y0, red); x1 = block_max_u64(x1, red); y1 = block_max_u64(y1, red);
        S = block_sum(S, redd); SX = block_sum(SX, redd); SY = block_sum(SY, redd);
        if (tid == 0) {
            const u64 pk = t.edges[j];
            const int pp = (int)(0xffffffffu - (uint32_t)pk), m = t.lab[pp];
            const int px = box.x0 + pp % bw, py = box.y0 + pp / bw;
            const double dm = (double)key2f((uint32_t)(pk >> 32));
            const u64 sd = t.sad[m];
            double *o = lobes + (size_t)j * VISTAF_NLOBE;
            o[VISTAF_LOBE_X] = (double)px;
            o[VISTAF_LOBE_Y] = (double)py;
            o[VISTAF_LOBE_DEPTH_MM] = dm;
            if (sd) {
                const int lo = LbTab::pass_lo(sd);
                const double dl = (double)key2f((uint32_t)(sd >> 32));
                o[VISTAF_LOBE_PROMINENCE_MM] = dm - dl;
                o[VISTAF_LOBE_SADDLE_X] = (double)(box.x0 + lo % bw);
                o[VISTAF_LOBE_SADDLE_Y] = (double)(box.y0 + lo / bw);
                o[VISTAF_LOBE_SADDLE_DEPTH_MM] = dl;
                o[VISTAF_LOBE_NEIGHBOUR] = (double)t.comp[t.into[m]];
            } else {
                o[VISTAF_LOBE_PROMINENCE_MM] = dm;
                o[VISTAF_LOBE_SADDLE_X] = nan64(); o[VISTAF_LOBE_SADDLE_Y] = nan64(); o[VISTAF_LOBE_SADDLE_DEPTH_MM] = nan64();
                o[VISTAF_LOBE_NEIGHBOUR] = -1.0;
            }
            o[VISTAF_LOBE_PIXELS] = (double)pix;
            o[VISTAF_LOBE_CONTACT_PIXELS] = (double)cpix;
            o[VISTAF_LOBE_AREA_MM2] = (double)cpix * s2;
            o[VISTAF_LOBE_VOLUME_CM3] = S * s2 / 1000.0;
            o[VISTAF_LOBE_CENTROID_X] = cpix ? SX / S : nan64();
            o[VISTAF_LOBE_CENTROID_Y] = cpix ? SY / S : nan64();
            o[VISTAF_LOBE_FORCE_SHARE_N] = all == 0.0 ? nan64() : force * S / all;
            o[VISTAF_LOBE_BASINS] = (double)basins;
            aux[j * LB_AUX + 0] = (u64)__double_as_longlong(S);
            aux[j * LB_AUX + 1] = (pk & 0xffffffff00000000ull) | (u64)(0xffffffffu - (uint32_t)((size_t)py * a.w + px));
            aux[j * LB_AUX + 2] = x0 | (y0 << 32);
            aux[j * LB_AUX + 3] = x1 | (y1 << 32);
        }
    }
    for (int i = L * VISTAF_NLOBE + tid; i < a.max_lobes * VISTAF_NLOBE; i += LB_NT) lobes[i] = nan64();

    if (tid == 0) {
        for (int j = 0; j < VISTAF_NLOBEROW; j++) row[j] = nan64();
        row[VISTAF_LOBEROW_PIXELS] = (double)npix;
        row[VISTAF_LOBEROW_RAW_MAXIMA] = (double)M;
        row[VISTAF_LOBEROW_PEAKS] = (double)peaks;
        row[VISTAF_LOBEROW_PEAKS_WRITTEN] = (double)L;
        row[VISTAF_LOBEROW_STATUS] = (double)(VISTAF_LOBEST_OK | (peaks > a.max_lobes ? VISTAF_LOBEST_TRUNCATED : 0));
        row[VISTAF_LOBEROW_THRESHOLD_MM] = tau;
        if (peaks >= 2) {
            const int p0 = (int)(0xffffffffu - (uint32_t)t.edges[0]), p1 = (int)(0xffffffffu - (uint32_t)t.edges[1]);
            const long long dx = p1 % bw - p0 % bw, dy = p1 / bw - p0 / bw;
            row[VISTAF_LOBEROW_SEPARATION_MM] = sqrt((double)(dx * dx + dy * dy)) * s;
        }
        if (deepest) row[VISTAF_LOBEROW_DEEPEST_SADDLE_MM] = (double)key2f((uint32_t)deepest);
        if (next) row[VISTAF_LOBEROW_NEXT_PROMINENCE_MM] = __longlong_as_double((long long)(next - 1ull));
    }
}

__global__ __launch_bounds__(LB_NT) void k_lobes_rows(LbArgs a)
{
    extern __shared__ u64 lb_lds[];
    const int b = blockIdx.x / a.K, k = blockIdx.x - b * a.K;
    double *row = a.rows + (size_t)blockIdx.x * VISTAF_NLOBEROW;
    double *lobes = a.lobes + (size_t)blockIdx.x * a.max_lobes * VISTAF_NLOBE;
    if (k >= clamp_count(a.count[b], a.K)) {
        if (threadIdx.x < VISTAF_NLOBEROW) row[threadIdx.x] = nan64();
        for (int i = threadIdx.x; i < a.max_lobes * VISTAF_NLOBE; i += LB_NT) lobes[i] = nan64();
        return;
    }
    const ContactBox box(a.contacts + (size_t)blockIdx.x * VISTAF_NCONTACT, a.h, a.w);
    if (!box.total()) { lb_empty_row(a, row, lobes); return; }
    if (lb_box_in_lds(box.bw, box.bh)) lb_row((uint8_t *)lb_lds, a, box, b, k);
    else lb_row(a.bf.rows + (size_t)blockIdx.x * a.bf.row_stride, a, box, b, k);
}

// One workgroup per frame: the written lobes of the rows in use, ranked by their peaks; the split table, its count and the parents
__global__ __launch_bounds__(LB_SPLIT_NT) void k_lobes_split(const double *__restrict__ lobes, const double *__restrict__ rows, const int32_t *__restrict__ count,
                                                       const double *__restrict__ mm_per_px, int K, int max_lobes, LobesBufs bf,
                                                       double *__restrict__ split, int32_t *__restrict__ split_count, int32_t *__restrict__ parent)
{
    __shared__ u64 keys[VISTAF_MAX_CONTACTS * LB_MAXL];
    __shared__ u64 red[16];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int kk = clamp_count(count[b], K), E = K * LB_MAXL;
    const u64 *aux = bf.aux + (size_t)b * K * LB_MAXL * LB_AUX;
    u64 mine = 0;
    for (int e = tid; e < E; e += LB_SPLIT_NT) {
        const int k = e / LB_MAXL, j = e - k * LB_MAXL;
        u64 key = 0;
        if (k < kk && j < max_lobes && j < (int)rows[((size_t)b * K + k) * VISTAF_NLOBEROW + VISTAF_LOBEROW_PEAKS_WRITTEN]) key = aux[(size_t)e * LB_AUX + 1];
        keys[e] = key;
        mine += key ? 1 : 0;
    }
    const int total = (int)block_sum(mine, red);
    __syncthreads();
    const int used = total < K ? total : K;
    for (int i = used * VISTAF_NCONTACT + tid; i < K * VISTAF_NCONTACT; i += LB_SPLIT_NT) split[(size_t)b * K * VISTAF_NCONTACT + i] = nan64();
    for (int i = used * 2 + tid; i < K * 2; i += LB_SPLIT_NT) parent[(size_t)b * K * 2 + i] = -1;
    if (tid == 0) split_count[b] = total;
    const double s = mm_per_px[b], s2 = s * s;
    for (int e = tid; e < E; e += LB_SPLIT_NT) {
        const u64 key = keys[e];
        int r = -1;
        if (key) {
            r = 0;
            for (int q = 0; q < E; q++) r += keys[q] > key ? 1 : 0;
        }
        bf.rank[(size_t)b * E + e] = r >= 0 && r < K ? r : -1;
        if (r < 0 || r >= K) continue;
        const int k = e / LB_MAXL, j = e - k * LB_MAXL;
        const double *lo = lobes + (((size_t)b * K + k) * max_lobes + j) * VISTAF_NLOBE;
        const u64 *ax = aux + (size_t)e * LB_AUX;
        double *o = split + ((size_t)b * K + r) * VISTAF_NCONTACT;
        const double cnt = lo[VISTAF_LOBE_CONTACT_PIXELS];
        o[VISTAF_CONTACT_PIXELS] = lo[VISTAF_LOBE_PIXELS];
        o[VISTAF_CONTACT_CONTACT_PIXELS] = cnt;
        o[VISTAF_CONTACT_AREA_MM2] = lo[VISTAF_LOBE_AREA_MM2];
        o[VISTAF_CONTACT_VOLUME_CM3] = cnt > 0 ? (double)(float)__longlong_as_double((long long)ax[0]) * s2 / 1000.0 : 0.0;
        o[VISTAF_CONTACT_MAX_DEPTH_MM] = lo[VISTAF_LOBE_DEPTH_MM];
        o[VISTAF_CONTACT_ARGMAX_INDEX] = (double)(0xffffffffu - (uint32_t)key);
        o[VISTAF_CONTACT_CENTROID_X] = lo[VISTAF_LOBE_CENTROID_X];
        o[VISTAF_CONTACT_CENTROID_Y] = lo[VISTAF_LOBE_CENTROID_Y];
        o[VISTAF_CONTACT_FORCE_N] = lo[VISTAF_LOBE_FORCE_SHARE_N];
        o[VISTAF_CONTACT_BBOX_X0] = (double)(uint32_t)ax[2];
        o[VISTAF_CONTACT_BBOX_Y0] = (double)(uint32_t)(ax[2] >> 32);
        o[VISTAF_CONTACT_BBOX_X1] = (double)(uint32_t)ax[3];
        o[VISTAF_CONTACT_BBOX_Y1] = (double)(uint32_t)(ax[3] >> 32);
        for (int f = VISTAF_CONTACT_BBOX_Y1 + 1; f < VISTAF_NCONTACT; f++) o[f] = nan64();
        parent[((size_t)b * K + r) * 2] = k;
        parent[((size_t)b * K + r) * 2 + 1] = j;
    }
}

__global__ __launch_bounds__(256) void k_lobes_plane(const int8_t *__restrict__ index, const int8_t *__restrict__ plane, const int32_t *__restrict__ count,
                                                     const int32_t *__restrict__ rank, int K, size_t P, size_t n, int8_t *__restrict__ split_index)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const size_t b = i / P;
        const int k = index[i], l = plane[i];
        int r = -1;
        if (k >= 0 && k < clamp_count(count[b], K) && l >= 0 && l < LB_MAXL) r = rank[(b * K + k) * LB_MAXL + l];
        split_index[i] = (int8_t)r;
    }
}

}  // namespace

static bool lobes_finite_nonneg(double v) { return v >= 0.0 && v <= 1.7976931348623157e308; }

extern "C" {

int vistaf_ftp_test_lobes_tier(int bw, int bh) { return tier_hook_answer(bw, bh, lb_box_in_lds); }

int vistaf_lobes_workspace_bytes(int h, int w, int batch, int max_contacts, size_t *bytes)
{
    return workspace_bytes_answer(bytes, plane_sizes_refusal(h, w, batch, max_contacts), [&] { return lobes_scratch_bytes(batch, h, w, max_contacts); });
}

int vistaf_lobes_measure(const int8_t *d_contact_index, const double *d_contacts, const int32_t *d_count, const double *d_mm_per_px,
                         const float *d_depth_mm, int batch, int h, int w, int max_contacts, int max_lobes, double min_prominence_mm,
                         double min_prominence_frac, double depth_eps_mm, double *d_lobes, double *d_rows, int8_t *d_lobe_index,
                         double *d_split_contacts, int32_t *d_split_count, int8_t *d_split_index, int32_t *d_split_parent, void *d_workspace,
                         size_t workspace_bytes, void *stream)
{
    if (const char *why = table_inputs_refusal(d_contact_index, d_contacts, d_count, d_mm_per_px)) return set_error(VISTAF_E_INVALID, why);
    if (!d_depth_mm) return set_error(VISTAF_E_INVALID, "d_depth_mm is null");
    if (!d_lobes) return set_error(VISTAF_E_INVALID, "d_lobes is null");
    if (!d_rows) return set_error(VISTAF_E_INVALID, "d_rows is null");
    if (const char *why = plane_sizes_refusal(h, w, batch, max_contacts)) return set_error(VISTAF_E_INVALID, why);
    if (max_lobes < 1 || max_lobes > VISTAF_LOBES_MAX) return set_error(VISTAF_E_INVALID, "max_lobes must be 1..64");
    if (!lobes_finite_nonneg(min_prominence_mm)) return set_error(VISTAF_E_INVALID, "min_prominence_mm must be finite and >= 0");
    if (!lobes_finite_nonneg(min_prominence_frac)) return set_error(VISTAF_E_INVALID, "min_prominence_frac must be finite and >= 0");
    if (!lobes_finite_nonneg(depth_eps_mm)) return set_error(VISTAF_E_INVALID, "depth_eps_mm must be finite and >= 0");
    const int nsplit = (d_split_contacts ? 1 : 0) + (d_split_count ? 1 : 0) + (d_split_index ? 1 : 0) + (d_split_parent ? 1 : 0);
    if (nsplit != 0 && nsplit != 4)
        return set_error(VISTAF_E_INVALID, "d_split_contacts, d_split_count, d_split_index and d_split_parent must be all null or all given");
    if (((uintptr_t)d_contacts | (uintptr_t)d_mm_per_px | (uintptr_t)d_lobes | (uintptr_t)d_rows | (uintptr_t)d_split_contacts) & 7)
        return set_error(VISTAF_E_INVALID, "d_contacts, d_mm_per_px, d_lobes, d_rows and d_split_contacts must be 8-byte aligned");
    if (((uintptr_t)d_count | (uintptr_t)d_depth_mm | (uintptr_t)d_split_count | (uintptr_t)d_split_parent) & 3)
        return set_error(VISTAF_E_INVALID, "d_count, d_depth_mm, d_split_count and d_split_parent must be 4-byte aligned");
    TRY(workspace_ok(d_workspace, workspace_bytes, lobes_scratch_bytes(batch, h, w, max_contacts), "vistaf_lobes_workspace_bytes"));
    ScratchLayout L(d_workspace);
    LbArgs a;
    a.index = d_contact_index; a.contacts = d_contacts; a.count = d_count; a.mm_per_px = d_mm_per_px; a.depth = d_depth_mm;
    a.h = h; a.w = w; a.K = max_contacts; a.max_lobes = max_lobes;
    a.min_mm = min_prominence_mm; a.min_frac = min_prominence_frac; a.eps = (float)depth_eps_mm;
    a.lobes = d_lobes; a.rows = d_rows;
    a.bf = lobes_scratch(L, batch, h, w, max_contacts);
    a.plane = d_lobe_index ? d_lobe_index : a.bf.plane;
    const dim3 grid((unsigned)(batch * max_contacts));
    hipStream_t st = (hipStream_t)stream;
    const size_t P = (size_t)h * w, n = (size_t)batch * P;
    launch_fill_i8<-1>(a.plane, n, st);
    hipLaunchKernelGGL(k_lobes_rows, grid, dim3(LB_NT), lb_launch_lds(h, w), st, a);
    if (d_split_contacts) {
        hipLaunchKernelGGL(k_lobes_split, dim3((unsigned)batch), dim3(LB_SPLIT_NT), 0, st, d_lobes, d_rows, d_count, d_mm_per_px, max_contacts, max_lobes, a.bf,
                           d_split_contacts, d_split_count, d_split_parent);
        hipLaunchKernelGGL(k_lobes_plane, fill_grid(n), dim3(256), 0, st, d_contact_index, (const int8_t *)a.plane, d_count, (const int32_t *)a.bf.rank,
                           max_contacts, P, n, d_split_index);
    }
    return launch_ok("k_lobes");
}

}  // extern "C"
