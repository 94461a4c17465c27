// Centreline read-out (include_ext/vistaf_centreline.h): skeleton, axis path, length, width profile, end tangents and bend of every contact, from
// the int8 index plane, table and counts vistaf_ftp_contacts wrote.  An extension, as the other per-contact read-outs: the reference has no
// counterpart.  The definition is in the header; tests/centreline_helpers.py restates it in NumPy.
//
// One workgroup of 256 threads per (frame, row); the row's clipped box is held as bit planes of 64-bit row words, (bh + 2) rows of
// W64 = ceil(bw / 64) words with a zero row above and below, seven planes: the mask M, two skeleton buffers, two frontier buffers and two
// planes that hold a walk's hop count modulo 4.  A box whose planes fit CL_LDS_BUDGET works in LDS; a larger one runs the same code over
// planes in the caller's workspace (cl_box_in_lds; test_hooks_centreline.h tells the tiers apart).
//   k_fill_i8<-1>      (only with d_skeleton; contact_rows.hpp) writes -1 over the skeleton plane.
//   k_centreline_rows  packs M with wave ballots; thins it (Guo-Hall, the two conditions and the small sums bit-sliced on 64 pixels per word,
//                      the buffers swapped after each sub-iteration, one workgroup barrier-with-OR per sub-iteration); counts skeleton, end and
//                      branch pixels bit-sliced; finds the seed by a max-reduction over D2, which is not a plane here: D2 of one pixel is
//                      the minimum over the rows around it of dy^2 + (distance to the row's nearest zero bit)^2, probed outward until dy^2
//                      reaches the best so far -- exact, O(local radius) rows, needed for skeleton pixels only; walks twice with a bit-plane
//                      frontier (dilate 3 x 3, AND skeleton, AND NOT visited), the second walk recording the hop count modulo 4 (neighbours
//                      differ by at most one hop, so modulo 4 tells "one less"); lane 0 then steps the path back, leaving the link to the
//                      predecessor in three freed planes when the listed order is the reverse of the stepping order; the stations go through
//                      LDS in chunks of 256: lane 0 lists them, every thread finds the D2 and depth of one, lane 0 folds the chunk into the
//                      running measures in station order.  With polyline pointers every pixel of the row gets its station number (or -1)
//                      and D2 in two frame-sized int32 planes of the workspace: the rows of a frame own disjoint pixels.
//   k_centreline_poly  (only with polyline pointers) applies the capacity rule over the rows' STATIONS and scatters each written row's pixels
//                      to their station slots.
// No memset, no float atomics, no host read-back: every double is computed once by one thread from exact integers, s and depth samples.
#include <string>

#include "../../include_ext/vistaf_centreline.h"
#include "contact_rows.hpp"
#include "host_util.hpp"
#include "mask_bits.hpp"
#include "test_hooks_centreline.h"

using namespace vf;

namespace {

typedef unsigned long long u64;

constexpr int CL_NT = 256, CL_PLANES = 7;
// The LDS a row's planes may take (contact_rows.hpp): it holds a box of a whole 224 x 224 frame (226 rows x 4 words x 8 bytes x 7 planes =
// 50,624 bytes), where three workgroups share a CU.
constexpr int CL_LDS_BUDGET = ROW_LDS_BUDGET;
constexpr int CL_NONE = -1;

// ---- pure rules -----------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline size_t cl_plane_words(int bw, int bh) { return (size_t)(bh + 2) * mb_w64(bw); }
__host__ __device__ inline size_t cl_planes_bytes(int bw, int bh) { return cl_plane_words(bw, bh) * CL_PLANES * 8; }
__host__ __device__ inline bool cl_box_in_lds(int bw, int bh) { return cl_planes_bytes(bw, bh) <= (size_t)CL_LDS_BUDGET; }
// the dynamic LDS of a launch over h x w frames: what the largest box that can take the LDS tier needs, never more than the budget
inline size_t cl_launch_lds(int h, int w) { return cl_box_in_lds(w, h) ? cl_planes_bytes(w, h) : (size_t)CL_LDS_BUDGET; }

// The workspace.  Per frame: the station number and D2 of every pixel (written on the pixels of the rows in use only, read on the same).  Per
// (frame, row): seven planes sized for a box of the whole frame, unless every box of such a frame takes the LDS tier.
struct CentrelineBufs {
    int32_t *stn, *d2;
    u64 *planes;
    size_t row_words;       // words of one row's seven planes (0: no box leaves LDS)
};

CentrelineBufs centreline_scratch(ScratchLayout &L, int B, int h, int w, int K)
{
    const size_t P = (size_t)h * w;
    CentrelineBufs bf;
    bf.stn = L.take<int32_t>((size_t)B * P, 256, "station_of_pixel");
    bf.d2 = L.take<int32_t>((size_t)B * P, 256, "d2_of_pixel");
    bf.row_words = cl_box_in_lds(w, h) ? 0 : cl_plane_words(w, h) * CL_PLANES;
    bf.planes = L.take<u64>((size_t)B * K * bf.row_words, 256, "row_planes");
    return bf;
}

size_t centreline_scratch_bytes(int B, int h, int w, int K, ScratchRec *rec = nullptr)
{
    return scratch_bytes([&](ScratchLayout &L) { return centreline_scratch(L, B, h, w, K); }, rec);
}

struct ClArgs {
    const int8_t *index;
    const double *contacts;
    const int32_t *count;
    const double *mm_per_px;
    const float *depth;
    int h, w, K, span, polylines;
    double *out;
    int8_t *skeleton;
    CentrelineBufs bf;
};

// the walk's neighbour order (header, step 4): N, E, S, W, NE, SE, SW, NW; the opposite of step d is cl_back(d); step 8 stays in place
__device__ __forceinline__ int cl_dx(int d) { return d == 1 || d == 4 || d == 5 ? 1 : (d == 3 || d == 6 || d == 7 ? -1 : 0); }
__device__ __forceinline__ int cl_dy(int d) { return d == 2 || d == 5 || d == 6 ? 1 : (d == 0 || d == 4 || d == 7 ? -1 : 0); }
__device__ __forceinline__ int cl_back(int d) { return d < 4 ? (d + 2) & 3 : 4 + ((d + 2) & 3); }

// The geometry of a row's planes and the word-level steps on them.  r is the box row, 0..bh-1; plane row r + 1.
struct ClGeom {
    int bw, bh, W64, nw;            // nw: the words of the box rows, bh * W64
    size_t pw;                      // words of a plane with its two guard rows
    __device__ inline ClGeom(int bw_, int bh_) : bw(bw_), bh(bh_), W64(mb_w64(bw_)), nw(bh_ * mb_w64(bw_)), pw(cl_plane_words(bw_, bh_)) {}
    __device__ inline size_t at(int t) const { return (size_t)t + W64; }           // word t of the box rows, row-major
    __device__ inline bool bit(const u64 *pl, int x, int y) const { return (pl[(size_t)(y + 1) * W64 + (x >> 6)] >> (x & 63)) & 1ull; }
};

// the eight neighbour planes of word (r, j) of S, header order P2..P9 at [0..7], and the word itself
template <typename PL>
__device__ __forceinline__ u64 cl_neighbours(PL S, const ClGeom &g, int r, int j, u64 P[8])
{
    const size_t c = (size_t)(r + 1) * g.W64 + j, u = c - g.W64, d = c + g.W64;
    const bool hl = j > 0, hr = j < g.W64 - 1;
    const u64 cc = S[c], cl = hl ? S[c - 1] : 0ull, cr = hr ? S[c + 1] : 0ull;
    const u64 uc = S[u], ul = hl ? S[u - 1] : 0ull, ur = hr ? S[u + 1] : 0ull;
    const u64 dc = S[d], dl = hl ? S[d - 1] : 0ull, dr = hr ? S[d + 1] : 0ull;
    P[0] = uc;                                   // N
    P[1] = (uc >> 1) | (ur << 63);               // NE: the pixel at x + 1 of the row above
    P[2] = (cc >> 1) | (cr << 63);               // E
    P[3] = (dc >> 1) | (dr << 63);               // SE
    P[4] = dc;                                   // S
    P[5] = (dc << 1) | (dl >> 63);               // SW
    P[6] = (cc << 1) | (cl >> 63);               // W
    P[7] = (uc << 1) | (ul >> 63);               // NW
    return cc;
}

// of four bit planes: at least two set, all four set, exactly one set
__device__ __forceinline__ u64 cl_ge2(u64 q1, u64 q2, u64 q3, u64 q4) { return (q1 & q2) | (q3 & q4) | ((q1 ^ q2) & (q3 ^ q4)); }
__device__ __forceinline__ u64 cl_all4(u64 q1, u64 q2, u64 q3, u64 q4) { return q1 & q2 & q3 & q4; }
__device__ __forceinline__ u64 cl_one(u64 q1, u64 q2, u64 q3, u64 q4) { return ((q1 ^ q2) ^ (q3 ^ q4)) & ~(q1 & q2) & ~(q3 & q4); }

// the pixels of word (r, j) a Guo-Hall sub-iteration deletes (header, step 3); it = 0 / 1
template <typename PL>
__device__ __forceinline__ u64 cl_thin_deletes(PL S, const ClGeom &g, int r, int j, int it, u64 &cc)
{
    u64 P[8];
    cc = cl_neighbours(S, g, r, j, P);
    if (!cc) return 0ull;
    const u64 P2 = P[0], P3 = P[1], P4 = P[2], P5 = P[3], P6 = P[4], P7 = P[5], P8 = P[6], P9 = P[7];
    const u64 c1 = cl_one(~P2 & (P3 | P4), ~P4 & (P5 | P6), ~P6 & (P7 | P8), ~P8 & (P9 | P2));
    const u64 a1 = P9 | P2, a2 = P3 | P4, a3 = P5 | P6, a4 = P7 | P8, b1 = P2 | P3, b2 = P4 | P5, b3 = P6 | P7, b4 = P8 | P9;
    // 2 <= min(N1, N2) <= 3: both at least 2 and not both 4
    const u64 n23 = cl_ge2(a1, a2, a3, a4) & cl_ge2(b1, b2, b3, b4) & ~(cl_all4(a1, a2, a3, a4) & cl_all4(b1, b2, b3, b4));
    const u64 m = it == 0 ? (P2 | P3 | ~P5) & P4 : (P6 | P7 | ~P9) & P8;
    return cc & c1 & n23 & ~m;
}

// the distance from column x of a mask row to its nearest zero column; columns -1 and bw are zero (bits from bw on are zero in M)
template <typename PL>
__device__ __forceinline__ int cl_zero_dist(PL row, int W64, int bw, int x)
{
    const int j = x >> 6, bit = x & 63;
    int dr = bw - x, dl = x + 1;
    u64 z = ~row[j] >> bit;
    if (z) dr = __ffsll((long long)z) - 1;
    else
        for (int q = j + 1; q < W64; q++) {
            z = ~row[q];
            if (z) { dr = q * 64 + __ffsll((long long)z) - 1 - x; break; }
        }
    z = ~row[j] << (63 - bit);
    if (z) dl = __clzll((long long)z);
    else
        for (int q = j - 1; q >= 0; q--) {
            z = ~row[q];
            if (z) { dl = x - (q * 64 + 63 - __clzll((long long)z)); break; }
        }
    return dl < dr ? dl : dr;
}

// D2 of box pixel (x, y) (header, step 2): rows outside the box are zero everywhere
template <typename PL>
__device__ __forceinline__ int cl_d2(PL M, const ClGeom &g, int x, int y)
{
    uint32_t best = 0xffffffffu;
    for (int dy = 0;; dy++) {
        const uint32_t dy2 = (uint32_t)dy * (uint32_t)dy;
        if (dy2 >= best) break;
        for (int side = 0; side < (dy ? 2 : 1); side++) {
            const int r = side ? y + dy : y - dy;
            const uint32_t dx = r < 0 || r >= g.bh ? 0u : (uint32_t)cl_zero_dist(M + (size_t)(r + 1) * g.W64, g.W64, g.bw, x);
            const uint32_t cand = dy2 + dx * dx;
            best = cand < best ? cand : best;
        }
    }
    return (int)best;
}

// One walk over S from (sx, sy) with a bit-plane frontier: V the visited pixels on return; with RECORD the hop count modulo 4 of every visited
// pixel in L0 (bit 0) and L1 (bit 1).  Returns the hops of the farthest pixels and the first of them in (fx, fy).  Every thread calls it.
template <bool RECORD, typename PL>
__device__ __forceinline__ int cl_walk(PL S, PL V, PL F, PL Fn, PL L0, PL L1, const ClGeom &g, int sx, int sy, int &fx, int &fy, u64 *red)
{
    const int tid = threadIdx.x;
    for (int t = tid; t < g.nw; t += CL_NT) {
        const size_t i = g.at(t);
        V[i] = 0ull; F[i] = 0ull; Fn[i] = 0ull;
        if (RECORD) { L0[i] = 0ull; L1[i] = 0ull; }
    }
    block_any_fenced(false);
    if (tid == 0) {
        const size_t i = (size_t)(sy + 1) * g.W64 + (sx >> 6);
        F[i] = 1ull << (sx & 63);
        V[i] = 1ull << (sx & 63);
    }
    block_any_fenced(false);
    int lev = 0;
    for (;;) {
        bool any = false;
        for (int t = tid; t < g.nw; t += CL_NT) {
            const int r = t / g.W64, j = t - r * g.W64;
            const size_t i = g.at(t);
            const u64 s = S[i];
            u64 nf = 0ull;
            if (s) {
                u64 P[8];
                const u64 cc = cl_neighbours(F, g, r, j, P);
                nf = (cc | P[0] | P[1] | P[2] | P[3] | P[4] | P[5] | P[6] | P[7]) & s & ~V[i];
            }
            Fn[i] = nf;
            if (nf) {
                V[i] |= nf;
                if (RECORD) {
                    if ((lev + 1) & 1) L0[i] |= nf;
                    if ((lev + 1) & 2) L1[i] |= nf;
                }
                any = true;
            }
        }
        if (!block_any_fenced(any)) break;
        PL tmp = F; F = Fn; Fn = tmp;
        lev++;
    }
    u64 first = ~0ull;                                        // the first pixel of the last frontier: words are in (y, x) order
    for (int t = tid; t < g.nw; t += CL_NT) {
        const u64 f = F[g.at(t)];
        if (f) { first = ((u64)t << 6) | (u64)(__ffsll((long long)f) - 1); break; }
    }
    first = block_min_u64(first, red);
    const int t = (int)(first >> 6);
    fy = t / g.W64;
    fx = (t - fy * g.W64) * 64 + (int)(first & 63);
    return lev;
}

// the step from (x, y), whose hop count is `lev`, to the first neighbour one hop nearer (header, step 4)
template <typename PL>
__device__ __forceinline__ int cl_step_back(PL V, PL L0, PL L1, const ClGeom &g, int x, int y, int lev)
{
    const int want = (lev - 1) & 3;
    for (int d = 0; d < 8; d++) {
        const int u = x + cl_dx(d), v = y + cl_dy(d);
        if (u < 0 || u >= g.bw || v < 0 || v >= g.bh) continue;
        if (g.bit(V, u, v) && ((int)g.bit(L0, u, v) | ((int)g.bit(L1, u, v) << 1)) == want) return d;
    }
    return 8;       // not reached: every pixel at hop lev > 0 has a neighbour at hop lev - 1.  Step 8 stays in place
}

template <typename PL>
__device__ __forceinline__ void cl_set_link(PL K0, PL K1, PL K2, const ClGeom &g, int x, int y, int d)
{
    const size_t i = (size_t)(y + 1) * g.W64 + (x >> 6);
    const u64 m = 1ull << (x & 63);
    K0[i] = (K0[i] & ~m) | ((d & 1) ? m : 0ull);
    K1[i] = (K1[i] & ~m) | ((d & 2) ? m : 0ull);
    K2[i] = (K2[i] & ~m) | ((d & 4) ? m : 0ull);
}

// The body of k_centreline_rows for a row with a box: pl holds the seven planes, in LDS or in the workspace
template <typename PL>
__device__ __forceinline__ void cl_row(PL pl, const ClArgs &a, const ContactBox &box, int b, int k)
{
    __shared__ u64 red[16];
    __shared__ int c_xy[CL_NT], c_d2[CL_NT];
    __shared__ float c_z[CL_NT];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const ClGeom g(box.bw, box.bh);
    const size_t P = (size_t)a.h * a.w;
    const int8_t *index = a.index + b * P;
    double *out = a.out + ((size_t)b * a.K + k) * VISTAF_NCENTRELINE;
    PL M = pl, Sa = pl + g.pw, Sb = pl + 2 * g.pw, F0 = pl + 3 * g.pw, F1 = pl + 4 * g.pw, L0 = pl + 5 * g.pw, L1 = pl + 6 * g.pw;

    // ---- the guard rows of every plane, and M packed from the index plane: a wave takes four words at a time, their loads in flight together
    for (int t = tid; t < CL_PLANES * 2 * g.W64; t += CL_NT) {
        const int p = t / (2 * g.W64), q = t - p * 2 * g.W64;
        pl[p * g.pw + (q < g.W64 ? (size_t)q : (size_t)(g.bh + 1) * g.W64 + (q - g.W64))] = 0ull;
    }
    unsigned long long npix = 0;
    for (int t0 = wid * 4; t0 < g.nw; t0 += (CL_NT / 64) * 4) {
        bool v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int t = t0 + u, r = t / g.W64, x = (t - r * g.W64) * 64 + lane;
            v[u] = t < g.nw && x < g.bw && index[(size_t)(box.y0 + r) * a.w + box.x0 + x] == k;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const u64 word = __ballot(v[u]);
            if (lane == 0 && t0 + u < g.nw) {
                M[g.at(t0 + u)] = word;
                Sa[g.at(t0 + u)] = word;
                npix += __popcll(word);
            }
        }
    }
    npix = block_sum(npix, red);            // its barriers order the LDS planes; the workspace planes are fenced by the block_any_fenced below
    if (npix == 0) {
        empty_row(out, VISTAF_NCENTRELINE, VISTAF_CENTRELINE_STATUS, VISTAF_CLST_NO_PIXELS);
        return;
    }
    block_any_fenced(false);

    // ---- thinning: every sub-iteration reads one buffer and writes the other; a pair leaves S in Sa again
    int passes = 0;
    for (;;) {
        int pair = 0;
        for (int it = 0; it < 2; it++) {
            PL src = it ? Sb : Sa, dst = it ? Sa : Sb;
            bool any = false;
            for (int t = tid; t < g.nw; t += CL_NT) {
                const int r = t / g.W64, j = t - r * g.W64;
                u64 cc;
                const u64 del = cl_thin_deletes(src, g, r, j, it, cc);
                dst[g.at(t)] = cc & ~del;
                any = any || del != 0ull;
            }
            pair |= block_any_fenced(any);
        }
        if (!pair) break;
        passes++;
    }

    // ---- the skeleton's counts, the skeleton plane, the seed; with polylines every pixel of the row starts without a station
    unsigned long long nskel = 0, nend = 0, nbranch = 0, seed = 0;
    for (int t = tid; t < g.nw; t += CL_NT) {
        const int r = t / g.W64, j = t - r * g.W64;
        if (a.polylines)
            for (u64 m = M[g.at(t)]; m; m &= m - 1)
                a.bf.stn[b * P + (size_t)(box.y0 + r) * a.w + box.x0 + j * 64 + __ffsll((long long)m) - 1] = CL_NONE;
        u64 N[8];
        const u64 cc = cl_neighbours(Sa, g, r, j, N);
        if (!cc) continue;
        u64 ones = 0, twos = 0, fours = 0, eights = 0, t1 = 0, t2 = 0, t4 = 0, t8 = 0;         // bit-sliced counters of neighbours and of 0 -> 1 transitions
#pragma unroll
        for (int q = 0; q < 8; q++) {
            u64 x = N[q], c = ones & x;
            ones ^= x; x = twos & c; twos ^= c; c = fours & x; fours ^= x; eights |= c;
            x = ~N[q] & N[(q + 1) & 7]; c = t1 & x;
            t1 ^= x; x = t2 & c; t2 ^= c; c = t4 & x; t4 ^= x; t8 |= c;
        }
        nskel += __popcll(cc);
        nend += __popcll(cc & ones & ~twos & ~fours & ~eights);
        nbranch += __popcll(cc & ((t1 & t2) | t4 | t8));
        for (u64 m = cc; m; m &= m - 1) {
            const int x = j * 64 + __ffsll((long long)m) - 1;
            if (a.skeleton) a.skeleton[b * P + (size_t)(box.y0 + r) * a.w + box.x0 + x] = (int8_t)k;
            const u64 key = ((u64)(uint32_t)cl_d2(M, g, x, r) << 32) | (0xffffffffu - (uint32_t)(r * g.bw + x));
            seed = key > seed ? key : seed;
        }
    }
    nskel = block_sum(nskel, red);
    nend = block_sum(nend, red);
    nbranch = block_sum(nbranch, red);
    seed = block_max_u64(seed, red);
    if (nskel == 0) {                                          // Guo-Hall empties no mask; were it to, the row reads as one without pixels
        empty_row(out, VISTAF_NCENTRELINE, VISTAF_CENTRELINE_STATUS, VISTAF_CLST_NO_PIXELS);
        return;
    }
    const int seed_d2 = (int)(seed >> 32), seed_p = (int)(0xffffffffu - (uint32_t)seed), seed_y = seed_p / g.bw, seed_x = seed_p - seed_y * g.bw;

    // ---- the two walks: seed -> A0, A0 -> B0 with the hop counts
    int ax, ay, bx, by;
    cl_walk<false>(Sa, Sb, F0, F1, L0, L1, g, seed_x, seed_y, ax, ay, red);
    const int n = cl_walk<true>(Sa, Sb, F0, F1, L0, L1, g, ax, ay, bx, by, red) + 1;
    PL V = Sb, K0 = F0, K1 = F1, K2 = Sa;                      // S and the frontiers are spent: their planes take the links
    const bool a_is_a0 = ay < by || (ay == by && ax < bx);     // the listed order runs from A0: the reverse of the stepping order (n == 1: either)

    // ---- lane 0 steps from B0 back to A0 and leaves at every pixel the step to the one it came from
    if (tid == 0 && a_is_a0) {
        int x = bx, y = by;
        for (int lev = n - 1; lev > 0; lev--) {
            const int d = cl_step_back(V, L0, L1, g, x, y, lev);
            x += cl_dx(d); y += cl_dy(d);
            cl_set_link(K0, K1, K2, g, x, y, cl_back(d));
        }
    }
    block_any_fenced(false);

    // ---- the stations in listed order, in chunks: lane 0 lists, every thread measures one, lane 0 folds
    const int Ax = a_is_a0 ? ax : bx, Ay = a_is_a0 ? ay : by, Bx = a_is_a0 ? bx : ax, By = a_is_a0 ? by : ay;     // box coordinates
    const int span = a.span, jt = n - 1 < span ? n - 1 : span, ends = n < span + 1 ? n : span + 1;
    const float *depth = a.depth ? a.depth + b * P : nullptr;
    int cx = Ax, cy = Ay, px = Ax, py = Ay;                     // lane 0: the station to list next, the one folded last
    int axial = 0, diag = 0, sag_at = 0, interior = 0, wmin_at = 0, wmax_at = 0, peak_at = 0, d2A = 0, d2B = 0, jax = Ax, jay = Ay, jbx = Bx, jby = By;
    long long sag = 0;
    double wsum = 0.0, wmin = 0.0, wmax = 0.0, zsum = 0.0, zA = 0.0, zB = 0.0, peak = 0.0;
    const double s = a.mm_per_px[b];
    for (int base = 0; base < n; base += CL_NT) {
        const int cnt = n - base < CL_NT ? n - base : CL_NT;
        if (tid == 0)
            for (int i = 0; i < cnt; i++) {
                c_xy[i] = cx | (cy << 16);
                if (base + i == n - 1) break;
                const int d = a_is_a0 ? ((int)g.bit(K0, cx, cy) | ((int)g.bit(K1, cx, cy) << 1) | ((int)g.bit(K2, cx, cy) << 2))
                                      : cl_step_back(V, L0, L1, g, cx, cy, n - 1 - (base + i));
                const int nx = cx + cl_dx(d), ny = cy + cl_dy(d);
                if (nx >= 0 && nx < g.bw && ny >= 0 && ny < g.bh) { cx = nx; cy = ny; }          // a path never leaves the box
            }
        __syncthreads();
        if (tid < cnt) {
            const int x = c_xy[tid] & 0xffff, y = c_xy[tid] >> 16;
            const size_t p = (size_t)(box.y0 + y) * a.w + box.x0 + x;
            const int d2 = cl_d2(M, g, x, y);
            c_d2[tid] = d2;
            c_z[tid] = depth ? depth[p] : 0.f;
            if (a.polylines) { a.bf.stn[b * P + p] = base + tid; a.bf.d2[b * P + p] = d2; }
        }
        __syncthreads();
        if (tid == 0)
            for (int q = 0; q < cnt; q++) {
                const int i = base + q, x = c_xy[q] & 0xffff, y = c_xy[q] >> 16, d2 = c_d2[q];
                if (i == 0) d2A = d2;
                if (i == n - 1) d2B = d2;
                if (i > 0) { if (x != px && y != py) diag++; else axial++; }
                px = x; py = y;
                const long long c = (long long)(Bx - Ax) * (y - Ay) - (long long)(By - Ay) * (x - Ax);
                if ((c < 0 ? -c : c) > (sag < 0 ? -sag : sag)) { sag = c; sag_at = i; }
                const long long ra = (long long)(x - Ax) * (x - Ax) + (long long)(y - Ay) * (y - Ay), rb = (long long)(x - Bx) * (x - Bx) + (long long)(y - By) * (y - By);
                if (ra >= 4ll * d2 && rb >= 4ll * d2) {
                    const double wd = (2.0 * sqrt((double)d2) - 1.0) * s;
                    wsum = interior ? wsum + wd : wd;
                    if (!interior || wd < wmin) { wmin = wd; wmin_at = i; }
                    if (!interior || wd > wmax) { wmax = wd; wmax_at = i; }
                    interior++;
                }
                if (i == jt) { jax = x; jay = y; }
                if (i == n - 1 - jt) { jbx = x; jby = y; }
                if (depth) {
                    const double z = (double)c_z[q];
                    zsum = i ? zsum + z : z;
                    if (i < ends) zA = i ? zA + z : z;
                    if (i >= n - ends) zB = i > n - ends ? zB + z : z;
                    if (i == 0 || z > peak) { peak = z; peak_at = i; }
                }
            }
    }

    if (tid == 0) {
        for (int j = 0; j < VISTAF_NCENTRELINE; j++) out[j] = nan64();
        const int fAx = box.x0 + Ax, fAy = box.y0 + Ay, fBx = box.x0 + Bx, fBy = box.y0 + By;
        const long long chord2 = (long long)(Bx - Ax) * (Bx - Ax) + (long long)(By - Ay) * (By - Ay);
        const double core = (double)axial + (double)diag * sqrt(2.0);
        out[VISTAF_CENTRELINE_PIXELS] = (double)npix;
        out[VISTAF_CENTRELINE_SKELETON_PIXELS] = (double)nskel;
        out[VISTAF_CENTRELINE_THINNING_PASSES] = (double)passes;
        out[VISTAF_CENTRELINE_END_PIXELS] = (double)nend;
        out[VISTAF_CENTRELINE_BRANCH_PIXELS] = (double)nbranch;
        out[VISTAF_CENTRELINE_STATIONS] = (double)n;
        out[VISTAF_CENTRELINE_STATIONS_WRITTEN] = 0.0;          // k_centreline_poly writes what it writes
        out[VISTAF_CENTRELINE_STATUS] = (double)((n == 1 ? VISTAF_CLST_POINT : VISTAF_CLST_OK) | (nbranch ? VISTAF_CLST_BRANCHED : 0) | VISTAF_CLST_TRUNCATED);
        out[VISTAF_CENTRELINE_A_X] = (double)fAx;
        out[VISTAF_CENTRELINE_A_Y] = (double)fAy;
        out[VISTAF_CENTRELINE_B_X] = (double)fBx;
        out[VISTAF_CENTRELINE_B_Y] = (double)fBy;
        const double path_mm = core * s, length_mm = (((core + sqrt((double)d2A)) + sqrt((double)d2B)) - 1.0) * s, chord_mm = sqrt((double)chord2) * s;
        out[VISTAF_CENTRELINE_PATH_LENGTH_MM] = path_mm;
        out[VISTAF_CENTRELINE_LENGTH_MM] = length_mm;
        out[VISTAF_CENTRELINE_CHORD_MM] = chord_mm;
        out[VISTAF_CENTRELINE_SAGITTA_STATION] = (double)sag_at;
        out[VISTAF_CENTRELINE_INTERIOR_STATIONS] = (double)interior;
        if (interior) {
            out[VISTAF_CENTRELINE_WIDTH_MEAN_MM] = wsum / (double)interior;
            out[VISTAF_CENTRELINE_WIDTH_MIN_MM] = wmin;
            out[VISTAF_CENTRELINE_WIDTH_MIN_STATION] = (double)wmin_at;
            out[VISTAF_CENTRELINE_WIDTH_MAX_MM] = wmax;
            out[VISTAF_CENTRELINE_WIDTH_MAX_STATION] = (double)wmax_at;
        }
        const double seed_mm = (2.0 * sqrt((double)seed_d2) - 1.0) * s;
        out[VISTAF_CENTRELINE_WIDTH_SEED_MM] = seed_mm;
        out[VISTAF_CENTRELINE_ELONGATION] = length_mm / seed_mm;
        if (n >= 2) {
            out[VISTAF_CENTRELINE_TORTUOSITY] = path_mm / chord_mm;
            out[VISTAF_CENTRELINE_SAGITTA_MM] = (double)sag / sqrt((double)chord2) * s;
            const double ra = sqrt((double)((long long)(jax - Ax) * (jax - Ax) + (long long)(jay - Ay) * (jay - Ay)));
            const double rb = sqrt((double)((long long)(jbx - Bx) * (jbx - Bx) + (long long)(jby - By) * (jby - By)));
            out[VISTAF_CENTRELINE_A_TX] = (double)(jax - Ax) / ra;
            out[VISTAF_CENTRELINE_A_TY] = (double)(jay - Ay) / ra;
            out[VISTAF_CENTRELINE_B_TX] = (double)(jbx - Bx) / rb;
            out[VISTAF_CENTRELINE_B_TY] = (double)(jby - By) / rb;
        }
        auto reach = [&](int x, int y) {
            int m = x + 1 < y + 1 ? x + 1 : y + 1;
            m = a.w - x < m ? a.w - x : m;
            m = a.h - y < m ? a.h - y : m;
            return (long long)m * m;
        };
        out[VISTAF_CENTRELINE_A_AT_BORDER] = reach(fAx, fAy) <= (long long)d2A ? 1.0 : 0.0;
        out[VISTAF_CENTRELINE_B_AT_BORDER] = reach(fBx, fBy) <= (long long)d2B ? 1.0 : 0.0;
        if (depth) {
            out[VISTAF_CENTRELINE_DEPTH_MEAN_MM] = zsum / (double)n;
            out[VISTAF_CENTRELINE_DEPTH_A_MM] = zA / (double)ends;
            out[VISTAF_CENTRELINE_DEPTH_B_MM] = zB / (double)ends;
            out[VISTAF_CENTRELINE_DEPTH_PEAK_MM] = peak;
            out[VISTAF_CENTRELINE_DEPTH_PEAK_STATION] = (double)peak_at;
        }
    }
}

__global__ __launch_bounds__(CL_NT) void k_centreline_rows(ClArgs a)
{
    extern __shared__ u64 cl_lds[];
    const int b = blockIdx.x / a.K, k = blockIdx.x - b * a.K;
    double *out = a.out + (size_t)blockIdx.x * VISTAF_NCENTRELINE;
    if (nan_row(k >= clamp_count(a.count[b], a.K), out, VISTAF_NCENTRELINE)) return;
    const ContactBox box(a.contacts + (size_t)blockIdx.x * VISTAF_NCONTACT, a.h, a.w);
    if (!box.total()) {
        empty_row(out, VISTAF_NCENTRELINE, VISTAF_CENTRELINE_STATUS, VISTAF_CLST_NO_PIXELS);
        return;
    }
    if (cl_box_in_lds(box.bw, box.bh)) cl_row<u64 *>(cl_lds, a, box, b, k);
    else cl_row<u64 *>(a.bf.planes + (size_t)blockIdx.x * a.bf.row_words, a, box, b, k);
}

__global__ __launch_bounds__(CL_NT) void k_centreline_poly(const int8_t *__restrict__ index, const double *__restrict__ contacts, const int32_t *__restrict__ count,
                                                           int h, int w, int K, int max_stations, CentrelineBufs bf, double *__restrict__ centrelines,
                                                           int32_t *__restrict__ stations, int32_t *__restrict__ station_d2, int32_t *__restrict__ offsets)
{
    const int b = blockIdx.x / K, k = blockIdx.x - b * K, tid = threadIdx.x;
    const int kk = clamp_count(count[b], K);
    const RowCapacity cap = row_capacity(centrelines, VISTAF_NCENTRELINE, VISTAF_CENTRELINE_STATIONS, b, K, k, kk, max_stations);
    const int before = cap.before, written = cap.written;
    if (tid == 0) {
        double *out = centrelines + (size_t)blockIdx.x * VISTAF_NCENTRELINE;
        if (k == 0) offsets[(size_t)b * (K + 1)] = 0;
        offsets[(size_t)b * (K + 1) + k + 1] = before + written;
        if (k < kk) {
            out[VISTAF_CENTRELINE_STATIONS_WRITTEN] = (double)written;
            if (written == (int)out[VISTAF_CENTRELINE_STATIONS]) out[VISTAF_CENTRELINE_STATUS] = (double)((int)out[VISTAF_CENTRELINE_STATUS] & ~VISTAF_CLST_TRUNCATED);
        }
    }
    if (!written) return;
    const size_t P = (size_t)h * w;
    const ContactBox box(contacts + (size_t)blockIdx.x * VISTAF_NCONTACT, h, w);
    const int8_t *plane = index + b * P;
    const int32_t *stn = bf.stn + b * P, *d2 = bf.d2 + b * P;
    BoxWalk<CL_NT>(box, tid).each([&](int x, int y) {
        const size_t p = (size_t)y * w + x;
        if (plane[p] != k) return;
        const int i = stn[p];
        if (i < 0) return;
        const size_t at = (size_t)b * max_stations + before + i;
        stations[2 * at] = x;
        stations[2 * at + 1] = y;
        if (station_d2) station_d2[at] = d2[p];
    });
}

}  // namespace

extern "C" {

int vistaf_ftp_test_centreline_tier(int bw, int bh) { return tier_hook_answer(bw, bh, cl_box_in_lds); }

int vistaf_centreline_workspace_bytes(int h, int w, int batch, int max_contacts, size_t *bytes)
{
    return workspace_bytes_answer(bytes, plane_sizes_refusal(h, w, batch, max_contacts), [&] { return centreline_scratch_bytes(batch, h, w, max_contacts); });
}

int vistaf_centreline_measure(const int8_t *d_contact_index, const double *d_contacts, const int32_t *d_count, const double *d_mm_per_px,
                              const float *d_depth_mm, int batch, int h, int w, int max_contacts, int tangent_span, int max_stations,
                              double *d_centrelines, int32_t *d_stations, int32_t *d_station_d2, int32_t *d_offsets, int8_t *d_skeleton,
                              void *d_workspace, size_t workspace_bytes, void *stream)
{
    if (const char *why = table_inputs_refusal(d_contact_index, d_contacts, d_count, d_mm_per_px)) return set_error(VISTAF_E_INVALID, why);
    if (!d_centrelines) return set_error(VISTAF_E_INVALID, "d_centrelines is null");
    if (const char *why = plane_sizes_refusal(h, w, batch, max_contacts)) return set_error(VISTAF_E_INVALID, why);
    if (tangent_span < 1 || tangent_span > 1024) return set_error(VISTAF_E_INVALID, "tangent_span must be 1..1024");
    if (max_stations < 0) return set_error(VISTAF_E_INVALID, "max_stations must be >= 0");
    if (!d_stations && d_offsets) return set_error(VISTAF_E_INVALID, "d_stations is null although d_offsets is given");
    if (!d_stations && d_station_d2) return set_error(VISTAF_E_INVALID, "d_stations is null although d_station_d2 is given");
    if (d_stations && !d_offsets) return set_error(VISTAF_E_INVALID, "d_offsets is null although d_stations is given");
    if (((uintptr_t)d_contacts | (uintptr_t)d_mm_per_px | (uintptr_t)d_centrelines) & 7)
        return set_error(VISTAF_E_INVALID, "d_contacts, d_mm_per_px and d_centrelines must be 8-byte aligned");
    if (((uintptr_t)d_count | (uintptr_t)d_depth_mm | (uintptr_t)d_stations | (uintptr_t)d_station_d2 | (uintptr_t)d_offsets) & 3)
        return set_error(VISTAF_E_INVALID, "d_count, d_depth_mm, d_stations, d_station_d2 and d_offsets must be 4-byte aligned");
    TRY(workspace_ok(d_workspace, workspace_bytes, centreline_scratch_bytes(batch, h, w, max_contacts), "vistaf_centreline_workspace_bytes"));
    ScratchLayout L(d_workspace);
    ClArgs a;
    a.index = d_contact_index; a.contacts = d_contacts; a.count = d_count; a.mm_per_px = d_mm_per_px; a.depth = d_depth_mm;
    a.h = h; a.w = w; a.K = max_contacts; a.span = tangent_span; a.polylines = d_stations ? 1 : 0;
    a.out = d_centrelines; a.skeleton = d_skeleton;
    a.bf = centreline_scratch(L, batch, h, w, max_contacts);
    const dim3 grid((unsigned)(batch * max_contacts));
    hipStream_t st = (hipStream_t)stream;
    if (d_skeleton) launch_fill_i8<-1>(d_skeleton, (size_t)batch * h * w, st);
    hipLaunchKernelGGL(k_centreline_rows, grid, dim3(CL_NT), cl_launch_lds(h, w), st, a);
    if (d_stations)
        hipLaunchKernelGGL(k_centreline_poly, grid, dim3(CL_NT), 0, st, d_contact_index, d_contacts, d_count, h, w, max_contacts, max_stations, a.bf,
                           d_centrelines, d_stations, d_station_d2, d_offsets);
    return launch_ok("k_centreline");
}

}  // extern "C"
