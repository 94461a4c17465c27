// Indenter match read-out (include_ext/vistaf_match.h): which known object touches, where and how turned, for every contact, from the depth plane
// of a predict and the index plane, table and counts vistaf_ftp_contacts wrote.  An extension, as the other per-contact read-outs: the reference
// has no counterpart.  The definition and the bank's layout are in the header; tests/match_helpers.py restates them in NumPy.
//
// The bank is built on the host (vistaf_match_build_bank, no HIP call) and moved to the device by the caller.  Three launches per call:
//   k_match_patch  one workgroup per (frame, row): the status of the row and its metric patch, S x S bilinear samples of the isolated depth
//                  about the centroid, rounded to float32 into d_patches.  Rows not in use, without a scale or without pixels are finished
//                  here (NaN patch, NaN scores, the status).
//   k_match_score  the hot path, g = bank . windows on the matrix cores: one workgroup of up to four waves per (frame, row, tile of 16 bank
//                  rows).  The patch sits in LDS as float32 with the disc's offsets dy*S + dx beside it.  The shifts are cut into tiles of 16;
//                  a wave owns TPW <= 5 consecutive tiles (4 * 5 * 16 >= 17^2; TPW = ceil(tiles / 4) is a template argument and the workgroup
//                  has as many waves as that takes, so the loop body is straight-line code and no wave idles) and steps through the disc four
//                  offsets at a time: lane l loads A = bank[row0 + (l & 15)][d0 + (l >> 4)] once from global memory (the bank stays in L2;
//                  the next step's load is issued before this step's MFMAs) and gathers B = patch[base(shift of tile i, l & 15) + off(d0 +
//                  (l >> 4))] from LDS for each of its tiles -- 16 consecutive float32 words per offset, four offsets, no systematic conflict
//                  -- into one v_mfma_f64_16x16x4_f64 per tile, operands zero beyond M, (2m+1)^2 and D.  S1, S2 and nz of a shift come from
//                  the same gather: a lane sums the offsets it fetches, the four lane groups are added by two shuffles.  A lane then holds
//                  four rows x its shift of every tile: score = g / sqrt(var), a running best per row over its tiles in ascending shift
//                  order, the 16 lanes of a row by four shuffles and the waves through LDS, always with the tie rule of the header (smallest
//                  shift index).  Per (frame, row, bank row) the best score, its g and its shift go to the workspace; the workgroup of tile 0
//                  also writes S1, var and nz per shift.
//   k_match_rows   one workgroup per (frame, row): valid shifts, per-template maxima (d_scores), winner, runner-up of another class and
//                  rotation contrast; up to six neighbouring dots (rotation -+1, sx -+1, sy -+1) recomputed by one wave each for the three
//                  parabolas; thread 0 writes the record.
// No memset, no atomics: every sum is formed in an order fixed by the bank and the launch geometry, so two calls give the same bits and a
// frame's rows do not depend on the batch it is measured in.
#include <cstring>
#include <string>
#include <vector>

#include "../../include_ext/vistaf_match.h"
#include "cgemm_mfma.hpp"
#include "contact_rows.hpp"
#include "host_util.hpp"

using namespace vf;

namespace {

constexpr int MT_NT = 256, MT_NW = MT_NT / 64;
constexpr int MT_TPW = 5;                                                     // tiles of 16 shifts a wave owns at most: 4 * 5 * 16 = 320 >= 17 * 17
constexpr int MT_SMAX = VISTAF_MATCH_MAX_P + 2 * VISTAF_MATCH_MAX_SHIFT;      // 49
constexpr int MT_DMAX = VISTAF_MATCH_MAX_P * VISTAF_MATCH_MAX_P + 3;          // Dp at most
constexpr int MT_NPRE = 4;                                                    // doubles per row of `pre`: status (-1: not in use), flags, rho
constexpr double MT_TWO_PI = 6.283185307179586476925286766559;
static_assert(MT_NW * MT_TPW * 16 >= (2 * VISTAF_MATCH_MAX_SHIFT + 1) * (2 * VISTAF_MATCH_MAX_SHIFT + 1), "every shift has a tile");

inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// the number of disc offsets of a P x P template (header, step 1)
int disc_count(int P)
{
    const int c = (P - 1) / 2;
    int n = 0;
    for (int dy = -c; dy <= c; dy++)
        for (int dx = -c; dx <= c; dx++) n += dx * dx + dy * dy <= c * c;
    return n;
}

// THE BANK of the header: byte offsets of its sections
struct BankLayout {
    int T, P, R, M, D, Dp;
    size_t cossin, rowtab, klass, symmetry, disc, mu, norm, rows, bytes;
};

BankLayout bank_layout(int T, int P, int R, int M, int D)
{
    BankLayout L;
    L.T = T; L.P = P; L.R = R; L.M = M; L.D = D; L.Dp = (D + 3) / 4 * 4;
    L.cossin = (size_t)VISTAF_MATCH_HEADER_INTS * 4;
    L.rowtab = L.cossin + (size_t)R * 16;
    L.klass = L.rowtab + (size_t)M * 8;
    L.symmetry = L.klass + (size_t)T * 4;
    L.disc = round_up(L.symmetry + (size_t)T * 4, 8);
    L.mu = L.disc + (size_t)D * 8;
    L.norm = L.mu + (size_t)M * 8;
    L.rows = round_up(L.norm + (size_t)M * 8, 256);
    L.bytes = L.rows + (size_t)M * L.Dp * 8;
    return L;
}

// the bank as the kernels see it
struct BankView {
    const double *cossin, *mu, *norm, *rows;
    const int32_t *rowtab, *klass, *symmetry, *disc;
    int T, P, R, M, D, Dp;
    double tmpp;
};

BankView bank_view(const void *base, const BankLayout &L, double tmpp)
{
    const uint8_t *p = (const uint8_t *)base;
    BankView v;
    v.cossin = (const double *)(p + L.cossin); v.mu = (const double *)(p + L.mu); v.norm = (const double *)(p + L.norm);
    v.rows = (const double *)(p + L.rows); v.rowtab = (const int32_t *)(p + L.rowtab); v.klass = (const int32_t *)(p + L.klass);
    v.symmetry = (const int32_t *)(p + L.symmetry); v.disc = (const int32_t *)(p + L.disc);
    v.T = L.T; v.P = L.P; v.R = L.R; v.M = L.M; v.D = L.D; v.Dp = L.Dp; v.tmpp = tmpp;
    return v;
}

// the sizes of a bank: the text of the refusal, or null with M set
const char *bank_sizes_refusal(int T, int P, int R, const int32_t *symmetry, int &M)
{
    M = 0;
    if (T < 1 || T > VISTAF_MATCH_MAX_T) return "T must be 1..64";
    if (P < VISTAF_MATCH_MIN_P || P > VISTAF_MATCH_MAX_P || P % 2 == 0) return "P must be odd and in 5..33";
    if (R < 1 || R > VISTAF_MATCH_MAX_R) return "R must be 1..64";
    if (!symmetry) return "symmetry is null";
    for (int t = 0; t < T; t++) {
        const int s = symmetry[t];
        if (s < 0 || s > VISTAF_MATCH_MAX_SYMMETRY) return "symmetry must be 0..8";
        if (s && R % s) return "symmetry must divide R (R % symmetry != 0)";
        M += s ? R / s : 1;
    }
    if (M > VISTAF_MATCH_MAX_ROWS) return "M, the rows of the bank (T, R, symmetry), must be at most 2048";
    return nullptr;
}

// The workspace, rows of it per (frame, row of the table): pre [MT_NPRE]; S1, var, nz per shift; the best score, its g and its shift per bank row
struct MatchBufs {
    double *pre, *s1, *var, *bscore, *bg;
    int32_t *nz, *bshift;
};

MatchBufs match_scratch(ScratchLayout &S, int B, int K, int m, int M)
{
    const size_t n = (size_t)B * K, ns = (size_t)(2 * m + 1) * (2 * m + 1);
    MatchBufs bf;
    bf.pre = S.take<double>(n * MT_NPRE, 256, "match_pre");
    bf.s1 = S.take<double>(n * ns, 256, "match_s1");
    bf.var = S.take<double>(n * ns, 256, "match_var");
    bf.bscore = S.take<double>(n * M, 256, "match_best_score");
    bf.bg = S.take<double>(n * M, 256, "match_best_g");
    bf.nz = S.take<int32_t>(n * ns, 256, "match_nz");
    bf.bshift = S.take<int32_t>(n * M, 256, "match_best_shift");
    return bf;
}

size_t match_scratch_bytes(int B, int K, int m, int M, ScratchRec *rec = nullptr)
{
    return scratch_bytes([&](ScratchLayout &S) { return match_scratch(S, B, K, m, M); }, rec);
}

// header, step 1, on the host: the bilinear sample of a P x P template, 0 outside the square
double sample_template(const float *tp, int P, double x, double y)
{
    const double xf = std::floor(x), yf = std::floor(y), fx = x - xf, fy = y - yf;
    const int x0 = (int)xf, y0 = (int)yf;
    auto at = [&](int xx, int yy) { return xx >= 0 && xx < P && yy >= 0 && yy < P ? (double)tp[(size_t)yy * P + xx] : 0.0; };
    const double v00 = at(x0, y0), v10 = at(x0 + 1, y0), v01 = at(x0, y0 + 1), v11 = at(x0 + 1, y0 + 1);
    return (v00 * (1.0 - fx) + v10 * fx) * (1.0 - fy) + (v01 * (1.0 - fx) + v11 * fx) * fy;
}

// header, step 3: the isolated depth at (xf, yf), coordinates as doubles so that any centroid and scale are safe to convert
__device__ inline double isolated(const float *depth, const int8_t *index, int h, int w, int k, double xf, double yf)
{
    if (!(xf >= 0.0 && xf <= (double)(w - 1) && yf >= 0.0 && yf <= (double)(h - 1))) return 0.0;
    const size_t p = (size_t)(int)yf * w + (int)xf;
    const float d = depth[p];
    return index[p] == k && finitef(d) ? (double)d : 0.0;
}

__global__ __launch_bounds__(MT_NT) void k_match_patch(const float *__restrict__ depth, const int8_t *__restrict__ index, const double *__restrict__ contacts,
                                                       const int32_t *__restrict__ count, const double *__restrict__ mm_per_px, double tmpp, int P, int m,
                                                       int T, int h, int w, int K, double *__restrict__ matches, double *__restrict__ scores,
                                                       float *__restrict__ patches, double *__restrict__ pre)
{
    const int b = blockIdx.x / K, k = blockIdx.x - b * K, tid = threadIdx.x;
    const int S = P + 2 * m, q = (P - 1) / 2 + m, SS = S * S;
    double *out = matches + (size_t)blockIdx.x * VISTAF_NMATCH, *sc = scores + (size_t)blockIdx.x * T, *pr = pre + (size_t)blockIdx.x * MT_NPRE;
    float *patch = patches + (size_t)blockIdx.x * SS;
    const double *row = contacts + (size_t)blockIdx.x * VISTAF_NCONTACT;
    const double s = mm_per_px[b], rho = tmpp / s, cx = row[VISTAF_CONTACT_CENTROID_X], cy = row[VISTAF_CONTACT_CENTROID_Y];
    int status = VISTAF_MATCHST_OK;
    if (k >= clamp_count(count[b], K)) status = -1;
    else if (!finitef(s) || !(s > 0.0) || !finitef(rho) || !(rho > 0.0)) status = VISTAF_MATCHST_NO_SCALE;
    else if (!finitef(cx) || !finitef(cy)) status = VISTAF_MATCHST_NO_PIXELS;
    if (status != VISTAF_MATCHST_OK) {                                 // workgroup-uniform
        for (int i = tid; i < SS; i += MT_NT) patch[i] = nanf32();
        for (int i = tid; i < T; i += MT_NT) sc[i] = nan64();
        if (tid < VISTAF_NMATCH) out[tid] = tid == VISTAF_MATCH_STATUS && status >= 0 ? (double)status : nan64();
        if (tid == 0) pr[0] = (double)status;
        return;
    }
    const float *dp = depth + (size_t)b * h * w;
    const int8_t *ip = index + (size_t)b * h * w;
    int clipped = 0;
    for (int i = tid; i < SS; i += MT_NT) {
        const int pi = i / S, pj = i - pi * S;
        const double x = cx + (double)(pj - q) * rho, y = cy + (double)(pi - q) * rho;
        const double xf = floor(x), yf = floor(y), fx = x - xf, fy = y - yf;
        const double v00 = isolated(dp, ip, h, w, k, xf, yf), v10 = isolated(dp, ip, h, w, k, xf + 1.0, yf);
        const double v01 = isolated(dp, ip, h, w, k, xf, yf + 1.0), v11 = isolated(dp, ip, h, w, k, xf + 1.0, yf + 1.0);
        patch[i] = (float)((v00 * (1.0 - fx) + v10 * fx) * (1.0 - fy) + (v01 * (1.0 - fx) + v11 * fx) * fy);
        clipped |= !(xf >= 0.0 && xf + 1.0 <= (double)(w - 1) && yf >= 0.0 && yf + 1.0 <= (double)(h - 1));
    }
    clipped = __syncthreads_or(clipped);
    if (tid == 0) {
        pr[0] = (double)VISTAF_MATCHST_OK;
        pr[1] = clipped ? (double)VISTAF_MATCHFL_CLIPPED : 0.0;
        pr[2] = rho;
    }
}

// the better of two candidates (score, shift index) under the tie rule: the larger score, among equals the smaller shift
__device__ inline bool beats(double s, int sh, double bs, int bsh) { return s > bs || (s == bs && sh < bsh); }

constexpr int MT_NONE = 0x7fffffff;

template <int TPW>
__global__ __launch_bounds__(MT_NT) void k_match_score(const float *__restrict__ patches, BankView bk, float eps, int m, int min_pixels, int rtiles, MatchBufs ws)
{
    __shared__ float pt[MT_SMAX * MT_SMAX];
    __shared__ int off[MT_DMAX];
    __shared__ double wsc[MT_NW][16], wgv[MT_NW][16];
    __shared__ int wsh[MT_NW][16];
    const int rowid = blockIdx.x / rtiles, rt = blockIdx.x - rowid * rtiles;
    if (!(ws.pre[(size_t)rowid * MT_NPRE] == (double)VISTAF_MATCHST_OK)) return;        // workgroup-uniform
    const int tid = threadIdx.x, nt = blockDim.x, nw = nt >> 6, lane = tid & 63, wv = tid >> 6, c16 = lane & 15, kq = lane >> 4;
    const int P = bk.P, S = P + 2 * m, q = (P - 1) / 2 + m, W = 2 * m + 1, NS = W * W, D = bk.D, Dp = bk.Dp, M = bk.M;
    const float *patch = patches + (size_t)rowid * S * S;
    for (int i = tid; i < S * S; i += nt) pt[i] = patch[i];
    for (int j = tid; j < Dp; j += nt) off[j] = j < D ? bk.disc[2 * j + 1] * S + bk.disc[2 * j] : 0;
    __syncthreads();

    // wave wv owns the shift tiles wv * TPW .. wv * TPW + TPW - 1; one behind the last tile works on zeros
    const int arow = rt * 16 + c16;
    const bool arow_in = arow < M;
    const double *ap = bk.rows + (size_t)(arow_in ? arow : 0) * Dp + kq;
    int base[TPW], shift[TPW];
    bool sin_[TPW];
    v4f64 acc[TPW];
    double s1[TPW], s2[TPW];
    int nz[TPW];
#pragma unroll
    for (int i = 0; i < TPW; i++) {
        const int s = (wv * TPW + i) * 16 + c16, sy = s / W, sx = s - sy * W;
        shift[i] = s;
        sin_[i] = s < NS;
        base[i] = sin_[i] ? (q - m + sy) * S + (q - m + sx) : q * S + q;              // the window's centre: q - m + sy in c..c+2m, so base + off is inside
        acc[i] = (v4f64){0.0, 0.0, 0.0, 0.0};
        s1[i] = 0.0; s2[i] = 0.0; nz[i] = 0;
    }
    double anext = arow_in ? ap[0] : 0.0;
    for (int d0 = 0; d0 < Dp; d0 += 4) {
        const int j = d0 + kq;                                                      // < Dp: the rows are padded with zeros
        const double a = anext;
        anext = arow_in && d0 + 4 < Dp ? ap[d0 + 4] : 0.0;                          // the next step's operand is on its way during this one's MFMAs
        const int o = off[j];
        const bool jin = j < D;
#pragma unroll
        for (int i = 0; i < TPW; i++) {
            const bool in = sin_[i] && jin;
            const float wf = in ? pt[base[i] + o] : 0.0f;
            const double wd = (double)wf;
            s1[i] += wd;
            s2[i] += wd * wd;
            nz[i] += in && wf > eps ? 1 : 0;                                        // a zero operand is no sample, whatever eps is
            acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, wd, acc[i], 0, 0, 0);
        }
    }
    // the lane's shift of every tile: its sums over the four lane groups, its verdict, and the running best of the lane's four rows
    double bs[4], bgv[4];
    int bsh[4];
#pragma unroll
    for (int r = 0; r < 4; r++) { bs[r] = -__builtin_inf(); bgv[r] = 0.0; bsh[r] = MT_NONE; }
#pragma unroll
    for (int i = 0; i < TPW; i++) {
        s1[i] += __shfl_xor(s1[i], 16); s1[i] += __shfl_xor(s1[i], 32);
        s2[i] += __shfl_xor(s2[i], 16); s2[i] += __shfl_xor(s2[i], 32);
        nz[i] += __shfl_xor(nz[i], 16); nz[i] += __shfl_xor(nz[i], 32);
        const double var = s2[i] - (s1[i] * s1[i]) / (double)D;
        const bool valid = sin_[i] && nz[i] >= min_pixels && var > 0.0;
        if (rt == 0 && kq == 0 && sin_[i]) {
            const size_t o = (size_t)rowid * NS + shift[i];
            ws.s1[o] = s1[i];
            ws.var[o] = var;
            ws.nz[o] = nz[i];
        }
        const double sd = sqrt(var);
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const double g = acc[i][r], sc = g / sd;
            if (valid && sc > bs[r]) { bs[r] = sc; bgv[r] = g; bsh[r] = shift[i]; }    // shifts ascend with i: the first of equals stays
        }
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
#pragma unroll
        for (int mask = 1; mask < 16; mask <<= 1) {
            const double os = __shfl_xor(bs[r], mask), og = __shfl_xor(bgv[r], mask);
            const int osh = __shfl_xor(bsh[r], mask);
            if (beats(os, osh, bs[r], bsh[r])) { bs[r] = os; bgv[r] = og; bsh[r] = osh; }
        }
        if (c16 == 0) { wsc[wv][kq + 4 * r] = bs[r]; wgv[wv][kq + 4 * r] = bgv[r]; wsh[wv][kq + 4 * r] = bsh[r]; }
    }
    __syncthreads();
    if (tid < 16 && rt * 16 + tid < M) {
        double fs = wsc[0][tid], fg = wgv[0][tid];
        int fsh = wsh[0][tid];
        for (int v = 1; v < nw; v++)
            if (beats(wsc[v][tid], wsh[v][tid], fs, fsh)) { fs = wsc[v][tid]; fg = wgv[v][tid]; fsh = wsh[v][tid]; }
        const size_t o = (size_t)rowid * M + rt * 16 + tid;
        const bool none = fsh == MT_NONE;
        ws.bscore[o] = none ? nan64() : fs;
        ws.bg[o] = none ? nan64() : fg;
        ws.bshift[o] = none ? -1 : fsh;
    }
}

__global__ __launch_bounds__(MT_NT) void k_match_rows(const double *__restrict__ contacts, const float *__restrict__ patches, BankView bk, MatchBufs ws, int m,
                                                      int min_pixels, double accept_score, double accept_margin, double *__restrict__ matches,
                                                      double *__restrict__ scores)
{
    __shared__ float pt[MT_SMAX * MT_SMAX];
    __shared__ double tmax[VISTAF_MATCH_MAX_T], tmin[VISTAF_MATCH_MAX_T], nb[6];
    __shared__ int trow[VISTAF_MATCH_MAX_T], wcount[MT_NW], win[2];
    const int rowid = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (!(ws.pre[(size_t)rowid * MT_NPRE] == (double)VISTAF_MATCHST_OK)) return;        // finished by k_match_patch
    const int P = bk.P, S = P + 2 * m, q = (P - 1) / 2 + m, W = 2 * m + 1, NS = W * W, D = bk.D, Dp = bk.Dp, M = bk.M, T = bk.T, R = bk.R;
    double *out = matches + (size_t)rowid * VISTAF_NMATCH;
    const float *patch = patches + (size_t)rowid * S * S;
    const double *var = ws.var + (size_t)rowid * NS, *bscore = ws.bscore + (size_t)rowid * M;
    const int32_t *nz = ws.nz + (size_t)rowid * NS, *bshift = ws.bshift + (size_t)rowid * M;
    for (int i = tid; i < S * S; i += MT_NT) pt[i] = patch[i];
    int c = 0;
    for (int s = tid; s < NS; s += MT_NT) c += nz[s] >= min_pixels && var[s] > 0.0;
    c = wave_sum(c);
    if (lane == 0) wcount[wv] = c;
    // per template: the best of its rows (ties to the smallest r) and the least, its rows being start..start+R_t-1
    if (tid < T) {
        int start = 0;
        for (int u = 0; u < tid; u++) start += bk.symmetry[u] ? R / bk.symmetry[u] : 1;
        const int rt = bk.symmetry[tid] ? R / bk.symmetry[tid] : 1;
        double best = 0.0, mn = 0.0;
        int brow = -1;
        for (int r = 0; r < rt; r++) {
            if (bshift[start + r] < 0) continue;
            const double sc = bscore[start + r];
            const bool first = brow < 0;
            if (first || sc > best) { best = sc; brow = start + r; }
            if (first || sc < mn) mn = sc;
        }
        tmax[tid] = brow >= 0 ? best : nan64();
        tmin[tid] = brow >= 0 ? mn : nan64();
        trow[tid] = brow;
        scores[(size_t)rowid * T + tid] = tmax[tid];
    }
    __syncthreads();
    if (tid == 0) {
        int wt = -1;
        for (int t = 0; t < T; t++)
            if (trow[t] >= 0 && (wt < 0 || tmax[t] > tmax[wt])) wt = t;
        win[0] = wt;
        win[1] = wt >= 0 ? trow[wt] : -1;
    }
    __syncthreads();
    const int wt = win[0], wrow = win[1];
    if (wt < 0) {
        if (tid < VISTAF_NMATCH) out[tid] = tid == VISTAF_MATCH_STATUS ? (double)VISTAF_MATCHST_NO_SUPPORT : (tid == VISTAF_MATCH_VALID_SHIFTS ? 0.0 : nan64());
        return;
    }
    const int sym = bk.symmetry[wt], rt = sym ? R / sym : 1, r = bk.rowtab[2 * wrow + 1], start = wrow - r;
    const int s = bshift[wrow], sy = s / W - m, sx = s - (s / W) * W - m;
    // ---- header, step 6: the neighbouring dots, one wave each
    for (int task = wv; task < 6; task += MT_NW) {
        int row = wrow, tx = sx, ty = sy;
        bool run = true;
        if (task == 0) { row = start + (r + rt - 1) % rt; run = rt >= 3; }
        if (task == 1) { row = start + (r + 1) % rt; run = rt >= 3; }
        if (task == 2) tx = sx - 1;
        if (task == 3) tx = sx + 1;
        if (task == 4) ty = sy - 1;
        if (task == 5) ty = sy + 1;
        run = run && tx >= -m && tx <= m && ty >= -m && ty <= m;
        const int ts = (ty + m) * W + (tx + m);
        run = run && nz[ts] >= min_pixels && var[ts] > 0.0;
        double score = nan64();
        if (run) {                                                                  // wave-uniform
            const double *br = bk.rows + (size_t)row * Dp;
            const int base = (q + ty) * S + (q + tx);
            double p = 0.0;
            for (int j = lane; j < D; j += 64) p += br[j] * (double)pt[base + bk.disc[2 * j + 1] * S + bk.disc[2 * j]];
            score = wave_sum(p) / sqrt(var[ts]);
        }
        if (lane == 0) nb[task] = score;
    }
    __syncthreads();
    if (tid != 0) return;
    int nvalid = 0;
    for (int v = 0; v < MT_NW; v++) nvalid += wcount[v];
    const double *crow = contacts + (size_t)rowid * VISTAF_NCONTACT;
    const double cx = crow[VISTAF_CONTACT_CENTROID_X], cy = crow[VISTAF_CONTACT_CENTROID_Y], rho = ws.pre[(size_t)rowid * MT_NPRE + 2];
    const double a0 = bscore[wrow], g = ws.bg[(size_t)rowid * M + wrow], s1 = ws.s1[(size_t)rowid * NS + s], vr = var[s];
    auto parabola = [&](double am, double ap) {
        if (!(am == am) || !(ap == ap)) return 0.0;
        const double den = (am - 2.0 * a0) + ap;
        return den < 0.0 ? (0.5 * (am - ap)) / den : 0.0;
    };
    const double dr = rt >= 3 ? parabola(nb[0], nb[1]) : 0.0, dx = parabola(nb[2], nb[3]), dy = parabola(nb[4], nb[5]);
    double ang = 0.0;
    if (sym) {
        const double per = MT_TWO_PI / (double)sym;
        ang = (((double)r + dr) * MT_TWO_PI) / (double)R;
        if (ang < 0.0) ang += per;
        if (ang >= per) ang -= per;
    }
    // the runner-up of another class
    int st = -1;
    for (int t = 0; t < T; t++)
        if (trow[t] >= 0 && bk.klass[t] != bk.klass[wt] && (st < 0 || tmax[t] > tmax[st])) st = t;
    const double second = st >= 0 ? tmax[st] : nan64(), margin = a0 - second;
    int flags = (int)ws.pre[(size_t)rowid * MT_NPRE + 1];
    if (m > 0 && (sx == -m || sx == m || sy == -m || sy == m)) flags |= VISTAF_MATCHFL_BORDER_SHIFT;
    if (a0 < accept_score) flags |= VISTAF_MATCHFL_WEAK;
    if (margin < accept_margin) flags |= VISTAF_MATCHFL_AMBIGUOUS;
    const double scale = g / bk.norm[wrow], rest = vr - g * g;
    out[VISTAF_MATCH_STATUS] = (double)VISTAF_MATCHST_OK;
    out[VISTAF_MATCH_FLAGS] = (double)flags;
    out[VISTAF_MATCH_LABEL] = flags & (VISTAF_MATCHFL_WEAK | VISTAF_MATCHFL_AMBIGUOUS) ? -1.0 : (double)bk.klass[wt];
    out[VISTAF_MATCH_TEMPLATE] = (double)wt;
    out[VISTAF_MATCH_CLASS] = (double)bk.klass[wt];
    out[VISTAF_MATCH_ROTATION] = (double)r;
    out[VISTAF_MATCH_SHIFT_X] = (double)sx;
    out[VISTAF_MATCH_SHIFT_Y] = (double)sy;
    out[VISTAF_MATCH_SCORE] = a0;
    out[VISTAF_MATCH_ANGLE_RAD] = ang;
    out[VISTAF_MATCH_X_PX] = cx + ((double)sx + dx) * rho;
    out[VISTAF_MATCH_Y_PX] = cy + ((double)sy + dy) * rho;
    out[VISTAF_MATCH_OFFSET_X_MM] = ((double)sx + dx) * bk.tmpp;
    out[VISTAF_MATCH_OFFSET_Y_MM] = ((double)sy + dy) * bk.tmpp;
    out[VISTAF_MATCH_SECOND_CLASS] = st >= 0 ? (double)bk.klass[st] : -1.0;
    out[VISTAF_MATCH_SECOND_SCORE] = second;
    out[VISTAF_MATCH_MARGIN] = margin;
    out[VISTAF_MATCH_ROT_CONTRAST] = a0 - tmin[wt];
    out[VISTAF_MATCH_SCALE] = scale;
    out[VISTAF_MATCH_BASE_MM] = s1 / (double)D - scale * bk.mu[wrow];
    out[VISTAF_MATCH_RESID_RMS_MM] = sqrt((rest > 0.0 ? rest : 0.0) / (double)D);
    out[VISTAF_MATCH_SUPPORT_PIXELS] = (double)nz[s];
    out[VISTAF_MATCH_VALID_SHIFTS] = (double)nvalid;
    out[23] = nan64();
}

// the size checks the workspace function and measure share: the text of the refusal, or null
const char *match_sizes_refusal(int h, int w, int batch, const char *batch_text, int max_contacts, int P, int max_shift, int M)
{
    if (const char *why = depth_sizes_refusal(h, w, batch, batch_text, max_contacts)) return why;
    if (P < VISTAF_MATCH_MIN_P || P > VISTAF_MATCH_MAX_P || P % 2 == 0) return "P must be odd and in 5..33";
    if (max_shift < 0 || max_shift > VISTAF_MATCH_MAX_SHIFT) return "max_shift must be 0..8";
    if (M < 1 || M > VISTAF_MATCH_MAX_ROWS) return "M must be 1..2048";
    return nullptr;
}

}  // namespace

extern "C" {

int vistaf_match_bank_bytes(int T, int P, int R, const int32_t *symmetry, size_t *bytes)
{
    if (!bytes) return set_error(VISTAF_E_INVALID, "bytes is null");
    *bytes = 0;
    int M;
    if (const char *why = bank_sizes_refusal(T, P, R, symmetry, M)) return set_error(VISTAF_E_INVALID, why);
    *bytes = bank_layout(T, P, R, M, disc_count(P)).bytes;
    return 0;
}

int vistaf_match_build_bank(const float *templates, const int32_t *klass, const int32_t *symmetry, int T, int P, int R, double template_mm_per_px,
                            void *h_bank, size_t bank_bytes)
{
    if (!templates) return set_error(VISTAF_E_INVALID, "templates is null");
    if (!klass) return set_error(VISTAF_E_INVALID, "klass is null");
    if (!h_bank) return set_error(VISTAF_E_INVALID, "h_bank is null");
    int M;
    if (const char *why = bank_sizes_refusal(T, P, R, symmetry, M)) return set_error(VISTAF_E_INVALID, why);
    for (int t = 0; t < T; t++)
        if (klass[t] < 0) return set_error(VISTAF_E_INVALID, "klass[" + std::to_string(t) + "] must be >= 0");
    if (!std::isfinite(template_mm_per_px) || !(template_mm_per_px > 0.0)) return set_error(VISTAF_E_INVALID, "template_mm_per_px must be finite and > 0");
    if ((uintptr_t)h_bank & 7) return set_error(VISTAF_E_INVALID, "h_bank must be 8-byte aligned");
    const int D = disc_count(P), c = (P - 1) / 2;
    const BankLayout L = bank_layout(T, P, R, M, D);
    if (bank_bytes != L.bytes) return set_error(VISTAF_E_INVALID, "bank_bytes is not what vistaf_match_bank_bytes gives for these sizes");
    uint8_t *base = (uint8_t *)h_bank;
    std::memset(base, 0, L.bytes);
    int32_t *hdr = (int32_t *)base, *rowtab = (int32_t *)(base + L.rowtab), *kl = (int32_t *)(base + L.klass), *sy = (int32_t *)(base + L.symmetry);
    int32_t *disc = (int32_t *)(base + L.disc);
    double *cs = (double *)(base + L.cossin), *mu = (double *)(base + L.mu), *norm = (double *)(base + L.norm), *rows = (double *)(base + L.rows);
    hdr[0] = VISTAF_MATCH_MAGIC; hdr[1] = T; hdr[2] = P; hdr[3] = R; hdr[4] = M; hdr[5] = D; hdr[6] = L.Dp;
    std::memcpy(hdr + 8, &template_mm_per_px, 8);
    for (int r = 0; r < R; r++) {
        const double theta = ((2.0 * M_PI) * (double)r) / (double)R;
        cs[2 * r] = std::cos(theta);
        cs[2 * r + 1] = std::sin(theta);
    }
    int n = 0;
    for (int dy = -c; dy <= c; dy++)
        for (int dx = -c; dx <= c; dx++)
            if (dx * dx + dy * dy <= c * c) { disc[2 * n] = dx; disc[2 * n + 1] = dy; n++; }
    std::vector<double> v((size_t)D);
    int row = 0;
    for (int t = 0; t < T; t++) {
        kl[t] = klass[t];
        sy[t] = symmetry[t];
        const int rt = symmetry[t] ? R / symmetry[t] : 1;
        const float *tp = templates + (size_t)t * P * P;
        for (int r = 0; r < rt; r++, row++) {
            rowtab[2 * row] = t;
            rowtab[2 * row + 1] = r;
            const double co = cs[2 * r], si = cs[2 * r + 1];
            double sum = 0.0;
            for (int j = 0; j < D; j++) {
                const double dx = (double)disc[2 * j], dy = (double)disc[2 * j + 1];
                v[j] = sample_template(tp, P, ((double)c + co * dx) + si * dy, ((double)c - si * dx) + co * dy);
                sum += v[j];
            }
            const double mean = sum / (double)D;
            double ss = 0.0;
            for (int j = 0; j < D; j++) ss += (v[j] - mean) * (v[j] - mean);
            const double nr = std::sqrt(ss);
            if (!std::isfinite(mean) || !std::isfinite(nr))
                return set_error(VISTAF_E_INVALID, "templates[" + std::to_string(t) + "] holds a value that is not finite");
            if (nr == 0.0) return set_error(VISTAF_E_INVALID, "templates[" + std::to_string(t) + "] is flat over the disc: nothing to correlate with");
            mu[row] = mean;
            norm[row] = nr;
            for (int j = 0; j < D; j++) rows[(size_t)row * L.Dp + j] = (v[j] - mean) / nr;
        }
    }
    return 0;
}

int vistaf_match_workspace_bytes(int h, int w, int max_batch, int max_contacts, int P, int max_shift, int M, size_t *bytes)
{
    return workspace_bytes_answer(bytes, match_sizes_refusal(h, w, max_batch, "max_batch must be 1..2^19", max_contacts, P, max_shift, M),
                                  [&] { return match_scratch_bytes(max_batch, max_contacts, max_shift, M); });
}

int vistaf_match_measure(const float *d_depth_mm, const int8_t *d_contact_index, const double *d_contacts, const int32_t *d_count,
                         const double *d_mm_per_px, const void *d_bank, size_t bank_bytes, const int32_t *h_bank_header, float depth_eps_mm,
                         int max_shift, int min_pixels, double accept_score, double accept_margin, int h, int w, int batch, int max_contacts,
                         double *d_matches, double *d_scores, float *d_patches, void *d_workspace, size_t workspace_bytes, void *stream)
{
    if (!d_depth_mm) return set_error(VISTAF_E_INVALID, "d_depth_mm is null");
    if (const char *why = table_inputs_refusal(d_contact_index, d_contacts, d_count, d_mm_per_px)) return set_error(VISTAF_E_INVALID, why);
    if (!d_bank) return set_error(VISTAF_E_INVALID, "d_bank is null");
    if (!h_bank_header) return set_error(VISTAF_E_INVALID, "h_bank_header is null");
    if (!d_matches) return set_error(VISTAF_E_INVALID, "d_matches is null");
    if (!d_scores) return set_error(VISTAF_E_INVALID, "d_scores is null");
    if (!d_patches) return set_error(VISTAF_E_INVALID, "d_patches is null");
    // the header, by value: what the builder wrote, held against bank_bytes
    const int T = h_bank_header[1], P = h_bank_header[2], R = h_bank_header[3], M = h_bank_header[4], D = h_bank_header[5], Dp = h_bank_header[6];
    double tmpp;
    std::memcpy(&tmpp, h_bank_header + 8, 8);
    if (h_bank_header[0] != VISTAF_MATCH_MAGIC) return set_error(VISTAF_E_INVALID, "h_bank_header does not start a bank of vistaf_match_build_bank");
    if (T < 1 || T > VISTAF_MATCH_MAX_T || R < 1 || R > VISTAF_MATCH_MAX_R || P < VISTAF_MATCH_MIN_P || P > VISTAF_MATCH_MAX_P || P % 2 == 0 || M < 1 ||
        M > VISTAF_MATCH_MAX_ROWS || M > T * R || D != disc_count(P) || Dp != (D + 3) / 4 * 4 || !std::isfinite(tmpp) || !(tmpp > 0.0))
        return set_error(VISTAF_E_INVALID, "h_bank_header holds sizes no bank has");
    const BankLayout L = bank_layout(T, P, R, M, D);
    if (bank_bytes != L.bytes) return set_error(VISTAF_E_INVALID, "bank_bytes is not the size of the bank h_bank_header describes");
    if (const char *why = match_sizes_refusal(h, w, batch, "batch must be 1..2^19", max_contacts, P, max_shift, M)) return set_error(VISTAF_E_INVALID, why);
    if (!std::isfinite(depth_eps_mm)) return set_error(VISTAF_E_INVALID, "depth_eps_mm must be finite");
    if (min_pixels < 1) return set_error(VISTAF_E_INVALID, "min_pixels must be >= 1");
    if (!std::isfinite(accept_score)) return set_error(VISTAF_E_INVALID, "accept_score must be finite");
    if (!std::isfinite(accept_margin)) return set_error(VISTAF_E_INVALID, "accept_margin must be finite");
    if (((uintptr_t)d_contacts | (uintptr_t)d_mm_per_px | (uintptr_t)d_bank | (uintptr_t)d_matches | (uintptr_t)d_scores) & 7)
        return set_error(VISTAF_E_INVALID, "d_contacts, d_mm_per_px, d_bank, d_matches and d_scores must be 8-byte aligned");
    if (((uintptr_t)d_depth_mm | (uintptr_t)d_count | (uintptr_t)d_patches) & 3)
        return set_error(VISTAF_E_INVALID, "d_depth_mm, d_count and d_patches must be 4-byte aligned");
    TRY(workspace_ok(d_workspace, workspace_bytes, match_scratch_bytes(batch, max_contacts, max_shift, M), "vistaf_match_workspace_bytes"));
    const int rows = batch * max_contacts, rtiles = (M + 15) / 16;
    if ((long long)rows * rtiles > 0x7fffffffll) return set_error(VISTAF_E_INVALID, "batch * max_contacts * ceil(M / 16) must be below 2^31");
    ScratchLayout S(d_workspace);
    const MatchBufs bf = match_scratch(S, batch, max_contacts, max_shift, M);
    const BankView bk = bank_view(d_bank, L, tmpp);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_match_patch, dim3((unsigned)rows), dim3(MT_NT), 0, st, d_depth_mm, d_contact_index, d_contacts, d_count, d_mm_per_px, tmpp, P,
                       max_shift, T, h, w, max_contacts, d_matches, d_scores, d_patches, bf.pre);
    // the shift tiles of 16, TPW of them per wave and as many waves as that takes (at most four)
    const int ntl = ((2 * max_shift + 1) * (2 * max_shift + 1) + 15) / 16, tpw = (ntl + MT_NW - 1) / MT_NW, nw = (ntl + tpw - 1) / tpw;
    const dim3 sgrid((unsigned)((size_t)rows * rtiles)), sblock((unsigned)(64 * nw));
#define MATCH_SCORE(N) hipLaunchKernelGGL(k_match_score<N>, sgrid, sblock, 0, st, d_patches, bk, depth_eps_mm, max_shift, min_pixels, rtiles, bf)
    switch (tpw) {
    case 1: MATCH_SCORE(1); break;
    case 2: MATCH_SCORE(2); break;
    case 3: MATCH_SCORE(3); break;
    case 4: MATCH_SCORE(4); break;
    default: MATCH_SCORE(5); break;
    }
#undef MATCH_SCORE
    hipLaunchKernelGGL(k_match_rows, dim3((unsigned)rows), dim3(MT_NT), 0, st, d_contacts, d_patches, bk, bf, max_shift, min_pixels, accept_score,
                       accept_margin, d_matches, d_scores);
    return launch_ok("k_match");
}

}  // extern "C"
