// Surface texture read-out (include_ext/vistaf_texture.h): roughness, lay and pitch of every contact, from the depth plane of a predict and the
// index plane, table and counts vistaf_ftp_contacts wrote.  An extension, as the other per-contact read-outs: the reference has no counterpart.
// The definition is in the header; tests/texture_helpers.py restates it in NumPy.
//
// Four launches per call, the first, second and fourth with one workgroup per (frame, row) as k_shape:
//   k_texture_form   walks the row's box (contact_rows.hpp) for the monomial sums of the evaluation pixels, thread 0 solves the form
//                    (form_fit.hpp, the copy k_shape uses) and the workgroup walks the box again (it sits in L2) to write the residual of every
//                    evaluation pixel.  Whether a pixel is an evaluation pixel depends on the planes and the table only, so the workgroups
//                    behind the B*K row workgroups fill the rest of the plane with NaN element-wise in the same launch: every element is
//                    written exactly once and there is no memset.
//   k_texture_stats  one walk over the residual plane for the height and slope sums (header, steps 4 and 5).  From here on an evaluation
//                    pixel of k is a pixel of the box with index == k whose residual is not NaN, which is the same set.
//   k_texture_acf    the hot path: m * (L+1) * (2L+1) multiply-adds per contact of m pixels.  One workgroup per (frame, row, dy), dy = 0..L, of
//                    16 waves (a native-size contact is a handful of workgroups: its rows have to be spread over many waves, and with four
//                    the un-overlapped loads of one wave's chunks were the whole time); lane l of a wave owns dx = l - L (2L+1 <= 63 lanes
//                    work, all 64 load).  A wave takes box rows y, y+16, ... and each in chunks of 64 pixels: the chunk of row y stays in
//                    registers (lane i holds r(p_i), a ballot its membership), the 64 + 2L pixels of row y+dy around it go to LDS as
//                    float64 with 0 for what is not an evaluation pixel.  For every pixel i of the chunk (groups of eight without an
//                    evaluation pixel are skipped) r(p_i) is broadcast through SGPRs (two v_readlane) and lane l reads word i + l of the window:
//                    consecutive float64 words over the 32 lanes of a half wave, all 64 banks once, conflict-free; one v_fma_f64 (the
//                    product of two widened float32 values is exact, so its bits are those of a multiplication and an addition).  A term
//                    with a 0 partner leaves the sum as it is, so C needs no mask; N(t) is popcount(mask of the chunk & the window's mask
//                    shifted by l), one per 64 pixels.  The waves' partial sums are added in wave order through LDS.
//   k_texture_rows   one wave per (frame, row): normalises and mirrors the half plane into the window (d_acf and LDS), one 64-bit mask of
//                    valid and of above-threshold lags per window row, lane j holding row j; the lobe grows from t = 0 by OR-ing the
//                    neighbouring rows' masks (shuffles) and saturating along the row until no lane changes; ring, SAL, RMAX by wave
//                    reductions of integer keys; lane 0 samples the profile and finds the pitch.
// No memset, no atomics: every float64 sum is formed in an order fixed by the box and the launch geometry, so two calls give the same bits and
// a frame's rows do not depend on the batch it is measured in.
#include <string>

#include "../../include_ext/vistaf_texture.h"
#include "contact_rows.hpp"
#include "form_fit.hpp"
#include "host_util.hpp"

using namespace vf;

namespace {

constexpr int TX_NT = 512, TX_NW = TX_NT / 64;            // k_texture_form, k_texture_stats
constexpr int TX_ACF_NT = 1024, TX_ACF_NW = TX_ACF_NT / 64;
constexpr int TX_WIN = 2 * VISTAF_TEXTURE_MAX_LAG + 1;    // 63
constexpr int TX_FILL_MAX = 4096;                         // workgroups of the NaN fill at most (a grid-stride loop)

// The workspace: N(t) and C(t) of the half plane, [B*K][L+1][2L+1], entry [dy][dx+L] (dy == 0, dx < 0 is computed but not read)
struct TextureBufs {
    double *C;
    int32_t *N;
};

TextureBufs texture_scratch(ScratchLayout &S, int B, int K, int L)
{
    const size_t n = (size_t)B * K * (L + 1) * (2 * L + 1);
    TextureBufs bf;
    bf.C = S.take<double>(n, 256, "acf_sums");
    bf.N = S.take<int32_t>(n, 256, "acf_counts");
    return bf;
}

// header, step 1, from the planes and the table: is (x, y), inside the clipped box, an evaluation pixel of row k; d = its depth
struct TxEval {
    const float *depth;
    const int8_t *index;
    int w, k;
    float eps, thr;
    bool all;
    __device__ inline TxEval(const float *dp, const int8_t *ip, int w_, int k_, float eps_, double frac, const double *row)
        : depth(dp), index(ip), w(w_), k(k_), eps(eps_), thr((float)(frac * row[VISTAF_CONTACT_MAX_DEPTH_MM])), all(frac == 0.0)
    {
    }
    __device__ inline bool operator()(int x, int y, float &d) const
    {
        const size_t p = (size_t)y * w + x;
        d = depth[p];
        if (d != d) d = 0.0f;
        return index[p] == k && d > eps && (all || d >= thr);
    }
};

// from k_texture_stats on: the evaluation pixels of k as the residual plane shows them
struct TxPlane {
    const float *res;
    const int8_t *index;
    int w, h, k, x0, y0, x1, y1;
    __device__ inline TxPlane(const float *rp, const int8_t *ip, int h_, int w_, int k_, const ContactBox &b)
        : res(rp), index(ip), w(w_), h(h_), k(k_), x0(b.x0), y0(b.y0), x1(b.x1), y1(b.y1)
    {
        if (!b.total()) { x0 = 0; x1 = -1; }
    }
    __device__ inline bool in(int x, int y, float &r) const
    {
        if (x < x0 || x > x1 || y < y0 || y > y1) return false;
        const size_t p = (size_t)y * w + x;
        r = res[p];
        return index[p] == k && r == r;
    }
};

__global__ __launch_bounds__(TX_NT) void k_texture_form(const float *__restrict__ depth, const int8_t *__restrict__ index, const double *__restrict__ contacts,
                                                        const int32_t *__restrict__ count, float eps, double frac, int degree, int h, int w, int B, int K,
                                                        int nfill, double *__restrict__ textures, float *__restrict__ resid)
{
    __shared__ double wf[TX_NW][FIT_NF], tf[FIT_NF], coef[6];
    __shared__ unsigned int wm[TX_NW];
    __shared__ int form_status;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int nrows = B * K;
    const size_t P = (size_t)h * w;
    if ((int)blockIdx.x >= nrows) {
        // ---- the rest of the plane: NaN wherever no row workgroup writes
        const size_t all = (size_t)B * P;
        for (size_t i = (size_t)(blockIdx.x - nrows) * TX_NT + tid; i < all; i += (size_t)nfill * TX_NT) {
            const size_t b = i / P, p = i - b * P;
            const int idx = index[i], kk = clamp_count(count[b], K);
            bool member = false;
            if (idx >= 0 && idx < kk) {
                const double *row = contacts + (b * K + idx) * VISTAF_NCONTACT;
                const ContactBox box(row, h, w);
                const int y = (int)(p / w), x = (int)(p - (size_t)y * w);
                if (box.total() && x >= box.x0 && x <= box.x1 && y >= box.y0 && y <= box.y1) {
                    const TxEval ev(depth + b * P, index + b * P, w, idx, eps, frac, row);
                    float d;
                    member = ev(x, y, d);
                }
            }
            if (!member) resid[i] = nanf32();
        }
        return;
    }
    const int b = blockIdx.x / K, k = blockIdx.x - b * K;
    double *out = textures + (size_t)blockIdx.x * VISTAF_NTEXTURE;
    if (nan_row(k >= clamp_count(count[b], K), out, VISTAF_NTEXTURE)) return;
    const double *row = contacts + (size_t)blockIdx.x * VISTAF_NCONTACT;
    const ContactBox box(row, h, w);
    const BoxWalk<TX_NT> walk(box, tid);
    const FitCoords uv(box.bx0, box.by0, box.bx1, box.by1);
    const TxEval ev(depth + b * P, index + b * P, w, k, eps, frac, row);
    float *res = resid + b * P;

    // ---- sweep 1: the monomial sums of the evaluation pixels
    unsigned int m = 0;
    double f[FIT_NF];
#pragma unroll
    for (int j = 0; j < FIT_NF; j++) f[j] = 0.0;
    walk.each([&](int px, int py) {
        float d;
        if (ev(px, py, d)) {
            m++;
            fit_accumulate(f, uv.u(px), uv.v(py), (double)d);
        }
    });
    m = wave_sum(m);
    if (lane == 0) wm[wid] = m;
#pragma unroll
    for (int j = 0; j < FIT_NF; j++) {
        const double s = wave_sum(f[j]);
        if (lane == 0) wf[wid][j] = s;
    }
    __syncthreads();
    if (tid < FIT_NF) {
        double s = 0.0;
        for (int q = 0; q < TX_NW; q++) s += wf[q][tid];
        tf[tid] = s;
    }
    __syncthreads();

    // ---- thread 0: the form
    if (tid == 0) {
        unsigned int mt = 0;
        for (int q = 0; q < TX_NW; q++) mt += wm[q];
        for (int j = 0; j < VISTAF_NTEXTURE; j++) out[j] = nan64();
        out[VISTAF_TEXTURE_EVAL_PIXELS] = (double)mt;
        int status = VISTAF_TEXTUREFORM_NONE;
        if (mt >= 6) {                                                   // max(N, 6)
            double c[6];
            const double dm = (double)mt;
            const int N = degree == 0 ? 1 : (degree == 1 ? 3 : 6);
            bool ok = degree == 0 ? fit_solve<1>(tf, dm, c) : (degree == 1 ? fit_solve<3>(tf, dm, c) : fit_solve<6>(tf, dm, c));
#pragma unroll
            for (int j = 0; j < 6; j++) {
                if (j >= N) c[j] = 0.0;
                ok = ok && finitef(c[j]);
            }
            if (ok) {
                status = VISTAF_TEXTUREFORM_OK;
#pragma unroll
                for (int j = 0; j < 6; j++) {
                    coef[j] = c[j];
                    out[VISTAF_TEXTURE_FORM_C0 + j] = c[j];
                }
            }
        }
        out[VISTAF_TEXTURE_FORM_STATUS] = (double)status;
        form_status = status;
    }
    __syncthreads();

    // ---- sweep 2: the residual of every evaluation pixel (NaN without a form)
    const bool ok = form_status == VISTAF_TEXTUREFORM_OK;
    double c[6];
#pragma unroll
    for (int j = 0; j < 6; j++) c[j] = ok ? coef[j] : 0.0;
    walk.each([&](int px, int py) {
        float d;
        if (ev(px, py, d)) res[(size_t)py * w + px] = ok ? (float)((double)d - fit_poly(c, uv.u(px), uv.v(py))) : nanf32();
    });
}

constexpr int TX_NS = 8;          // float64 sums of k_texture_stats: |r|, r^2, r^3, r^4, Jxx, Jyy, Jxy, the SDR terms

__global__ __launch_bounds__(TX_NT) void k_texture_stats(const int8_t *__restrict__ index, const double *__restrict__ contacts, const int32_t *__restrict__ count,
                                                         const double *__restrict__ mm_per_px, const float *__restrict__ resid, int h, int w, int K,
                                                         double *textures)
{
    __shared__ double wf[TX_NW][TX_NS];
    __shared__ unsigned long long wk[TX_NW][2];
    __shared__ unsigned int wg[TX_NW];
    const int b = blockIdx.x / K, k = blockIdx.x - b * K;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    double *out = textures + (size_t)blockIdx.x * VISTAF_NTEXTURE;
    if (k >= clamp_count(count[b], K)) return;
    if (!(out[VISTAF_TEXTURE_FORM_STATUS] == (double)VISTAF_TEXTUREFORM_OK)) return;
    const size_t P = (size_t)h * w;
    const ContactBox box(contacts + (size_t)blockIdx.x * VISTAF_NCONTACT, h, w);
    const BoxWalk<TX_NT> walk(box, tid);
    const TxPlane pl(resid + b * P, index + b * P, h, w, k, box);
    const double s2 = 2.0 * mm_per_px[b];

    double f[TX_NS];
#pragma unroll
    for (int j = 0; j < TX_NS; j++) f[j] = 0.0;
    unsigned int g = 0;
    unsigned long long kmax = 0, kmin = 0;          // arg-max keys of r and of -r: the larger value, among equals the smaller index
    walk.each([&](int px, int py) {
        float r;
        if (!pl.in(px, py, r)) return;
        const double rd = (double)r, r2 = rd * rd;
        f[0] += fabs(rd); f[1] += r2; f[2] += r2 * rd; f[3] += r2 * r2;
        const unsigned flat = (unsigned)((size_t)py * w + px);
        const unsigned long long ka = argmax_key(r + 0.0f, flat), kb = argmax_key(0.0f - r, flat);
        kmax = ka > kmax ? ka : kmax;
        kmin = kb > kmin ? kb : kmin;
        float rw, re, rn, rs;
        if (px > 0 && px + 1 < w && py > 0 && py + 1 < h && pl.in(px - 1, py, rw) && pl.in(px + 1, py, re) && pl.in(px, py - 1, rn) &&
            pl.in(px, py + 1, rs)) {
            const double rx = ((double)re - (double)rw) / s2, ry = ((double)rs - (double)rn) / s2;
            g++;
            f[4] += rx * rx; f[5] += ry * ry; f[6] += rx * ry;
            f[7] += sqrt((1.0 + rx * rx) + ry * ry) - 1.0;
        }
    });
#pragma unroll
    for (int j = 0; j < TX_NS; j++) {
        const double s = wave_sum(f[j]);
        if (lane == 0) wf[wid][j] = s;
    }
    g = wave_sum(g);
    kmax = wave_max_u64(kmax);
    kmin = wave_max_u64(kmin);
    if (lane == 0) { wg[wid] = g; wk[wid][0] = kmax; wk[wid][1] = kmin; }
    __syncthreads();
    if (tid != 0) return;
    double t[TX_NS];
#pragma unroll
    for (int j = 0; j < TX_NS; j++) {
        double s = 0.0;
        for (int q = 0; q < TX_NW; q++) s += wf[q][j];
        t[j] = s;
    }
    unsigned int gt = 0;
    unsigned long long ka = 0, kb = 0;
    for (int q = 0; q < TX_NW; q++) {
        gt += wg[q];
        ka = wk[q][0] > ka ? wk[q][0] : ka;
        kb = wk[q][1] > kb ? wk[q][1] : kb;
    }
    const double dm = out[VISTAF_TEXTURE_EVAL_PIXELS];
    out[VISTAF_TEXTURE_SP_PIXEL] = (double)(0xffffffffu - (uint32_t)ka);
    out[VISTAF_TEXTURE_SV_PIXEL] = (double)(0xffffffffu - (uint32_t)kb);
    if (t[1] == 0.0) {
        out[VISTAF_TEXTURE_FORM_STATUS] = (double)VISTAF_TEXTUREFORM_FLAT;
        out[VISTAF_TEXTURE_SA_MM] = 0.0; out[VISTAF_TEXTURE_SQ_MM] = 0.0; out[VISTAF_TEXTURE_SP_MM] = 0.0; out[VISTAF_TEXTURE_SV_MM] = 0.0;
        out[VISTAF_TEXTURE_SZ_MM] = 0.0;
        return;
    }
    const double sq = sqrt(t[1] / dm), sp = (double)key2f((uint32_t)(ka >> 32)), sv = (double)key2f((uint32_t)(kb >> 32));
    out[VISTAF_TEXTURE_SA_MM] = t[0] / dm;
    out[VISTAF_TEXTURE_SQ_MM] = sq;
    out[VISTAF_TEXTURE_SSK] = (t[2] / dm) / (sq * sq * sq);
    out[VISTAF_TEXTURE_SKU] = (t[3] / dm) / ((sq * sq) * (sq * sq));
    out[VISTAF_TEXTURE_SP_MM] = sp;
    out[VISTAF_TEXTURE_SV_MM] = sv;
    out[VISTAF_TEXTURE_SZ_MM] = sp + sv;
    out[VISTAF_TEXTURE_GRAD_PIXELS] = (double)gt;
    if (!gt) return;
    const double dg = (double)gt, jxx = t[4], jyy = t[5], jxy = t[6];
    out[VISTAF_TEXTURE_SDQ] = sqrt((jxx + jyy) / dg);
    out[VISTAF_TEXTURE_SDR] = t[7] / dg;
    const double hd = (jxx - jyy) / 2.0, rad = sqrt(hd * hd + jxy * jxy);
    const double ex = hd >= 0.0 ? hd + rad : jxy, ey = hd >= 0.0 ? jxy : rad - hd;
    double gx = 1.0, gy = 0.0;
    if (!(ex == 0.0 && ey == 0.0)) {
        const double n = sqrt(ex * ex + ey * ey);
        gx = ex / n;
        gy = ey / n;
        if (gx < 0.0 || (gx == 0.0 && gy < 0.0)) { gx = -gx; gy = -gy; }
    }
    out[VISTAF_TEXTURE_GRAD_DIR_X] = gx;
    out[VISTAF_TEXTURE_GRAD_DIR_Y] = gy;
    out[VISTAF_TEXTURE_COHERENCE] = rad / ((jxx + jyy) / 2.0);
}

__global__ __launch_bounds__(TX_ACF_NT) void k_texture_acf(const int8_t *__restrict__ index, const double *__restrict__ contacts, const int32_t *__restrict__ count,
                                                           const double *__restrict__ textures, const float *__restrict__ resid, int h, int w, int K, int L,
                                                           double *__restrict__ wsC, int32_t *__restrict__ wsN)
{
    __shared__ double win[TX_ACF_NW][128];          // 64 + 2L <= 126 words of row y+dy, window word j = pixel cx - L + j
    __shared__ double pc[TX_ACF_NW][64];
    __shared__ int pn[TX_ACF_NW][64];
    const int dy = blockIdx.x % (L + 1), rowid = blockIdx.x / (L + 1);
    const int b = rowid / K, k = rowid - b * K;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // rows not in use, rows without a form and flat rows leave before touching the planes
    if (k >= clamp_count(count[b], K)) return;
    if (!(textures[(size_t)rowid * VISTAF_NTEXTURE + VISTAF_TEXTURE_FORM_STATUS] == (double)VISTAF_TEXTUREFORM_OK)) return;
    const ContactBox box(contacts + (size_t)rowid * VISTAF_NCONTACT, h, w);
    if (!box.total()) return;
    const size_t P = (size_t)h * w;
    const float *res = resid + b * P;
    const int8_t *idx = index + b * P;
    const int D = 2 * L + 1;

    double acc = 0.0;
    int n = 0;
    for (int y = box.y0 + wv; y + dy <= box.y1; y += TX_ACF_NW) {
        const size_t ra = (size_t)y * w, rb = (size_t)(y + dy) * w;
        for (int cx = box.x0; cx <= box.x1; cx += 64) {
            // the chunk of row y and the window of row y+dy around it: all loads first, one latency
            const int xa = cx + lane;
            float ra_v = nanf32(), rb_v[2] = {nanf32(), nanf32()};
            int ia = -1, ib[2] = {-1, -1};
            if (xa <= box.x1) { ra_v = res[ra + xa]; ia = idx[ra + xa]; }
#pragma unroll
            for (int part = 0; part < 2; part++) {
                const int j = lane + 64 * part, xb = cx - L + j;
                if (j < 64 + 2 * L && xb >= box.x0 && xb <= box.x1) { rb_v[part] = res[rb + xb]; ib[part] = idx[rb + xb]; }
            }
            const bool ma = ia == k && ra_v == ra_v;
            const unsigned long long mA = __ballot(ma);
            if (!mA) continue;
            __builtin_amdgcn_wave_barrier();                      // the window of the chunk before has been read
            unsigned long long mB[2];
#pragma unroll
            for (int part = 0; part < 2; part++) {
                const bool mb = ib[part] == k && rb_v[part] == rb_v[part];
                mB[part] = __ballot(mb);
                win[wv][lane + 64 * part] = mb ? (double)rb_v[part] : 0.0;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const unsigned long long sh = lane == 0 ? mB[0] : (mB[0] >> lane) | (mB[1] << (64 - lane));
            n += __popcll(mA & sh);
            const unsigned long long abits = (unsigned long long)__double_as_longlong(ma ? (double)ra_v : 0.0);
            const double *wl = &win[wv][lane];
            // The 64 pixels in order, eight at a time, a group without an evaluation pixel skipped: the lane and the window offset are
            // constants of the unrolled code, so a pixel costs two v_readlane, one ds_read_b64 and the v_fma_f64 and no address or bit
            // arithmetic; a pixel of the group that is not an evaluation pixel adds 0 * (a finite word), which leaves the sum as it is.
#pragma unroll
            for (int g = 0; g < 8; g++) {
                if (!((mA >> (8 * g)) & 0xffull)) continue;
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const int i = 8 * g + u;
                    acc = fma(__longlong_as_double((long long)readlane64(abits, i)), wl[i], acc);      // i + lane <= 126
                }
            }
        }
    }
    pc[wv][lane] = acc;
    pn[wv][lane] = n;
    __syncthreads();
    if (tid < D) {
        double s = 0.0;
        int c = 0;
        for (int q = 0; q < TX_ACF_NW; q++) { s += pc[q][tid]; c += pn[q][tid]; }
        const size_t o = ((size_t)rowid * (L + 1) + dy) * D + tid;
        wsC[o] = s;
        wsN[o] = c;
    }
}

__global__ __launch_bounds__(64) void k_texture_rows(const int32_t *__restrict__ count, const double *__restrict__ mm_per_px, const double *__restrict__ wsC,
                                                     const int32_t *__restrict__ wsN, double thr, double peak_min, int K, int L, double *textures,
                                                     double *__restrict__ acf)
{
    __shared__ double A[TX_WIN * TX_WIN];
    __shared__ double prof[VISTAF_TEXTURE_MAX_LAG + 1];
    const int rowid = blockIdx.x, b = rowid / K, k = rowid - b * K, lane = threadIdx.x;
    const int D = 2 * L + 1, DD = D * D;
    double *win = acf + (size_t)rowid * DD, *out = textures + (size_t)rowid * VISTAF_NTEXTURE;
    const bool live = k < clamp_count(count[b], K) && out[VISTAF_TEXTURE_FORM_STATUS] == (double)VISTAF_TEXTUREFORM_OK;
    if (!live) {
        for (int i = lane; i < DD; i += 64) win[i] = nan64();
        return;
    }
    // ---- header, step 6: the window, mirrored from the half plane
    const double dm = out[VISTAF_TEXTURE_EVAL_PIXELS], s = mm_per_px[b];
    const long long mi = (long long)dm, need = mi / 8 > 16 ? mi / 8 : 16;
    const size_t base = (size_t)rowid * (L + 1) * D;
    const double c0m = wsC[base + L] / dm;
    for (int i = lane; i < DD; i += 64) {
        const int jy = i / D, jx = i - jy * D;
        int dx = jx - L, dy = jy - L;
        if (dy < 0 || (dy == 0 && dx < 0)) { dx = -dx; dy = -dy; }
        const size_t o = base + (size_t)dy * D + dx + L;
        const int N = wsN[o];
        const double a = N >= need ? (wsC[o] / (double)N) / c0m : nan64();
        A[i] = a;
        win[i] = a;
    }
    __syncthreads();
    // lane j holds window row j: its valid lags and those above the threshold
    unsigned long long valid = 0, above = 0;
    if (lane < D)
        for (int x = 0; x < D; x++) {
            const double a = A[lane * D + x];
            if (a == a) {
                valid |= 1ull << x;
                if (a > thr) above |= 1ull << x;
            }
        }
    const unsigned int nvalid = wave_sum((unsigned int)__popcll(valid));
    if (lane == 0) out[VISTAF_TEXTURE_ACF_VALID_LAGS] = (double)nvalid;
    if (!((readlane64(valid, L) >> L) & 1ull)) return;          // t = 0 is not valid: no lag is

    // ---- step 7: the lobe grows from t = 0 until no row changes
    unsigned long long lobe = lane == L ? (1ull << L) & above : 0ull;
    for (;;) {
        const unsigned long long up = __shfl_up(lobe, 1), down = __shfl_down(lobe, 1);
        unsigned long long nl = lobe | (((lane > 0 ? up : 0ull) | (lane < 63 ? down : 0ull)) & above);
        for (;;) {
            const unsigned long long t = nl | (((nl << 1) | (nl >> 1)) & above);
            if (t == nl) break;
            nl = t;
        }
        const bool changed = nl != lobe;
        lobe = nl;
        if (!__any(changed)) break;
    }
    const unsigned int nlobe = wave_sum((unsigned int)__popcll(lobe));
    const unsigned long long full = (1ull << D) - 1ull;
    const unsigned long long up = __shfl_up(lobe, 1), down = __shfl_down(lobe, 1);
    const unsigned long long dil = lane < D ? ((lobe << 1) | (lobe >> 1) | (lane > 0 ? up : 0ull) | (lane < 63 ? down : 0ull)) & full & ~lobe : 0ull;
    const unsigned long long ring = dil & valid;
    const bool open = (dil & ~valid) != 0 || (lobe & (1ull | (1ull << (D - 1)))) != 0 || ((lane == 0 || lane == D - 1) && lobe != 0);
    const bool any_open = __any(open);
    unsigned long long kmin = ~0ull;
    unsigned int d2max = 0;
    {
        const int dy = lane - L;
        for (unsigned long long mm = ring; mm; mm &= mm - 1) {
            const int x = __builtin_ctzll(mm), dx = x - L;
            const unsigned int d2 = (unsigned int)(dx * dx + dy * dy);
            d2max = d2 > d2max ? d2 : d2max;
            if (dy > 0 || (dy == 0 && dx >= 0)) {
                const unsigned long long key = ((unsigned long long)d2 << 32) | ((unsigned long long)dy << 16) | (unsigned long long)x;
                kmin = key < kmin ? key : kmin;
            }
        }
    }
    kmin = wave_min_u64(kmin);
    d2max = wave_max_u32(d2max);
    if (lane != 0) return;
    out[VISTAF_TEXTURE_LOBE_LAGS] = (double)nlobe;
    out[VISTAF_TEXTURE_LOBE_STATUS] = any_open ? 1.0 : 0.0;
    if (d2max) {
        const double sal = s * sqrt((double)(unsigned int)(kmin >> 32)), rmax = s * sqrt((double)d2max);
        out[VISTAF_TEXTURE_SAL_MM] = sal;
        out[VISTAF_TEXTURE_SAL_LAG_X] = (double)((int)(kmin & 0xffffull) - L);
        out[VISTAF_TEXTURE_SAL_LAG_Y] = (double)(int)((kmin >> 16) & 0xffffull);
        out[VISTAF_TEXTURE_RMAX_MM] = rmax;
        out[VISTAF_TEXTURE_STR] = sal / rmax;
    }
    // ---- step 8: the profile along the dominant gradient and its first peak
    const double gx = out[VISTAF_TEXTURE_GRAD_DIR_X], gy = out[VISTAF_TEXTURE_GRAD_DIR_Y];
    int ns = 1;
    prof[0] = 1.0;
    if (finitef(gx) && finitef(gy))
        for (int j = 1; j <= L; j++) {
            const double fx = floor((double)j * gx + 0.5), fy = floor((double)j * gy + 0.5);
            if (!(fx >= (double)-L && fx <= (double)L && fy >= (double)-L && fy <= (double)L)) break;
            const double a = A[((int)fy + L) * D + (int)fx + L];
            if (a != a) break;
            prof[j] = a;
            ns++;
        }
    out[VISTAF_TEXTURE_PROFILE_SAMPLES] = (double)ns;
    bool below = false;
    for (int j = 2; j <= L - 1 && j + 1 < ns; j++) {
        const double am = prof[j - 1], a0 = prof[j], ap = prof[j + 1];
        below = below || am <= thr;
        if (am < a0 && a0 >= ap && a0 >= peak_min && below) {
            out[VISTAF_TEXTURE_PITCH_MM] = s * ((double)j + (0.5 * (am - ap)) / (am - 2.0 * a0 + ap));
            out[VISTAF_TEXTURE_PITCH_ACF] = a0;
            break;
        }
    }
}

}  // namespace

namespace vf {

size_t texture_scratch_bytes(int B, int K, int L, ScratchRec *rec)
{
    return scratch_bytes([&](ScratchLayout &S) { return texture_scratch(S, B, K, L); }, rec);
}

}  // namespace vf

// the size checks both functions share: the text of the refusal, or null
static const char *texture_sizes_refusal(int h, int w, int batch, const char *batch_text, int max_contacts, int max_lag)
{
    if (const char *why = depth_sizes_refusal(h, w, batch, batch_text, max_contacts)) return why;
    if (max_lag < VISTAF_TEXTURE_MIN_LAG || max_lag > VISTAF_TEXTURE_MAX_LAG) return "max_lag must be 2..31";
    return nullptr;
}

extern "C" {

int vistaf_texture_workspace_bytes(int h, int w, int max_batch, int max_contacts, int max_lag, size_t *bytes)
{
    return workspace_bytes_answer(bytes, texture_sizes_refusal(h, w, max_batch, "max_batch must be 1..2^19", max_contacts, max_lag),
                                  [&] { return texture_scratch_bytes(max_batch, max_contacts, max_lag, nullptr); });
}

int vistaf_texture_measure(const float *d_depth_mm, const int8_t *d_contact_index, const double *d_contacts, const int32_t *d_count,
                           const double *d_mm_per_px, float depth_eps_mm, double eval_min_fraction, int form_degree, int max_lag,
                           double acf_threshold, double peak_min, int h, int w, int batch, int max_contacts, double *d_textures,
                           float *d_residual_mm, double *d_acf, void *d_workspace, size_t workspace_bytes, void *stream)
{
    if (!d_depth_mm) return set_error(VISTAF_E_INVALID, "d_depth_mm is null");
    if (const char *why = table_inputs_refusal(d_contact_index, d_contacts, d_count, d_mm_per_px)) return set_error(VISTAF_E_INVALID, why);
    if (!d_textures) return set_error(VISTAF_E_INVALID, "d_textures is null");
    if (!d_residual_mm) return set_error(VISTAF_E_INVALID, "d_residual_mm is null");
    if (!d_acf) return set_error(VISTAF_E_INVALID, "d_acf is null");
    if (const char *why = texture_sizes_refusal(h, w, batch, "batch must be 1..2^19", max_contacts, max_lag)) return set_error(VISTAF_E_INVALID, why);
    if (!std::isfinite(depth_eps_mm)) return set_error(VISTAF_E_INVALID, "depth_eps_mm must be finite");
    if (!(eval_min_fraction >= 0.0) || !(eval_min_fraction < 1.0)) return set_error(VISTAF_E_INVALID, "eval_min_fraction must be in [0, 1)");
    if (form_degree < 0 || form_degree > 2) return set_error(VISTAF_E_INVALID, "form_degree must be 0, 1 or 2");
    if (!(acf_threshold > 0.0) || !(acf_threshold < 1.0)) return set_error(VISTAF_E_INVALID, "acf_threshold must be in (0, 1)");
    if (!(peak_min > 0.0) || !(peak_min < 1.0)) return set_error(VISTAF_E_INVALID, "peak_min must be in (0, 1)");
    if (((uintptr_t)d_contacts | (uintptr_t)d_mm_per_px | (uintptr_t)d_textures | (uintptr_t)d_acf) & 7)
        return set_error(VISTAF_E_INVALID, "d_contacts, d_mm_per_px, d_textures and d_acf must be 8-byte aligned");
    if (((uintptr_t)d_depth_mm | (uintptr_t)d_count | (uintptr_t)d_residual_mm) & 3)
        return set_error(VISTAF_E_INVALID, "d_depth_mm, d_count and d_residual_mm must be 4-byte aligned");
    TRY(workspace_ok(d_workspace, workspace_bytes, texture_scratch_bytes(batch, max_contacts, max_lag, nullptr), "vistaf_texture_workspace_bytes"));
    ScratchLayout S(d_workspace);
    const TextureBufs bf = texture_scratch(S, batch, max_contacts, max_lag);
    const int rows = batch * max_contacts;
    const size_t all = (size_t)batch * h * w, per = (size_t)TX_NT * 8;
    const int nfill = (int)std::min<size_t>((all + per - 1) / per, (size_t)TX_FILL_MAX);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_texture_form, dim3((unsigned)(rows + nfill)), dim3(TX_NT), 0, st, d_depth_mm, d_contact_index, d_contacts, d_count, depth_eps_mm,
                       eval_min_fraction, form_degree, h, w, batch, max_contacts, nfill, d_textures, d_residual_mm);
    hipLaunchKernelGGL(k_texture_stats, dim3((unsigned)rows), dim3(TX_NT), 0, st, d_contact_index, d_contacts, d_count, d_mm_per_px, d_residual_mm, h, w,
                       max_contacts, d_textures);
    hipLaunchKernelGGL(k_texture_acf, dim3((unsigned)(rows * (max_lag + 1))), dim3(TX_ACF_NT), 0, st, d_contact_index, d_contacts, d_count, d_textures,
                       d_residual_mm, h, w, max_contacts, max_lag, bf.C, bf.N);
    hipLaunchKernelGGL(k_texture_rows, dim3((unsigned)rows), dim3(64), 0, st, d_count, d_mm_per_px, bf.C, bf.N, acf_threshold, peak_min, max_contacts, max_lag,
                       d_textures, d_acf);
    return launch_ok("k_texture");
}

}  // extern "C"
