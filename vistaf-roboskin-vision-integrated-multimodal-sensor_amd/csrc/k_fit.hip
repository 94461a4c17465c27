// robust_polyfit2d on the GPU (shape_ftp.py:1086-1136), one 1024-thread workgroup per frame.
//
// IRLS: per iteration a weighted least-squares fit of z on [xn, yn, 1, xn^2, xn*yn, yn^2] (coordinates
// normalised to [-1,1] in float32), then r = z - A.coef, sigma = 1.4826*(median|r - median r| + 1e-6),
// w = 1/(1+(r/(c*sigma))^2).  The reference solves each step with float32 LAPACK lstsq on the N x 6
// system; here the 6x6 normal equations of the same float32-rounded rows (A*w, z*w) are accumulated
// in float64 by a block reduction and solved by Cholesky (condition number of the scaled design is
// O(10), so this is the more accurate of the two).  Medians are exact order statistics (select.hpp).
// Output plane = z - fit (float32, fit evaluated with the reference's operation order), NaN where z is NaN.
//
// Every pass walks the plane itself (z f32 + mask u8 = 5 B/px, coordinates from two LDS tables) with
// SEL_U / FIT_U independent loads in flight per thread: the passes are bound by memory round trips, not bytes.
#include <cstdio>
#include <algorithm>
#include <type_traits>
#include "kernels.hpp"
#ifdef VISTAF_DEBUG
// cycle sums of frame 0's fits (thread 0): [0] histogram clear, [1] histogram pass, [2] bucket search, [3] candidate collection, [4] sort,
// [5] second order statistic by a pass, [6] column sums, [7] reduction + solve, [8] load, [9] residual plane, [10] launches
namespace vf { __device__ unsigned long long g_fit_dbg[16]; __device__ unsigned long long g_fit_last; }
#define SEL_STAMP(i) do { if (blockIdx.x == 0 && threadIdx.x == 0) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); vf::g_fit_dbg[i] += t_ - vf::g_fit_last; vf::g_fit_last = t_; } } while (0)
// g_fit_m: over ALL frames, how many levels of a median chose a bucket of <= 64, <= 128, <= 256, <= 512, <= 1024, more keys (the last: another level)
namespace vf { __device__ unsigned int g_fit_m[6]; }
#define SEL_COUNT_M(m) do { if (threadIdx.x == 0) { const unsigned m_ = (m); atomicAdd(&vf::g_fit_m[m_ <= 64u ? 0 : m_ <= 128u ? 1 : m_ <= 256u ? 2 : m_ <= 512u ? 3 : m_ <= 1024u ? 4 : 5], 1u); } } while (0)
#define FIT_START() do { if (blockIdx.x == 0 && threadIdx.x == 0) { vf::g_fit_last = __builtin_amdgcn_s_memtime(); vf::g_fit_dbg[10]++; } } while (0)
#else
#define FIT_START() do { } while (0)
#endif
#include "select.hpp"
#include "fit_rules.hpp"
#include "chol.hpp"

namespace vf {

constexpr int FIT_TAB = 4096;     // LDS coordinate tables: xn[w] followed by yn[h] when w + h <= FIT_TAB
constexpr int FIT_YTAB = 1280;    // rows of the column variant's yn table (5 KB: the kernel stays at 44 KB of LDS, see k_inpaint_win.hip's first tier)
constexpr int FIT_U = 8;          // samples per thread in flight in the normal-equation pass

struct FitCtx {
    const float *z;
    const uint8_t *m;
    const float *tab;           // LDS: xn[0..w), yn[0..h)
    bool use_tab;               // false: divide on the fly (tables too small)
    int w;
    uint32_t magic;             // i / w == umulhi(i, magic) (0: plain division; chosen on the host)
    float cxf, cyf;
    int order;
    float coef[6];
    float med;                  // for the MAD pass
    int mode;                   // 0: key = r, 1: key = |r - med|
    __device__ inline void coords(int i, float &xn, float &yn) const
    {
        int y = magic ? (int)__umulhi((uint32_t)i, magic) : i / w, x = i - y * w;
        if (use_tab) { xn = tab[x]; yn = tab[w + y]; }
        else { xn = fit_coord(x, cxf); yn = fit_coord(y, cyf); }
    }
    // this kernel's own residual for the weights and medians: an fma chain, not fit_eval's order and not the column form
    __device__ inline float resid(float zz, float xn, float yn) const
    {
        float f = __fmul_rn(coef[0], xn);
        f = fmaf(coef[1], yn, f);
        f = __fadd_rn(f, coef[2]);
        if (order >= 2) {
            f = fmaf(coef[3], __fmul_rn(xn, xn), f);
            f = fmaf(coef[4], __fmul_rn(xn, yn), f);
            f = fmaf(coef[5], __fmul_rn(yn, yn), f);
        }
        return __fsub_rn(zz, f);
    }
    // z is the kernel's working copy of the plane: NaN wherever the pixel is not fitted (mask 0 or non-finite input)
    __device__ inline bool sample(int i, float &zz, float &xn, float &yn) const
    {
        zz = z[i];
        coords(i, xn, yn);
        return finitef(zz);
    }
    __device__ bool operator()(int i, uint32_t &key) const
    {
        float zz, xn, yn;
        bool ok = sample(i, zz, xn, yn);
        float r = resid(zz, xn, yn);
        if (mode) r = fabsf(__fsub_rn(r, med));
        key = f2key(r);
        return ok;
    }
};

__global__ __launch_bounds__(SEL_T) void k_robust_polyfit(const float *__restrict__ z_all, const uint8_t *__restrict__ mask_all, int order,
                                                          int iters, float c, int min_count, int min_mask_count, float *__restrict__ coef_out,
                                                          float *__restrict__ resid_all, int h, int w, uint32_t magic)
{
    __shared__ SelShared sh;
    __shared__ double s_part[16][27];
    __shared__ double s_sum[27];
    __shared__ float s_coef[6];
    __shared__ float s_tab[FIT_TAB];
    const size_t b = blockIdx.x;
    const int P = h * w, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int nc = order >= 2 ? 6 : 3;
    const float *z = z_all + b * (size_t)P;
    const uint8_t *m = mask_all + b * (size_t)P;
    const float cxf = fit_centre(w), cyf = fit_centre(h);
    const bool use_tab = w + h <= FIT_TAB;
    if (use_tab) {
        for (int i = tid; i < w + h; i += SEL_T)
            s_tab[i] = i < w ? fit_coord(i, cxf) : fit_coord(i - w, cyf);
    }
    sel_init(sh);
    __syncthreads();

    // Working copy in the output plane (it is only written at the very end): z where the pixel is fitted, NaN elsewhere.  The ~40 passes
    // of the fit then read 4 B per pixel instead of 5 (they run at HBM / Infinity-Cache speed: 256 frames do not fit the L2s).  Every
    // thread only ever touches the pixels tid, tid + 1024, ...: its own stores, so no fence is needed.
    float *zc = resid_all + b * (size_t)P;
    // the same pass counts the fitted pixels and finds the range of z (coefficients are still zero: r = z)
    uint32_t cntm = 0;
    SelRange rg;
    {
        const auto first = [&](int p, float zz, uint8_t mk) {
            const bool ok = mk && finitef(zz);
            cntm += mk != 0;
            zc[p] = ok ? zz : nanf32();
            if (ok) rg.add(f2key(zz));
        };
        int p = tid;
        for (; p + (FIT_U - 1) * SEL_T < P; p += FIT_U * SEL_T) {
            float zz[FIT_U];
            uint8_t mk[FIT_U];
#pragma unroll
            for (int u = 0; u < FIT_U; u++) { zz[u] = z[p + u * SEL_T]; mk[u] = m[p + u * SEL_T]; }
#pragma unroll
            for (int u = 0; u < FIT_U; u++) first(p + u * SEL_T, zz[u], mk[u]);
        }
        for (; p < P; p += SEL_T) first(p, z[p], m[p]);
    }
    FitCtx ctx;
    ctx.z = zc; ctx.m = m; ctx.tab = s_tab; ctx.use_tab = use_tab; ctx.w = w; ctx.magic = magic; ctx.cxf = cxf; ctx.cyf = cyf;
    ctx.order = order; ctx.med = 0.f; ctx.mode = 0;
    for (int i = 0; i < 6; i++) ctx.coef[i] = 0.f;

    // ---- number of fitted pixels (mask != 0 and finite z) and the range of z (coefficients are still zero: r = z)
    uint32_t n, zkmin, zkmax;
    __syncthreads();
    rg.reduce(sh.wsum, sh.red64, n, zkmin, zkmax, min_mask_count > 0, cntm);
    __syncthreads();
    const float zmin = key2f(zkmin), zmax = key2f(zkmax);
    const bool do_fit = fit_gate((int)n, (int)cntm, min_count, min_mask_count);

    float csig = 1.f;      // c * sigma of the previous iteration
    for (int it = 0; do_fit && it < iters; it++) {
        // ---- weighted normal equations
        double acc[27];
#pragma unroll
        for (int i = 0; i < 27; i++) acc[i] = 0.0;
        auto accumulate = [&](float zz, float xn, float yn) {
            float wt = 1.f;
            if (it > 0) {
                float u = __fdiv_rn(ctx.resid(zz, xn, yn), csig);
                wt = __fdiv_rn(1.0f, __fadd_rn(1.0f, __fmul_rn(u, u)));
            }
            float a[6];
            a[0] = __fmul_rn(xn, wt); a[1] = __fmul_rn(yn, wt); a[2] = wt;
            a[3] = __fmul_rn(__fmul_rn(xn, xn), wt); a[4] = __fmul_rn(__fmul_rn(xn, yn), wt); a[5] = __fmul_rn(__fmul_rn(yn, yn), wt);
            double zw = (double)__fmul_rn(zz, wt);
            int k = 0;
#pragma unroll
            for (int i = 0; i < 6; i++) {
#pragma unroll
                for (int j = i; j < 6; j++) { acc[k] = fma((double)a[i], (double)a[j], acc[k]); k++; }
            }
#pragma unroll
            for (int i = 0; i < 6; i++) acc[21 + i] = fma((double)a[i], zw, acc[21 + i]);
        };
        {
            int i = tid;
            for (; i + (FIT_U - 1) * SEL_T < P; i += FIT_U * SEL_T) {
                float zz[FIT_U], xn[FIT_U], yn[FIT_U];
                bool ok[FIT_U];
#pragma unroll
                for (int u = 0; u < FIT_U; u++) ok[u] = ctx.sample(i + u * SEL_T, zz[u], xn[u], yn[u]);
#pragma unroll
                for (int u = 0; u < FIT_U; u++)
                    if (ok[u]) accumulate(zz[u], xn[u], yn[u]);
            }
            for (; i < P; i += SEL_T) {
                float zz, xn, yn;
                if (ctx.sample(i, zz, xn, yn)) accumulate(zz, xn, yn);
            }
        }
        // 27 sums: DPP network inside each wave, then the 16 wave partials in a fixed order
#pragma unroll
        for (int i = 0; i < 27; i++) {
            double v = wave_sum(acc[i]);
            if (lane == 0) s_part[wid][i] = v;
        }
        __syncthreads();
        if (tid < 27) {
            double v = 0.0;
            for (int k = 0; k < 16; k++) v += s_part[k][tid];
            s_sum[tid] = v;
        }
        __syncthreads();
        if (tid == 0) {
            double A[6][6], rhs[6];
            int k = 0;
#pragma unroll
            for (int i = 0; i < 6; i++) {
#pragma unroll
                for (int j = i; j < 6; j++) { A[i][j] = s_sum[k]; A[j][i] = s_sum[k]; k++; }
            }
#pragma unroll
            for (int i = 0; i < 6; i++) rhs[i] = s_sum[21 + i];
            bool ok = nc == 6 ? chol_solve<6>(A, rhs) : chol_solve<3>(A, rhs);
#pragma unroll
            for (int i = 0; i < 6; i++) s_coef[i] = (ok && i < nc) ? (float)rhs[i] : 0.f;
        }
        __syncthreads();
        for (int i = 0; i < 6; i++) ctx.coef[i] = s_coef[i];
        if (it == iters - 1) break;   // the weights of the last iteration are never used upstream
        // ---- the next step's scale from the two medians; their key ranges come from bounds, not from passes (fit_rules.hpp)
        ctx.mode = 0;
        const FitKeys kr = fit_resid_range(ctx.coef, zmin, zmax);
        float medr = block_median(ctx, P, sh, n, kr.kmin, kr.kmax);
        __syncthreads();
        ctx.med = medr; ctx.mode = 1;
        const FitKeys ka = fit_mad_range(kr, medr);
        float mad = block_median(ctx, P, sh, n, ka.kmin, ka.kmax);
        __syncthreads();
        ctx.mode = 0;
        csig = fit_csig(c, mad);
    }
    if (tid < 6) coef_out[b * 6 + tid] = do_fit ? ctx.coef[tid] : 0.f;
    // residual plane: z - fit, fit evaluated as eval_poly2d does (shape_ftp.py:1093-1097, :1132-1135)
    float *out = resid_all + b * (size_t)P;
    for (int p = tid; p < P; p += SEL_T) {
        float zz = z[p];
        float fit = 0.f;
        if (do_fit) {
            float xn, yn;
            ctx.coords(p, xn, yn);
            fit = fit_eval(ctx.coef, order, xn, yn);
        }
        out[p] = __fsub_rn(zz, fit);
    }
}

// lane l's value of v as a wave-uniform value (two v_readlane)
__device__ inline double readlane_f64(double v, int l)
{
    const unsigned long long r = (unsigned long long)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)r, l), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(r >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Register-resident, column-owning variant for the batched frame sizes (w <= 1024, h / floor(1024 / w64) <= 64; 224 x 224: RP = 56).
//
// Thread t owns ONE image column x (threads run along x, padded to a multiple of 64 so that every wave lies inside one row group) and
// the rows y = grp + groups * k, k < RP, of it; its samples stay in RP VGPRs for the whole fit (NaN = not fitted).  The ~35 passes of an
// IRLS fit then cost neither memory traffic (the first variants walked a working copy of the plane: 5.3 GB of HBM traffic per batch of
// 256 for 0.35 GB of input and output) nor coordinate arithmetic: with x fixed per thread and y uniform per wave,
//     fit(x, y) = (c0 x + c2 + c3 x^2) + y (c1 + c4 x) + c5 y^2 = A_t + y B_t + C_y        -- one fma and one add per sample,
// and the normal equations are accumulated as the 8 per-thread column sums  P_b = sum_k w^2 y^b (b = 0..4),  Q_b = sum_k w^2 z y^b
// (b = 0..2) in float64, multiplied by the powers of x once per iteration and thread:  (A^T W^2 A)_ij = sum x^a y^b w^2  over the 15
// monomials of degree <= 4, rhs_i likewise.  Same minimisation as the reference's lstsq on (A * w, z * w) (:1119-1121); float64 sums of
// exact products instead of float32-rounded rows, i.e. closer to the exact solution than either LAPACK's float32 SVD or the first variant.
// Medians are exact order statistics as before.  The residual plane is evaluated with eval_poly2d's own operation order (:1093-1097).
// GT: row groups as a compile-time constant (0: the runtime value).  With a constant stride every yn read is one LDS read at an immediate
// offset from a single base; with a runtime stride the RP row addresses of a pass are scalar values of their own (hundreds of SGPR spills).
//
// Two compile-time flags give the window kernel and the chained launches the same body (the plain kernels are the instances with both off, and
// their code is what it was before the flags existed):
// WIN    A thread keeps RP slots of its unit starting at its OWN first slot u0, not at slot 0: it reads the mask bytes of all
//        need = ceil(h / groups) <= fit_plain_rp(RP) rows of its unit first (a 64-bit map per lane), takes u0 = first mask row and
//        extent = last - first + 1 from the map, and the workgroup writes need_flag[b] = (any extent > RP).  A flagged frame returns with
//        nothing else written (the retry kernel runs it); otherwise the thread's rows are grp + groups * (u0 + u), u < RP, which hold every
//        mask pixel of the unit, in ascending order, in the same lane of the same wave as in the plain kernel: the same sums, the same keys.
//        u0 is clamped to need - RP, so the window never leaves the unit and the yn table needs no more rows.
// PASSES The fit runs ex.npass (1 or 2) times as a loop over a parameter list {order, min_mask_count, output plane}: pass 1 fits what pass 0 has
//        stored, from the registers (the stored float where the mask is set, NaN elsewhere), under the same mask and window.
struct FitChain {
    int *need_flag;             // WIN: [B], written 0 / 1 for every frame.  !WIN && PASSES: read, frames with 0 return at once (null: none does)
    int npass;                  // 1 or 2
    int order2, min_mask_count2;
    float *resid2_all;          // pass 1's output plane (pass 1's input is resid_all, pass 0's output)
};
constexpr int fit_plain_rp(int rp) { return rp == 16 ? 32 : rp == 32 ? 48 : rp == 48 ? 56 : 64; }      // the plain instance a window of rp slots stands in for
template <int RP, int NT, int GT, bool WIN = false, bool PASSES = false>
__device__ __attribute__((always_inline)) inline void robust_polyfit_col_body(const float *__restrict__ z_all, const uint8_t *__restrict__ mask_all, int order,
                                                              int iters, float c, int min_count, int min_mask_count, float *__restrict__ coef_out,
                                                              float *__restrict__ resid_all, int h, int w, int cols_pad, int groups_rt,
                                                              const FitChain ex = FitChain())
{
    // everything below that depends on the workgroup size takes it from NT (block reductions through 16-entry scratch arrays, NT / 64
    // partial sums, the selection's NT-strided loops): the launcher must start exactly NT threads and derive the row groups from NT
    static_assert(NT % 64 == 0 && NT >= 256 && NT / 64 <= 16, "block_sum / block_min / block_max scratch holds 16 waves");
    static_assert(RP >= 1 && RP <= 128, "rows per thread live in registers");
    static_assert(GT >= 0 && (GT == 0 || (RP - 1) * GT + GT + 15 < FIT_YTAB), "row table");
    const int groups = GT > 0 ? GT : groups_rt;
    // select.hpp's SELF: the window and chained instances run the self-cleaning levels; the plain instances keep the levels' former
    // bookkeeping, with which the compiler spills less than the parent build (k_robust_polyfit_col<56,4>: 39 spills for 40, with SELF 46)
    constexpr bool SF = WIN || PASSES;
    FIT_START();
    __shared__ SelShared sh;
    __shared__ double s_part[NT / 64][21];
    __shared__ float s_coef[6];
    __shared__ float s_yn[FIT_YTAB];
    const size_t b = blockIdx.x;
    const int P = h * w, tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    int nc = order >= 2 ? 6 : 3;
    const float *z = z_all + b * (size_t)P;
    const uint8_t *m = mask_all + b * (size_t)P;
    if constexpr (PASSES && !WIN) {
        if (ex.need_flag && ex.need_flag[b] == 0) return;                         // the window kernel has done this frame
    }
    const float cxf = fit_centre(w), cyf = fit_centre(h);
    for (int i = tid; i < FIT_YTAB; i += NT) s_yn[i] = fit_coord(i, cyf);       // rows >= h: only read for samples that are NaN
    if constexpr (SF) sel_init<NT>(sh);                                         // the barriers around the first range reduction come before the first median
    const int col = tid % cols_pad, grp = __builtin_amdgcn_readfirstlane(tid / cols_pad);   // uniform inside a wave (cols_pad % 64 == 0)
    const bool owner = col < w && grp < groups;
    const float xn = fit_coord(col, cxf);
    const float qnan = nanf32();
    // ---- load this thread's column samples; count fitted / masked pixels, range of z
    float zr[RP];
    uint32_t cntm = 0;
    SelRange rg;
    // WIN / PASSES: the unit's mask as a bit per slot, the thread's first slot, its row and its 32-bit element offset in the frame (P < 2^31),
    // the offset from one slot to the next, and the rows of a unit
    unsigned long long mbits = 0;
    int u0 = 0, y0 = grp;
    const uint32_t gw = (uint32_t)(groups * w);
    const int need = (h + groups - 1) / groups;
    if constexpr (WIN) {
        constexpr int RPF = fit_plain_rp(RP), MU = 16;
        static_assert(RPF <= 64, "one bit per slot");
        const uint32_t mo = (uint32_t)(grp * w + col);
#pragma unroll
        for (int a = 0; a < RPF; a += MU) {
            uint8_t mk[MU];
#pragma unroll
            for (int v = 0; v < MU; v++) {
                const int u = a + v;
                if (u < RPF) mk[v] = (owner && grp + groups * u < h) ? m[mo + (uint32_t)u * gw] : (uint8_t)0;
            }
#pragma unroll
            for (int v = 0; v < MU; v++) {
                const int u = a + v;
                if (u < RPF) mbits |= (unsigned long long)(mk[v] != 0) << u;
            }
        }
        const int first = mbits ? __builtin_ctzll(mbits) : 0, last = mbits ? 63 - __builtin_clzll(mbits) : -1;
        const int over = __syncthreads_or(last - first + 1 > RP);
        if (tid == 0) ex.need_flag[b] = over ? 1 : 0;
        if (over) return;
        u0 = max(0, min(first, need - RP));
        y0 = grp + groups * u0;
        mbits >>= u0;                                                             // bit u: slot u of the window
    }
    const uint32_t o0 = (uint32_t)(y0 * w + col);
    if constexpr (WIN || PASSES) {
        constexpr int LU = 8;
#pragma unroll
        for (int a = 0; a < RP; a += LU) {
            uint8_t mk[LU];
#pragma unroll
            for (int v = 0; v < LU; v++) {
                const int u = a + v;
                if (u < RP) {
                    const bool in = owner && y0 + groups * u < h;
                    zr[u] = in ? z[o0 + (uint32_t)u * gw] : qnan;
                    if constexpr (!WIN) mk[v] = in ? m[o0 + (uint32_t)u * gw] : (uint8_t)0;
                }
            }
            if constexpr (!WIN) {
#pragma unroll
                for (int v = 0; v < LU; v++) {
                    const int u = a + v;
                    if (u < RP) mbits |= (unsigned long long)(mk[v] != 0) << u;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < RP; u++) zr[u] = (mbits >> u & 1) ? zr[u] : qnan;   // the fitted-pixel test itself is the pass loop's
    } else {
        constexpr int LU = 8;
        uint8_t mk[LU];
#pragma unroll
        for (int u0 = 0; u0 < RP; u0 += LU) {
#pragma unroll
            for (int v = 0; v < LU; v++) {
                const int u = u0 + v;
                if (u < RP) {
                    const int y = grp + groups * u;
                    const bool in = owner && y < h;
                    zr[u] = in ? z[(size_t)y * w + col] : qnan;
                    mk[v] = in ? m[(size_t)y * w + col] : (uint8_t)0;
                }
            }
#pragma unroll
            for (int v = 0; v < LU; v++) {
                const int u = u0 + v;
                if (u < RP) {
                    const float zz = zr[u];
                    const bool ok = mk[v] && finitef(zz);
                    cntm += mk[v] != 0;
                    zr[u] = ok ? zz : qnan;
                    if (ok) rg.add(f2key(zz));
                }
            }
        }
    }
    // the fits of this launch: one, or with PASSES ex.npass of them over {order, min_mask_count, zsrc -> out}
    const int npass = PASSES ? ex.npass : 1;
    const float *zsrc = z;                       // what the residual phase reads for the pixels that are not fitted
    float *out = nullptr;
#pragma unroll 1
    for (int pass = 0;; pass++) {
    if constexpr (PASSES) {
        if (pass) { order = ex.order2; nc = order >= 2 ? 6 : 3; min_mask_count = ex.min_mask_count2; zsrc = out; out = ex.resid2_all + b * (size_t)P; }
        else out = resid_all + b * (size_t)P;
        // count, range and finiteness from the registers: the first pass's loaded samples, or what the pass before has stored
        cntm = (uint32_t)__builtin_popcountll(mbits);
        rg = SelRange();
        // (below, mb / oo / gg: opaque copies per pass -- as invariants of the pass loop the RP mask tests and element offsets would be
        // hoisted out of it and kept live next to the samples, like the row coordinates of `each`)
#pragma unroll
        for (int u = 0; u < RP; u++) {
            const float zz = zr[u];
            const bool ok = finitef(zz);
            zr[u] = ok ? zz : qnan;
            if (ok) rg.add(f2key(zz));
        }
    }
    __syncthreads();
    uint32_t n, zkmin, zkmax;
    rg.reduce(sh.wsum, sh.red64, n, zkmin, zkmax, min_mask_count > 0, cntm);
    __syncthreads();
    const float zmin = key2f(zkmin), zmax = key2f(zkmax);
    const bool do_fit = fit_gate((int)n, (int)cntm, min_count, min_mask_count);
    SEL_STAMP(8);

    float coef[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float At = 0.f, Bt = 0.f;          // fit(x, y) = At + yn * Bt + c5 * yn^2 for this thread's column
    float med = 0.f;
    int mode = 0;                      // 0: key = r, 1: key = |r - med|
    // residual of sample u (its row is uniform across the wave: the yn read is a broadcast).  g0: an opaque copy of the row group made at
    // the start of every pass -- as loop invariants the RP row coordinates would be hoisted out of the IRLS loop and kept live next to
    // the samples (hundreds of spills)
    auto resid_of = [&](int g0, int u, float zz) -> float {
        const float yn = s_yn[g0 + groups * u];                      // < FIT_YTAB (checked by the launcher)
        return __fsub_rn(zz, fit_col_eval(At, Bt, coef[5], yn));
    };
    auto each = [&](auto body) {
        int g0 = y0;
        if constexpr (WIN) asm volatile("" : "+v"(g0));      // a lane's own first row
        else asm volatile("" : "+s"(g0));
#pragma unroll
        for (int u = 0; u < RP; u++) {
            // the test is on the RESIDUAL (NaN for a sample that is not fitted), not on the sample: "is zr[u] finite" is invariant across
            // the IRLS loop, so the compiler kept all RP answers as exec masks in SGPRs (450 of them spilled to VGPR lanes and read
            // back with two v_readlane per sample and sweep)
            float r = resid_of(g0, u, zr[u]);
            if (finitef(r)) {
                if (mode) r = fabsf(__fsub_rn(r, med));
                body(f2key(r));
            }
        }
    };

    float csig = 1.f;
    // one weighted least-squares step with NC = 3 (order 1) or 6 coefficients: sweep, reduction, solve.  An order-1 step accumulates and
    // reduces only the nine sums its 3 x 3 system reads (the monomials of degree <= 2 from P_0..P_2, x Q_0, Q_1, Q_0), each formed by the
    // same operations in the same order as in the order-2 step.
    auto irls_step = [&](auto ncc, int it) {
        constexpr int NC = decltype(ncc)::value, DEG = NC == 6 ? 4 : 2;
        constexpr int NM = (DEG + 1) * (DEG + 2) / 2, NV = NM + NC;           // monomial sums, all sums: 15 + 6 or 6 + 3
        // ---- column sums P_b = sum w^2 yn^b (b = 0..DEG), Q_b = sum w^2 z yn^b (b = 0..DEG / 2), float64
        double Pb[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, Qb[3] = {0.0, 0.0, 0.0};
        const float inv_csig = __fdiv_rn(1.0f, csig);
        int g0 = y0;
        if constexpr (WIN) asm volatile("" : "+v"(g0));      // a lane's own first row
        else asm volatile("" : "+s"(g0));
#pragma unroll
        for (int u = 0; u < RP; u++) {
            const float zz = zr[u];
            if (finitef(__fmul_rn(zz, inv_csig))) {               // (finite exactly when zz is; not invariant across the IRLS loop, see `each`)
                float wt = 1.f;
                if (it > 0) {
                    wt = fit_cauchy(resid_of(g0, u, zz), inv_csig);
                }
                const double yd = (double)s_yn[g0 + groups * u];
                const double w2 = (double)wt * (double)wt;
                const double t1 = w2 * yd, t2 = t1 * yd;
                Pb[0] += w2; Pb[1] += t1; Pb[2] += t2;
                const double zw = w2 * (double)zz;
                Qb[0] += zw; Qb[1] = fma(zw, yd, Qb[1]);
                if constexpr (NC == 6) {
                    const double t3 = t2 * yd, t4 = t3 * yd;
                    Pb[3] += t3; Pb[4] += t4;
                    Qb[2] = fma(zw, yd * yd, Qb[2]);
                }
            }
        }
        // the monomial sums m[a][b] = sum x^a P_b (a + b <= DEG) and the right-hand sides, reduced over the workgroup
        double vs[NV];
        {
            const double x1 = (double)xn, x2 = x1 * x1, x3 = x2 * x1, x4 = x2 * x2;
            const double xp[5] = {1.0, x1, x2, x3, x4};
            int k = 0;
#pragma unroll
            for (int bb = 0; bb <= DEG; bb++)
#pragma unroll
                for (int aa = 0; aa + bb <= DEG; aa++) vs[k++] = xp[aa] * Pb[bb];     // k = fit_mono(aa, bb, DEG)
            vs[NM + 0] = x1 * Qb[0]; vs[NM + 1] = Qb[1]; vs[NM + 2] = Qb[0];
            if constexpr (NC == 6) { vs[NM + 3] = x2 * Qb[0]; vs[NM + 4] = x1 * Qb[1]; vs[NM + 5] = Qb[2]; }
        }
        SEL_STAMP(6);
#pragma unroll
        for (int i = 0; i < NV; i++) {
            const double v = wave_sum(vs[i]);
            if (lane == 0) s_part[wid][i] = v;
        }
        __syncthreads();
        SEL_STAMP(11);
        // Wave 0 alone finishes the step: lane i < NV adds the NT / 64 partials of sum i in their fixed order, the sums reach the solver
        // as scalars through v_readlane (no second LDS round trip and no barrier in between), and every lane of the wave runs the same
        // solve on them -- as fast as one lane would.
        if (wid == 0) {
            double sv = 0.0;
            const int si = lane < NV ? lane : NV - 1;
            for (int k = 0; k < NT / 64; k++) sv += s_part[k][si];
            double S[NV];
#pragma unroll
            for (int i = 0; i < NV; i++) S[i] = readlane_f64(sv, i);
            SEL_STAMP(12);
            double A[6][6], rhs[6];
            fit_assemble<NC, DEG>(S, A, rhs);
            const bool ok = chol_solve<NC>(A, rhs);
            if (lane == 0) {
#pragma unroll
                for (int i = 0; i < 6; i++) s_coef[i] = (ok && i < NC) ? (float)rhs[i] : 0.f;
            }
        }
        SEL_STAMP(13);
        __syncthreads();
        for (int i = 0; i < 6; i++) coef[i] = s_coef[i];
        const FitCol ct = fit_col_terms(coef, xn);
        At = ct.At; Bt = ct.Bt;
        SEL_STAMP(7);
    };
    for (int it = 0; do_fit && it < iters; it++) {
        if (nc == 6) irls_step(std::integral_constant<int, 6>(), it);
        else irls_step(std::integral_constant<int, 3>(), it);
        if (it == iters - 1) break;   // the weights of the last iteration are never used upstream
        // ---- the next step's scale from the two medians
        mode = 0;
        const FitKeys kr = fit_resid_range(coef, zmin, zmax);
        const float medr = block_median_each<NT, SF>(each, sh, n, kr.kmin, kr.kmax);
        __syncthreads();
        med = medr; mode = 1;
        const FitKeys ka = fit_mad_range(kr, medr);
        const float mad = block_median_each<NT, SF>(each, sh, n, ka.kmin, ka.kmax);
        __syncthreads();
        mode = 0;
        csig = fit_csig(c, mad);
    }
    if (tid < 6) coef_out[b * 6 + tid] = do_fit ? coef[tid] : 0.f;
    // residual plane: z - fit over the WHOLE plane, unfitted pixels included (fit evaluated as eval_poly2d does, :1093-1097, :1132-1135)
    if constexpr (!PASSES) out = resid_all + b * (size_t)P;
    if constexpr (WIN || PASSES) {
        if (owner) {
            // as below, through the 32-bit offsets; a chained launch keeps what it stores where the mask is set: the next pass's samples
            unsigned long long mb = mbits;
            uint32_t oo = o0, gg = gw;
            int yy = y0;
            asm volatile("" : "+v"(mb), "+v"(oo), "+s"(gg), "+v"(yy));
#pragma unroll
            for (int u = 0; u < RP; u++) {
                if (yy + groups * u < h && !finitef(zr[u])) zr[u] = zsrc[oo + (uint32_t)u * gg];
            }
#pragma unroll
            for (int u = 0; u < RP; u++) {
                const int y = yy + groups * u;
                if (y < h) {
                    const float fit = do_fit ? fit_eval(coef, order, xn, s_yn[y]) : 0.f;
                    const float o = __fsub_rn(zr[u], fit);
                    out[oo + (uint32_t)u * gg] = o;
                    if constexpr (PASSES) zr[u] = (mb >> u & 1) ? o : qnan;
                }
            }
            if constexpr (WIN) {
                // the need - RP rows of the unit outside the window: slots (u0 + RP + j) mod need, none of them under the mask
                constexpr int NO = fit_plain_rp(RP) - RP;
                float zo[NO];
                int yo[NO];
#pragma unroll
                for (int j = 0; j < NO; j++) {
                    int s = u0 + RP + j;
                    if (s >= need) s -= need;
                    yo[j] = (j < need - RP && grp + groups * s < h) ? grp + groups * s : -1;
                    zo[j] = yo[j] >= 0 ? zsrc[(uint32_t)(yo[j] * w + col)] : 0.f;
                }
#pragma unroll
                for (int j = 0; j < NO; j++) {
                    if (yo[j] >= 0) {
                        const float fit = do_fit ? fit_eval(coef, order, xn, s_yn[yo[j]]) : 0.f;
                        out[(uint32_t)(yo[j] * w + col)] = __fsub_rn(zo[j], fit);
                    }
                }
            }
        }
    } else {
    if (owner) {
        // fitted pixels still sit in the registers; the others (masked out or NaN upstream) are read again -- all of those loads first, in
        // batches of independent requests (one dependent load per row made this loop a tenth of the kernel), then arithmetic and stores
#pragma unroll
        for (int u = 0; u < RP; u++) {
            const int y = grp + groups * u;
            if (y < h && !finitef(zr[u])) zr[u] = z[(size_t)y * w + col];
        }
#pragma unroll
        for (int u = 0; u < RP; u++) {
            const int y = grp + groups * u;
            if (y < h) {
                const float fit = do_fit ? fit_eval(coef, order, xn, s_yn[y]) : 0.f;
                out[(size_t)y * w + col] = __fsub_rn(zr[u], fit);
            }
        }
    }
    }
    SEL_STAMP(9);
    if constexpr (!PASSES) break;
    else if (pass + 1 >= npass) break;
    }       // pass
}

#ifdef VISTAF_DEBUG
void fit_debug_dump()
{
    unsigned long long d[16];
    if (hipMemcpyFromSymbol(d, HIP_SYMBOL(g_fit_dbg), sizeof(d)) != hipSuccess) return;
    printf("[fit dbg] frame 0, %llu launches so far, cycle sums: load %llu | column sums %llu | reduce+solve %llu | hist clear %llu | hist pass %llu | bucket search %llu | "
           "collect %llu | sort %llu | second statistic pass %llu | residual plane %llu || of reduce+solve: wave sums %llu | partials %llu | solve %llu | rest in [reduce+solve]\n", d[10], d[8], d[6], d[7], d[0], d[1], d[2], d[3], d[4], d[5], d[9], d[11], d[12], d[13]);
    unsigned int mm[6];
    if (hipMemcpyFromSymbol(mm, HIP_SYMBOL(g_fit_m), sizeof(mm)) != hipSuccess) return;
    printf("[fit dbg] all frames, chosen buckets by count: <=64 %u | <=128 %u | <=256 %u | <=512 %u | <=1024 %u | more %u\n", mm[0], mm[1], mm[2], mm[3], mm[4], mm[5]);
}
#endif

#define VF_FIT_ARGS const float *__restrict__ z_all, const uint8_t *__restrict__ mask_all, int order, int iters, float c, int min_count, int min_mask_count, \
                    float *__restrict__ coef_out, float *__restrict__ resid_all, int h, int w, int cols_pad, int groups
#define VF_FIT_PASS z_all, mask_all, order, iters, c, min_count, min_mask_count, coef_out, resid_all, h, w, cols_pad, groups
template <int RP, int GT>
__global__ __launch_bounds__(SEL_T) void k_robust_polyfit_col(VF_FIT_ARGS) { robust_polyfit_col_body<RP, SEL_T, GT>(VF_FIT_PASS); }
// The window kernel (see robust_polyfit_col_body: WIN, PASSES) and the kernel behind it: the chained body at the plain RP for the frames the
// window kernel has flagged in need_flag (every frame when need_flag is null).  npass = 1: one fit, the second parameter set is not read.
#define VF_FIT_CHAIN_ARGS int order2, int min_mask_count2, float *resid2_all, int npass, int *need_flag
#define VF_FIT_CHAIN_PASS FitChain{need_flag, npass, order2, min_mask_count2, resid2_all}
template <int RP, int GT>
__global__ __launch_bounds__(SEL_T) void k_robust_polyfit_colwin(VF_FIT_ARGS, VF_FIT_CHAIN_ARGS) { robust_polyfit_col_body<RP, SEL_T, GT, true, true>(VF_FIT_PASS, VF_FIT_CHAIN_PASS); }
template <int RP, int GT>
__global__ __launch_bounds__(SEL_T) void k_robust_polyfit_col_retry(VF_FIT_ARGS, VF_FIT_CHAIN_ARGS) { robust_polyfit_col_body<RP, SEL_T, GT, false, true>(VF_FIT_PASS, VF_FIT_CHAIN_PASS); }
#undef VF_FIT_CHAIN_ARGS
#undef VF_FIT_CHAIN_PASS
#undef VF_FIT_ARGS
#undef VF_FIT_PASS

// Which of the ten kernels fits a batch of B frames of h x w (big: the caller holds scratch for the k_big.hip chain).  The one place
// where the choice is made: the launcher below switches on the result, the tests read it through vistaf_ftp_test_polyfit.
// Column kernels: thread t owns one column padded to 64 (cols_pad), the 1024 threads form `groups` row groups, a thread keeps
// need = ceil(h / groups) samples in registers (<= 64) and the yn table must hold h + groups * 16 rows.
int polyfit_variant(int B, int h, int w, bool big, int *cols_pad_out, int *groups_out)
{
    if (big && big_frames(B, h * w)) return FITV_BIG;
    constexpr int NT = SEL_T;                      // threads of every column kernel (robust_polyfit_col_body's NT): the row groups follow from it
    const int cols_pad = ((w + 63) / 64) * 64;
    const int groups = cols_pad <= NT ? std::min(NT / cols_pad, h) : 0;
    const int need = groups ? (h + groups - 1) / groups : 1 << 30;
    if (cols_pad_out) *cols_pad_out = cols_pad;
    if (groups_out) *groups_out = groups;
    if (need <= 64 && h + groups * 16 <= FIT_YTAB) {
        if (groups == 4 && need > 32) return need <= 48 ? FITV_COL48_G4 : need <= 56 ? FITV_COL56_G4 : FITV_COL64_G4;
        return need <= 16 ? FITV_COL16 : need <= 32 ? FITV_COL32 : need <= 48 ? FITV_COL48 : need <= 56 ? FITV_COL56 : FITV_COL64;
    }
    // i / w == umulhi(i, magic) for every i < h * w as long as h * w * w < 2^32
    return (unsigned long long)h * w * w < 0x100000000ull ? FITV_GENERIC : FITV_GENERIC_DIV;
}

// min_count: 200 fitted pixels upstream (:1103); min_mask_count: 500 mask pixels for the debug_ramp call (shape_ftp.py:1364-1366), else 0
void launch_robust_polyfit(const float *z, const uint8_t *mask, int order, int iters, float c, int min_count, int min_mask_count, float *coef_out,
                           float *resid_out, int B, int h, int w, hipStream_t st, void *big_scratch)
{
    int cols_pad = 0, groups = 0;                                // of the column kernels, as polyfit_variant worked them out
    const int variant = polyfit_variant(B, h, w, big_scratch != nullptr, &cols_pad, &groups);
#define VF_FIT_COL(KERNEL, NTV, GR) hipLaunchKernelGGL(KERNEL, dim3(B), dim3(NTV), 0, st, z, mask, order, iters, c, min_count, min_mask_count, coef_out, resid_out, h, w, cols_pad, GR)
    switch (variant) {
    case FITV_BIG:                                               // large frames: every sweep over all pixels of the batch (k_big.hip)
        launch_robust_polyfit_big(z, mask, order, iters, c, min_count, min_mask_count, coef_out, resid_out, B, h, w, big_scratch, st);
        break;
    case FITV_COL48_G4: VF_FIT_COL((k_robust_polyfit_col<48, 4>), SEL_T, 4); break;
    case FITV_COL56_G4: VF_FIT_COL((k_robust_polyfit_col<56, 4>), SEL_T, 4); break;
    case FITV_COL64_G4: VF_FIT_COL((k_robust_polyfit_col<64, 4>), SEL_T, 4); break;
    case FITV_COL16: VF_FIT_COL((k_robust_polyfit_col<16, 0>), SEL_T, groups); break;
    case FITV_COL32: VF_FIT_COL((k_robust_polyfit_col<32, 0>), SEL_T, groups); break;
    case FITV_COL48: VF_FIT_COL((k_robust_polyfit_col<48, 0>), SEL_T, groups); break;
    case FITV_COL56: VF_FIT_COL((k_robust_polyfit_col<56, 0>), SEL_T, groups); break;
    case FITV_COL64: VF_FIT_COL((k_robust_polyfit_col<64, 0>), SEL_T, groups); break;
    case FITV_GENERIC:
        hipLaunchKernelGGL(k_robust_polyfit, dim3(B), dim3(SEL_T), 0, st, z, mask, order, iters, c, min_count, min_mask_count, coef_out, resid_out, h, w,
                           (uint32_t)(0x100000000ull / (unsigned)w) + 1u);
        break;
    default:                                                     // FITV_GENERIC_DIV: magic 0, plain division
        hipLaunchKernelGGL(k_robust_polyfit, dim3(B), dim3(SEL_T), 0, st, z, mask, order, iters, c, min_count, min_mask_count, coef_out, resid_out, h, w, 0u);
        break;
    }
#undef VF_FIT_COL
}

// The window instance of a plain column variant: the ladder step below it with the same GT, or -1 (the smallest step, the generic and the
// big variants have none).  A frame takes it when no thread's mask rows span more slots than the instance keeps.
int polyfit_window_of(int plain_variant)
{
    switch (plain_variant) {
    case FITV_COL32: return FITV_WIN16;
    case FITV_COL48: return FITV_WIN32;
    case FITV_COL56: return FITV_WIN48;
    case FITV_COL64: return FITV_WIN56;
    case FITV_COL48_G4: return FITV_WIN32_G4;
    case FITV_COL56_G4: return FITV_WIN48_G4;
    case FITV_COL64_G4: return FITV_WIN56_G4;
    default: return -1;
    }
}
int polyfit_window_variant(int B, int h, int w, bool big) { return polyfit_window_of(polyfit_variant(B, h, w, big)); }

namespace {
using FitChainKernel = void (*)(const float *, const uint8_t *, int, int, float, int, int, float *, float *, int, int, int, int, int, int, float *, int, int *);
struct FitWindowKernels { FitChainKernel win, retry; int gt; };     // retry: the chained body at the plain variant's RP
FitWindowKernels fit_window_kernels(int plain_variant)
{
    switch (plain_variant) {
    case FITV_COL16: return {nullptr, k_robust_polyfit_col_retry<16, 0>, 0};
    case FITV_COL32: return {k_robust_polyfit_colwin<16, 0>, k_robust_polyfit_col_retry<32, 0>, 0};
    case FITV_COL48: return {k_robust_polyfit_colwin<32, 0>, k_robust_polyfit_col_retry<48, 0>, 0};
    case FITV_COL56: return {k_robust_polyfit_colwin<48, 0>, k_robust_polyfit_col_retry<56, 0>, 0};
    case FITV_COL64: return {k_robust_polyfit_colwin<56, 0>, k_robust_polyfit_col_retry<64, 0>, 0};
    case FITV_COL48_G4: return {k_robust_polyfit_colwin<32, 4>, k_robust_polyfit_col_retry<48, 4>, 4};
    case FITV_COL56_G4: return {k_robust_polyfit_colwin<48, 4>, k_robust_polyfit_col_retry<56, 4>, 4};
    case FITV_COL64_G4: return {k_robust_polyfit_colwin<56, 4>, k_robust_polyfit_col_retry<64, 4>, 4};
    default: return {nullptr, nullptr, 0};
    }
}
}  // namespace

// One fit, or with `second` two chained ones (the second fits the first's output plane under the same mask), through the window kernel.
// window: Tiers::fit_window.  force: 0 the dispatch -- with `window` and a column variant the window kernel, then the kernel behind it for the
// frames flagged in need_flag ([B] ints; a column variant without a window instance runs the chained body alone); otherwise the plain launches,
// two of them for a chain -- FIT_WINDOW_ONLY the window kernel alone (the caller has checked polyfit_window_variant), FIT_PLAIN the plain
// launches.  Returns the FitVariant of the first kernel launched.
int launch_robust_polyfit_window(const float *z, const uint8_t *mask, int order, int iters, float c, int min_count, int min_mask_count, float *coef_out,
                                 float *resid_out, const FitSecond *second, int *need_flag, bool window, int force, int B, int h, int w, hipStream_t st,
                                 void *big_scratch)
{
    int cols_pad = 0, groups = 0;
    const int variant = polyfit_variant(B, h, w, big_scratch != nullptr, &cols_pad, &groups);
    const FitWindowKernels k = fit_window_kernels(variant);
    if (force == FIT_PLAIN || (force == 0 && (!window || !k.retry))) {
        launch_robust_polyfit(z, mask, order, iters, c, min_count, min_mask_count, coef_out, resid_out, B, h, w, st, big_scratch);
        if (second) launch_robust_polyfit(resid_out, mask, second->order, iters, c, min_count, second->min_mask_count, coef_out, second->resid_out, B, h, w, st, big_scratch);
        return variant;
    }
    const int gr = k.gt ? k.gt : groups;
    const int order2 = second ? second->order : order, mmc2 = second ? second->min_mask_count : 0, npass = second ? 2 : 1;
    float *resid2 = second ? second->resid_out : nullptr;
#define VF_FIT_CHAIN(KERNEL, NEED) hipLaunchKernelGGL(KERNEL, dim3(B), dim3(SEL_T), 0, st, z, mask, order, iters, c, min_count, min_mask_count, coef_out, resid_out, h, w, cols_pad, gr, \
                                                      order2, mmc2, resid2, npass, NEED)
    if (!k.win) {                                                // the smallest ladder step: no window, the chained body for every frame
        VF_FIT_CHAIN(k.retry, (int *)nullptr);
        return variant;
    }
    VF_FIT_CHAIN(k.win, need_flag);
    if (force != FIT_WINDOW_ONLY) VF_FIT_CHAIN(k.retry, need_flag);
#undef VF_FIT_CHAIN
    return polyfit_window_of(variant);
}

}  // namespace vf
