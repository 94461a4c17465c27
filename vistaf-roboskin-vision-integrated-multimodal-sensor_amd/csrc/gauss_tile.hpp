// The separable Gaussian's column sum and the LDS tile body of the short blurs (ksize <= GF_MAXK), shared by the plain blur
// (k_basic.hip) and the blurs with an element-wise pass fused in front and behind (k_blurchain.hip); and the row and column bodies of the
// long blurs' strip kernel (k_gauss_strip, k_basic.hip), the same sequences with their LDS reads requested one step ahead.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include "common.hpp"
#include "kernels.hpp"

namespace vf {

// Column pass: cv::SymmColumnFilter's symmetric form, s = k[r]*S[y]; s = fma(k[r+j], S[y+j] + S[y-j], s) for j = 1..r (the order the
// parity tests' CPU restatement executes too: same operations in the same order, so the same bits).  Each thread produces
// GC_R consecutive rows of one column; lanes run along x so every row read is coalesced.  The two source rows a step needs for its GC_R
// outputs are the previous step's shifted by one row, so a step costs two new reads (register windows `up` / `dn`).
constexpr int GC_R = 8;

template <class Load>
__device__ inline void gauss_col_symm(Load ld, const float *__restrict__ kern, int r, float (&acc)[GC_R])
{
    // ld(i): source value i rows below the centre of output 0 (i in [-r, GC_R - 1 + r])
    float up[GC_R], dn[GC_R];
    const float kc = kern[r];
#pragma unroll
    for (int o = 0; o < GC_R; o++) { const float v = ld(o); acc[o] = __fmul_rn(kc, v); up[o] = v; dn[o] = v; }
    for (int j = 1; j <= r; j++) {
        const float nu = ld(GC_R - 1 + j), nd = ld(-j);
#pragma unroll
        for (int o = 0; o < GC_R - 1; o++) up[o] = up[o + 1];
        up[GC_R - 1] = nu;
#pragma unroll
        for (int o = GC_R - 1; o > 0; o--) dn[o] = dn[o - 1];
        dn[0] = nd;
        const float kj = kern[r + j];
#pragma unroll
        for (int o = 0; o < GC_R; o++) acc[o] = fmaf(kj, __fadd_rn(up[o], dn[o]), acc[o]);
    }
}

// gauss_col_symm with the two reads and the tap of step j + 1 requested before step j's arithmetic, for a kernel whose column pass runs at
// few waves per SIMD (k_gauss_strip): same operations in the same order per output.  kl(j): tap k[r + j]; ld and kl are called with j up to
// r + 1 clamped to r by this function, so they see only indices gauss_col_symm would give them.
template <class Load, class Tap>
__device__ inline void gauss_col_symm_ahead(Load ld, Tap kl, int r, float (&acc)[GC_R])
{
    float up[GC_R], dn[GC_R];
    const float kc = kl(0);
#pragma unroll
    for (int o = 0; o < GC_R; o++) { const float v = ld(o); acc[o] = __fmul_rn(kc, v); up[o] = v; dn[o] = v; }
    int jn = min(1, r);
    float nu = ld(GC_R - 1 + jn), nd = ld(-jn), kj = kl(jn);
    for (int j = 1; j <= r; j++) {
        jn = min(j + 1, r);
        const float nu1 = ld(GC_R - 1 + jn), nd1 = ld(-jn), kj1 = kl(jn);
#pragma unroll
        for (int o = 0; o < GC_R - 1; o++) up[o] = up[o + 1];
        up[GC_R - 1] = nu;
#pragma unroll
        for (int o = GC_R - 1; o > 0; o--) dn[o] = dn[o - 1];
        dn[0] = nd;
#pragma unroll
        for (int o = 0; o < GC_R; o++) acc[o] = fmaf(kj, __fadd_rn(up[o], dn[o]), acc[o]);
        nu = nu1; nd = nd1; kj = kj1;
    }
}

// gauss_row4 with the taps in LDS and the refill and the taps of step g + 1 requested before step g's arithmetic (k_gauss_strip): same
// operations in the same order per output.  ks4: taps k[1 ..] as float4 (k[4 g + 1 .. 4 g + 4] in element g), k0 = k[0]
__device__ inline float4 gauss_row4_ahead(const float4 *t4, const float4 *ks4, float k0, int ksize)
{
    const float4 c = t4[0];
    float v0 = c.x, v1 = c.y, v2 = c.z, v3 = c.w;
    float a0 = k0 * v0, a1 = k0 * v1, a2 = k0 * v2, a3 = k0 * v3;
    const int ng = (ksize - 1) >> 2, last = (ksize + 2) >> 2;      // full steps of four taps; the last refill the outputs use
    float4 n = t4[1], kk = ks4[0];
#define GR_TAP(K, N) { v0 = v1; v1 = v2; v2 = v3; v3 = (N); a0 = fmaf((K), v0, a0); a1 = fmaf((K), v1, a1); a2 = fmaf((K), v2, a2); a3 = fmaf((K), v3, a3); }
    for (int g = 0; g < ng; g++) {
        const float4 n1 = t4[min(g + 2, last)], kk1 = ks4[min(g + 1, last - 1)];
        GR_TAP(kk.x, n.x) GR_TAP(kk.y, n.y) GR_TAP(kk.z, n.z) GR_TAP(kk.w, n.w)
        n = n1; kk = kk1;
    }
    if ((ksize - 1) & 3) { GR_TAP(kk.x, n.x) GR_TAP(kk.y, n.y) }      // ksize is odd: two taps are left, or none
#undef GR_TAP
    return make_float4(a0, a1, a2, a3);
}

// Row pass: FOUR adjacent outputs per thread out of one sliding window of taps that is refilled four taps at a time by an aligned 16-byte LDS
// read (ds_read_b128); every output is still  s = k[0] S[0]; s = fma(k[j], S[j], s)  in ascending j.  t4: the window's start S[0..3], 16-byte
// aligned.  The last refill may reach up to three floats past the ksize + 3 the outputs use: the caller's row pitch holds them.
__device__ inline float4 gauss_row4(const float4 *t4, const float *__restrict__ kern, int ksize)
{
    const float4 c = t4[0];
    float v0 = c.x, v1 = c.y, v2 = c.z, v3 = c.w;
    const float k0 = kern[0];
    float a0 = k0 * v0, a1 = k0 * v1, a2 = k0 * v2, a3 = k0 * v3;
    for (int jb = 1; jb < ksize; jb += 4) {
        const float4 n = t4[(jb + 3) >> 2];      // S[jb + 3 .. jb + 6]
        const float nn[4] = {n.x, n.y, n.z, n.w};
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (jb + u < ksize) {
                v0 = v1; v1 = v2; v2 = v3; v3 = nn[u];
                const float kj = kern[jb + u];
                a0 = fmaf(kj, v0, a0); a1 = fmaf(kj, v1, a1); a2 = fmaf(kj, v2, a2); a3 = fmaf(kj, v3, a3);
            }
        }
    }
    return make_float4(a0, a1, a2, a3);
}

// Both passes in one kernel for short kernels (ksize <= GF_MAXK): a 64 x 32 output tile with its halo goes through LDS once -- row pass
// into a second LDS plane (rounded to float exactly as the intermediate plane of the two-kernel path is), column pass out of it -- so the
// intermediate plane never travels to memory.  Same taps, same order of the operations per output: same bits as the two kernels.
//
// The value that is blurred comes from a load functor and the blurred value goes to a store functor, so an element-wise pass in front of
// the blur and one behind it run inside the tile instead of as kernels of their own:
//   ld(b, y, x, v)          v[0..NV): the value(s) of frame b at pixel (y, x); (y, x) is inside the frame (reflect101 applied)
//   st(b, y, x, blur, ctr)  blur[0..NV): the blurred value(s) of output pixel (y, x); ctr[0..NV): what ld gave for that pixel
// RMAX is the largest radius an instance takes: it sizes the two LDS planes and the count of halo rows a wave loads, which the wave issues
// as one round of independent loads before it stores any of them.  The rows of the input tile are GF_PITCH apart, a multiple of 4, so
// that the row pass reads its sliding window of taps as aligned float4 (ds_read_b128: 16 lanes cover 64 consecutive banks) instead of
// single floats four banks apart.
constexpr int GF_TX = 64, GF_TY = 32;      // GF_MAXK: kernels.hpp
constexpr int GF_RSMALL = 2, GF_RLARGE = GF_MAXK / 2;      // the two classes: up to 5 taps, up to GF_MAXK taps
constexpr int gf_pitch(int rmax) { return (GF_TX + 2 * rmax + 3) & ~3; }

template <int RMAX, int NV>
struct GaussTile {
    float in_t[NV][(GF_TY + 2 * RMAX) * gf_pitch(RMAX)];
    float mid_t[NV][(GF_TY + 2 * RMAX) * GF_TX];
};

// A store step that reads planes of its own may split those reads off into a third functor, so that they do not wait behind the arithmetic of
// the row before:
//   pre(b, y, x)                 returns what output pixel (y, x) needs from memory, as a small struct; called for all GC_R rows first
//   st(b, y, x, blur, ctr, cx)   then takes that struct as its last argument
struct GaussNoPre {};

template <int RMAX, int NV, class Load, class Pre, class Store>
__device__ inline void gauss_tile(GaussTile<RMAX, NV> &t, Load ld, Pre pre, Store st, const float *__restrict__ kern, int ksize, int h, int w)
{
    static_assert(GF_TY == 4 * GC_R, "four waves of GC_R rows");
    constexpr int PITCH = gf_pitch(RMAX);
    constexpr int NIT = (GF_TY + 2 * RMAX + 3) / 4;      // halo rows per wave
    const int r = ksize / 2;
    const int tw = GF_TX + 2 * r, th = GF_TY + 2 * r;
    const int x0 = blockIdx.x * GF_TX, y0 = blockIdx.y * GF_TY;
    const size_t b = blockIdx.z;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // tile with halo: a wave per tile row, the lane's (at most two) source columns reflected once; all the wave's rows are requested
    // before the first one is stored (rows past the tile repeat its last row and are not stored)
    {
        const bool two = lane + 64 < tw;
        const int sx0 = reflect101(x0 + lane - r, w), sx1 = reflect101(x0 + (two ? lane + 64 : lane) - r, w);
        int sy[NIT];
#pragma unroll
        for (int i = 0; i < NIT; i++) sy[i] = reflect101(y0 + min(wv + 4 * i, th - 1) - r, h);
        // (no branch between the loads: lanes without a second column repeat their first one)
        float va[NIT][NV], vb[NIT][NV];
#pragma unroll
        for (int i = 0; i < NIT; i++) {
            ld(b, sy[i], sx0, va[i]);
            ld(b, sy[i], sx1, vb[i]);
        }
#pragma unroll
        for (int i = 0; i < NIT; i++) {
            const int ty = wv + 4 * i;
            if (ty < th) {
#pragma unroll
                for (int v = 0; v < NV; v++) {
                    t.in_t[v][ty * PITCH + lane] = va[i][v];
                    if (two) t.in_t[v][ty * PITCH + lane + 64] = vb[i][v];
                }
            }
        }
    }
    __syncthreads();
    // row pass: th rows x 64 columns, four adjacent outputs per thread (gauss_row4).  (The last refill may reach up to three floats past
    // the tile's tw columns: inside the row's pitch, never used.)
    for (int q = threadIdx.x; q < th * 16; q += 256) {
        const int ty = q >> 4, tx = (q & 15) * 4;
#pragma unroll
        for (int v = 0; v < NV; v++)
            *reinterpret_cast<float4 *>(t.mid_t[v] + ty * GF_TX + tx) =
                gauss_row4(reinterpret_cast<const float4 *>(t.in_t[v] + ty * PITCH + tx), kern, ksize);
    }
    __syncthreads();
    // column pass: symmetric sum over GC_R output rows of one column (gauss_col_symm)
    const int x = x0 + lane, yb = y0 + wv * GC_R;
    if (x >= w || yb >= h) return;
    float acc[NV][GC_R];
#pragma unroll
    for (int v = 0; v < NV; v++) {
        const float *tc = t.mid_t[v] + (wv * GC_R + r) * GF_TX + lane;
        gauss_col_symm([&](int i) { return tc[i * GF_TX]; }, kern, r, acc[v]);
    }
    if constexpr (std::is_same<Pre, GaussNoPre>::value) {
#pragma unroll
        for (int o = 0; o < GC_R; o++) {
            if (yb + o < h) {
                float bl[NV], ctr[NV];
#pragma unroll
                for (int v = 0; v < NV; v++) { bl[v] = acc[v][o]; ctr[v] = t.in_t[v][(wv * GC_R + o + r) * PITCH + lane + r]; }
                st(b, yb + o, x, bl, ctr);
            }
        }
    } else {
        // everything the GC_R output rows need from memory is requested before the first row is consumed (rows past the frame repeat its
        // last row: no branch between the loads)
        decltype(pre(b, 0, 0)) cx[GC_R];
#pragma unroll
        for (int o = 0; o < GC_R; o++) cx[o] = pre(b, min(yb + o, h - 1), x);
#pragma unroll
        for (int o = 0; o < GC_R; o++) {
            if (yb + o < h) {
                float bl[NV], ctr[NV];
#pragma unroll
                for (int v = 0; v < NV; v++) { bl[v] = acc[v][o]; ctr[v] = t.in_t[v][(wv * GC_R + o + r) * PITCH + lane + r]; }
                st(b, yb + o, x, bl, ctr, cx[o]);
            }
        }
    }
}

template <int RMAX, int NV, class Load, class Store>
__device__ inline void gauss_tile(GaussTile<RMAX, NV> &t, Load ld, Store st, const float *__restrict__ kern, int ksize, int h, int w)
{
    gauss_tile(t, ld, GaussNoPre(), st, kern, ksize, h, w);
}

// launch one of the two radius classes of a tile kernel template K<RMAX>
#define VF_LAUNCH_GAUSS_TILE(K, ksize, B, h, w, st, ...)                                                                         \
    do {                                                                                                                         \
        const dim3 grid_((w + GF_TX - 1) / GF_TX, (h + GF_TY - 1) / GF_TY, B);                                                   \
        if ((ksize) / 2 <= GF_RSMALL) hipLaunchKernelGGL(K<GF_RSMALL>, grid_, dim3(256), 0, st, __VA_ARGS__);                     \
        else hipLaunchKernelGGL(K<GF_RLARGE>, grid_, dim3(256), 0, st, __VA_ARGS__);                                            \
    } while (0)

}  // namespace vf
