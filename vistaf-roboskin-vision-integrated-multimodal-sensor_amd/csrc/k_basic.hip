// Per-pixel / stencil kernels of the FTP preprocessing (bandwidth-bound; planes are [B, h, w]).
//   to_gray        cv2.cvtColor(BGR2GRAY) fixed point          (shape_ftp.py:1511-1512)
//   sobel_mag      cv2.Sobel x/y ksize 3 + magnitude            (shape_ftp.py:633-635)
//   bad_flags      (img >= hi) | (grad >= g) & valid            (shape_ftp.py:638-639)
//   morph          cv2.dilate / erode with ELLIPSE element      (shape_ftp.py:644-646, :758-760, :1734-1736)
//   gauss_rows/cols cv2.GaussianBlur((0,0), sigma) REFLECT_101  (shape_ftp.py:746, :831, :836, :1145-1146)
//   illum_norm     I/(blur+1e-6) - 1                            (shape_ftp.py:832)
#include "kernels.hpp"
#include "gauss_tile.hpp"
#include "pixel_ops.hpp"
#include "mask_bits.hpp"

namespace vf {

// ------------------------------------------------------------------------------------------------
__global__ void k_to_gray(const void *__restrict__ frames, int format, float *__restrict__ gray, int P)
{
    int p = blockIdx.x * blockDim.x + threadIdx.x;
    size_t b = blockIdx.y;
    if (p >= P) return;
    size_t i = b * (size_t)P + p;
    float v;
    if (format == 0) v = (float)((const uint8_t *)frames)[i];
    else if (format == 2) v = rintf(__half2float(((const __half *)frames)[i]));
    else {
        int bb, gg, rr;
        if (format == 1) { const uint8_t *s = (const uint8_t *)frames + 3 * i; bb = s[0]; gg = s[1]; rr = s[2]; }
        else { const __half *s = (const __half *)frames + 3 * i; bb = (int)rintf(__half2float(s[0])); gg = (int)rintf(__half2float(s[1])); rr = (int)rintf(__half2float(s[2])); }
        // OpenCV 4.x RGB2Gray 8u: descale(b*BY15 + g*GY15 + r*RY15, 15), BY15=3735 GY15=19235 RY15=9798
        v = (float)((bb * 3735 + gg * 19235 + rr * 9798 + (1 << 14)) >> 15);
    }
    gray[i] = v;
}

void launch_to_gray(const void *frames, int format, float *gray, int B, int P, hipStream_t st, int w)
{
    if (format > 3) { launch_camera_gray(frames, format, gray, B, P / w, w, st); return; }      // the camera formats: k_formats.hip
    dim3 grid((P + 255) / 256, B);
    hipLaunchKernelGGL(k_to_gray, grid, dim3(256), 0, st, frames, format, gray, P);
}

// ------------------------------------------------------------------------------------------------
__global__ void k_sobel_mag(const float *__restrict__ img, float *__restrict__ grad, int h, int w)
{
    int x = blockIdx.x * blockDim.x + threadIdx.x;
    int y = blockIdx.y;
    size_t b = blockIdx.z;
    if (x >= w) return;
    const float *s = img + b * (size_t)h * w;
    int ym = reflect101(y - 1, h), yp = reflect101(y + 1, h), xm = reflect101(x - 1, w), xp = reflect101(x + 1, w);
    float a00 = s[(size_t)ym * w + xm], a01 = s[(size_t)ym * w + x], a02 = s[(size_t)ym * w + xp];
    float a10 = s[(size_t)y * w + xm], a12 = s[(size_t)y * w + xp];
    float a20 = s[(size_t)yp * w + xm], a21 = s[(size_t)yp * w + x], a22 = s[(size_t)yp * w + xp];
    float gx = __fadd_rn(__fadd_rn(__fsub_rn(a02, a00), __fmul_rn(2.0f, __fsub_rn(a12, a10))), __fsub_rn(a22, a20));
    float gy = __fadd_rn(__fadd_rn(__fsub_rn(a20, a00), __fmul_rn(2.0f, __fsub_rn(a21, a01))), __fsub_rn(a22, a02));
    grad[b * (size_t)h * w + (size_t)y * w + x] = sqrtf(__fadd_rn(__fmul_rn(gx, gx), __fmul_rn(gy, gy)));
}

void launch_sobel_mag(const float *img, float *grad, int B, int h, int w, hipStream_t st)
{
    dim3 grid((w + 255) / 256, h, B);
    hipLaunchKernelGGL(k_sobel_mag, grid, dim3(256), 0, st, img, grad, h, w);
}

// ------------------------------------------------------------------------------------------------
__global__ void k_bad_flags(const float *__restrict__ img, const float *__restrict__ grad, const uint8_t *__restrict__ valid,
                            const float *__restrict__ thr_hi, const float *__restrict__ thr_g, uint8_t *__restrict__ bad, int P)
{
    int p = blockIdx.x * blockDim.x + threadIdx.x;
    size_t b = blockIdx.y;
    if (p >= P) return;
    size_t i = b * (size_t)P + p;
    bad[i] = (uint8_t)bad_flag_px(valid[p], img[i], grad[i], thr_hi[b], thr_g[b]);
}

void launch_bad_flags(const float *img, const float *grad, const uint8_t *valid, const float *thr_hi, const float *thr_g,
                      uint8_t *bad, int B, int P, hipStream_t st)
{
    dim3 grid((P + 255) / 256, B);
    hipLaunchKernelGGL(k_bad_flags, grid, dim3(256), 0, st, img, grad, valid, thr_hi, thr_g, bad, P);
}

// ------------------------------------------------------------------------------------------------
// Binary dilate / erode, element given as row spans; out-of-image pixels never contribute
// (cv::morphologyDefaultBorderValue).  Optional AND with a static [P] and/or a per-frame [B,P] mask.
__global__ void k_morph(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, int h, int w, RowSpanSE se, int dilate,
                        const uint8_t *__restrict__ and_static, const uint8_t *__restrict__ and_frame)
{
    int x = blockIdx.x * blockDim.x + threadIdx.x;
    int y = blockIdx.y;
    size_t b = blockIdx.z;
    if (x >= w) return;
    const uint8_t *s = src + b * (size_t)h * w;
    int r = se.k / 2;
    // no early exit and clamped addresses: every load is independent of the others, so they are issued back to back
    // instead of one memory round trip per element pixel
    int any = 0, all = 1;
    for (int i = 0; i < se.k; i++) {
        const int yy = y + i - r;
        const bool rowin = yy >= 0 && yy < h;
        const uint8_t *row = s + (size_t)(yy < 0 ? 0 : (yy >= h ? h - 1 : yy)) * w;
        const int lo = se.lo[i], hi = se.hi[i];
#pragma unroll 4
        for (int dx = lo; dx <= hi; dx++) {
            const int xx = x + dx;
            const bool in = rowin && xx >= 0 && xx < w;
            const uint8_t px = row[xx < 0 ? 0 : (xx >= w ? w - 1 : xx)];
            any |= (in && px) ? 1 : 0;
            all &= (!in || px) ? 1 : 0;
        }
    }
    int v = dilate ? any : all;
    size_t p = (size_t)y * w + x;
    if (and_static && !and_static[p]) v = 0;
    if (and_frame && !and_frame[b * (size_t)h * w + p]) v = 0;
    dst[b * (size_t)h * w + p] = (uint8_t)v;
}

// Row-prefix variant for wide elements: inc[y][x] = number of set pixels in row y up to and including x, so
// "any / all set in [x0, x1]" is two loads per element row instead of a scan of the span.
__global__ __launch_bounds__(256) void k_row_prefix(const uint8_t *__restrict__ src, uint16_t *__restrict__ inc, int rows, int w)
{
    int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const uint8_t *s = src + (size_t)row * w;
    uint16_t *o = inc + (size_t)row * w;
    const unsigned long long le_mask = (lane == 63) ? ~0ull : ((2ull << lane) - 1ull);
    unsigned int run = 0;
    for (int x0 = 0; x0 < w; x0 += 64) {
        int x = x0 + lane;
        bool on = x < w && s[x] != 0;
        unsigned long long bm = __ballot(on);
        if (x < w) o[x] = (uint16_t)(run + (unsigned int)__popcll(bm & le_mask));
        run += (unsigned int)__popcll(bm);
    }
}

__global__ void k_morph_prefix(const uint16_t *__restrict__ inc, uint8_t *__restrict__ dst, int h, int w, RowSpanSE se, int dilate,
                               const uint8_t *__restrict__ and_static, const uint8_t *__restrict__ and_frame)
{
    int x = blockIdx.x * blockDim.x + threadIdx.x;
    int y = blockIdx.y;
    size_t b = blockIdx.z;
    if (x >= w) return;
    const uint16_t *I = inc + b * (size_t)h * w;
    int r = se.k / 2;
    // no early exit: the 2 * k loads are independent, so they are all in flight together (one memory round trip
    // per pixel instead of up to 2 * k dependent ones)
    int any = 0, all = 1;
#pragma unroll 8
    for (int i = 0; i < se.k; i++) {
        int yy = y + i - r;
        int x0 = x + se.lo[i], x1 = x + se.hi[i];
        if (x0 < 0) x0 = 0;
        if (x1 > w - 1) x1 = w - 1;
        const bool valid = yy >= 0 && yy < h && x1 >= x0;
        const int yc = yy < 0 ? 0 : (yy >= h ? h - 1 : yy);
        const int x1c = x1 < 0 ? 0 : x1, x0c = x0 > 0 ? x0 - 1 : 0;
        const uint16_t *row = I + (size_t)yc * w;
        const int hi = (int)row[x1c], lo = (int)row[x0c];
        const int cnt = hi - (x0 > 0 ? lo : 0);
        any |= (valid && cnt > 0) ? 1 : 0;
        all &= (!valid || cnt == x1 - x0 + 1) ? 1 : 0;
    }
    int v = dilate ? any : all;
    size_t p = (size_t)y * w + x;
    if (and_static && !and_static[p]) v = 0;
    if (and_frame && !and_frame[b * (size_t)h * w + p]) v = 0;
    dst[b * (size_t)h * w + p] = (uint8_t)v;
}

// Bit-plane variant for symmetric row spans [-a_i, a_i] (every cv ELLIPSE / RECT element): one workgroup per frame
// packs the mask into 64-bit words with ballots (coalesced byte loads), dilates in LDS with word shifts -- a
// 15x15 element costs a few hundred 64-bit ops per output word -- and unpacks.  Erosion is the dual: complement inside
// the image, dilate, complement (out-of-image pixels never erode: cv::morphologyDefaultBorderValue).
// The steps themselves (mb_pack, mb_morph_step, mb_unpack) and morph_bits_ok are in mask_bits.hpp, shared with the fused mask chains.
__global__ __launch_bounds__(MB_T) void k_morph_bits(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, int h, int w, MorphSeq seq,
                                                     const uint8_t *__restrict__ and_static, const uint8_t *__restrict__ and_frame)
{
    extern __shared__ unsigned long long mb_lds[];
    const int W64 = (w + 63) >> 6, nw = h * W64;
    unsigned long long *A = mb_lds, *O = mb_lds + nw;
    const size_t b = blockIdx.x;
    const uint8_t *s = src + b * (size_t)h * w;
    mb_pack(A, h, w, [s, w](int y, int x) { return s[(size_t)y * w + x]; });
    __syncthreads();
    const unsigned long long last_valid = mb_last_valid(w);
    for (int op = 0; op < seq.n; op++) mb_morph_step(A, O, h, W64, seq.se[op], seq.dilate[op] != 0, last_valid);
    // unpack (A holds the result)
    mb_unpack(A, dst + b * (size_t)h * w, h, w, and_static, and_frame ? and_frame + b * (size_t)h * w : nullptr);
}

void launch_morph(const uint8_t *src, uint8_t *dst, int B, int h, int w, const RowSpanSE &se, bool dilate,
                  const uint8_t *and_static, const uint8_t *and_frame, hipStream_t st, uint16_t *prefix_scratch, int force)
{
    const int tier = force ? force : morph_tier(se, h, w, prefix_scratch != nullptr);
    if (tier == MORPH_BITS) {
        MorphSeq seq;
        seq.n = 1; seq.dilate[0] = dilate ? 1 : 0; seq.se[0] = se;
        size_t lds = (size_t)h * ((w + 63) >> 6) * 16;
        hipLaunchKernelGGL(k_morph_bits, dim3(B), dim3(MB_T), lds, st, src, dst, h, w, seq, and_static, and_frame);
        return;
    }
    dim3 grid((w + 255) / 256, h, B);
    if (tier == MORPH_PREFIX) {
        int rows = B * h;
        hipLaunchKernelGGL(k_row_prefix, dim3((rows + 3) / 4), dim3(256), 0, st, src, prefix_scratch, rows, w);
        hipLaunchKernelGGL(k_morph_prefix, grid, dim3(256), 0, st, prefix_scratch, dst, h, w, se, dilate ? 1 : 0, and_static, and_frame);
        return;
    }
    hipLaunchKernelGGL(k_morph, grid, dim3(256), 0, st, src, dst, h, w, se, dilate ? 1 : 0, and_static, and_frame);
}

// n operations with the same element back to back (dilates[i] != 0: dilate, else erode); the AND masks apply to the final result.
// One kernel (pack once, unpack once) when the bit-plane path applies; `tmp` is a scratch plane for the fallback chain.
void launch_morph_seq(const uint8_t *src, uint8_t *dst, uint8_t *tmp, int B, int h, int w, const RowSpanSE &se, const int *dilates, int n,
                      const uint8_t *and_static, const uint8_t *and_frame, hipStream_t st, uint16_t *prefix_scratch)
{
    if (n >= 1 && n <= MB_MAXOPS && morph_bits_ok(se, h, w)) {
        MorphSeq seq;
        seq.n = n;
        for (int i = 0; i < n; i++) { seq.dilate[i] = dilates[i] ? 1 : 0; seq.se[i] = se; }
        size_t lds = (size_t)h * ((w + 63) >> 6) * 16;
        hipLaunchKernelGGL(k_morph_bits, dim3(B), dim3(MB_T), lds, st, src, dst, h, w, seq, and_static, and_frame);
        return;
    }
    const uint8_t *cur = src;
    for (int i = 0; i < n; i++) {
        // alternate so that the last operation writes dst
        uint8_t *out = ((n - 1 - i) & 1) ? tmp : dst;
        const bool last = i == n - 1;
        launch_morph(cur, out, B, h, w, se, dilates[i] != 0, last ? and_static : nullptr, last ? and_frame : nullptr, st, prefix_scratch);
        cur = out;
    }
}

// ------------------------------------------------------------------------------------------------
// Separable Gaussian, BORDER_REFLECT_101.  Row pass: 64-column x 16-row tile staged in LDS with halo.
constexpr int GB_TX = 64, GB_TY = 16, GB_MAXK = 512;

__global__ __launch_bounds__(256) void k_gauss_rows(const float *__restrict__ src, float *__restrict__ dst,
                                                    const float *__restrict__ kern, int ksize, int h, int w)
{
    // 64 columns x GB_TY rows per workgroup; a thread produces the same column of GB_TY / 4 rows, so a tap fetched once (a scalar
    // load: wave-uniform address in read-only memory) feeds that many outputs and the row loads of the tile are all in flight together
    extern __shared__ float lds[];
    constexpr int NR = GB_TY / 4;
    const int r = ksize / 2;
    const int tw = GB_TX + 2 * r;
    float *tile = lds;                  // GB_TY rows of tw
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int x0 = blockIdx.x * GB_TX, y0 = blockIdx.y * GB_TY;
    const size_t b = blockIdx.z;
    const float *plane = src + b * (size_t)h * w;
    for (int rr = ty; rr < GB_TY; rr += 4) {
        const int y = y0 + rr;
        if (y >= h) break;
        const float *row = plane + (size_t)y * w;
        for (int i = tx; i < tw; i += 64) tile[rr * tw + i] = row[reflect101(x0 + i - r, w)];
    }
    __syncthreads();
    const int x = x0 + tx;
    if (x >= w) return;
    float acc[NR];
    const float *t = tile + ty * tw + tx;
    {
        const float k0 = kern[0];
#pragma unroll
        for (int q = 0; q < NR; q++) acc[q] = k0 * t[q * 4 * tw];
    }
    for (int j = 1; j < ksize; j++) {
        const float kj = kern[j];
#pragma unroll
        for (int q = 0; q < NR; q++) acc[q] = fmaf(kj, t[q * 4 * tw + j], acc[q]);
    }
#pragma unroll
    for (int q = 0; q < NR; q++) {
        const int y = y0 + ty + 4 * q;
        if (y < h) dst[b * (size_t)h * w + (size_t)y * w + x] = acc[q];
    }
}

// Column pass: gauss_col_symm (gauss_tile.hpp), GC_R consecutive rows of one column per thread.
// global-memory form (kernels too long for the LDS tile)
__global__ __launch_bounds__(256) void k_gauss_cols(const float *__restrict__ src, float *__restrict__ dst,
                                                    const float *__restrict__ kern, int ksize, int h, int w)
{
    const int r = ksize / 2;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y0 = (blockIdx.y * 4 + (threadIdx.x >> 6)) * GC_R;
    const size_t b = blockIdx.z;
    if (x >= w || y0 >= h) return;
    const float *s = src + b * (size_t)h * w;
    float acc[GC_R];
    gauss_col_symm([&](int i) { return s[(size_t)reflect101(y0 + i, h) * w + x]; }, kern, r, acc);
#pragma unroll
    for (int o = 0; o < GC_R; o++)
        if (y0 + o < h) dst[b * (size_t)h * w + (size_t)(y0 + o) * w + x] = acc[o];
}

// Column pass through LDS: the block's 64 columns x (32 + 2r) source rows are staged with ONE round of independent coalesced loads
// (the global form walks its taps with dependent loads), then every thread runs the symmetric sum over its 8 output rows.
__global__ __launch_bounds__(256) void k_gauss_cols_lds(const float *__restrict__ src, float *__restrict__ dst,
                                                        const float *__restrict__ kern, int ksize, int h, int w)
{
    extern __shared__ float lds[];
    float *tile = lds;                     // [(32 + 2r)][64]
    const int r = ksize / 2, rows = 32 + 2 * r;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int x = blockIdx.x * 64 + tx;
    const int yb = blockIdx.y * 32;
    const size_t b = blockIdx.z;
    const float *s = src + b * (size_t)h * w;
    const int xc = x < w ? x : w - 1;
    for (int j = ty; j < rows; j += 4) tile[j * 64 + tx] = s[(size_t)reflect101(yb + j - r, h) * w + xc];
    __syncthreads();
    const int y0 = yb + ty * GC_R;
    if (x >= w || y0 >= h) return;
    const float *tc = tile + (ty * GC_R + r) * 64 + tx;
    float acc[GC_R];
    gauss_col_symm([&](int i) { return tc[i * 64]; }, kern, r, acc);
#pragma unroll
    for (int o = 0; o < GC_R; o++)
        if (y0 + o < h) dst[b * (size_t)h * w + (size_t)(y0 + o) * w + x] = acc[o];
}

void launch_gauss_rows(const float *src, float *dst, const float *kern, int ksize, int B, int h, int w, hipStream_t st)
{
    dim3 grid((w + GB_TX - 1) / GB_TX, (h + GB_TY - 1) / GB_TY, B);
    size_t lds = (size_t)GB_TY * (GB_TX + 2 * (ksize / 2)) * sizeof(float);
    hipLaunchKernelGGL(k_gauss_rows, grid, dim3(256), lds, st, src, dst, kern, ksize, h, w);
}

void launch_gauss_cols(const float *src, float *dst, const float *kern, int ksize, int B, int h, int w, hipStream_t st)
{
    dim3 grid((w + 63) / 64, (h + 4 * GC_R - 1) / (4 * GC_R), B);
    const size_t lds = (size_t)(32 + 2 * (ksize / 2)) * 64 * sizeof(float);
    if (lds <= 64 * 1024) { hipLaunchKernelGGL(k_gauss_cols_lds, grid, dim3(256), lds, st, src, dst, kern, ksize, h, w); return; }
    hipLaunchKernelGGL(k_gauss_cols, grid, dim3(256), 0, st, src, dst, kern, ksize, h, w);
}

// Both passes in one kernel for short kernels (ksize <= GF_MAXK): the tile body of gauss_tile.hpp with nothing in front and nothing behind.
template <int RMAX>
__global__ __launch_bounds__(256) void k_gauss_fused(const float *__restrict__ src, float *__restrict__ dst, const float *__restrict__ kern,
                                                     int ksize, int h, int w)
{
    __shared__ __align__(16) GaussTile<RMAX, 1> tile;
    const size_t P = (size_t)h * w;
    gauss_tile(tile,
               [&](size_t b, int y, int x, float (&v)[1]) { v[0] = src[b * P + (size_t)y * w + x]; },
               [&](size_t b, int y, int x, const float (&blur)[1], const float (&)[1]) { dst[b * P + (size_t)y * w + x] = blur[0]; },
               kern, ksize, h, w);
}

// Both passes in one kernel for long kernels on frames whose height fits LDS (gauss_strip_fits, kernels.hpp): a workgroup owns GS_TX output
// columns of one frame over the full height.  Row pass: the strip's input, GS_TX + 2r columns wide, goes through an LDS tile in chunks of GS_CH
// rows; the next chunk's loads are in flight (in registers) while the current one is filtered by gauss_row4_ahead into the LDS plane
// mid[h][GS_TX], rounded to float exactly as the intermediate plane of the two-kernel path is.  Column pass: gauss_col_symm's sequence
// (gauss_col_symm_ahead) out of that plane, rows beyond the frame as reflect101 indices into it, so a strip needs no row halo and any radius
// works.  Same taps, same order per output: same bits as k_gauss_rows + k_gauss_cols.  src != dst: neighbouring strips read each other's
// columns.  The taps are copied to LDS first: at three waves per SIMD the kernel lives on having the next step's LDS reads in flight, and
// scalar loads of the taps inside the loops would share a counter with them and drain it every step.
//
// A wave loads, stores and filters the same eight rows of a chunk, 2 wv + {0, 1} + {0, 8, 16, 24}: with a pitch that is an odd multiple of
// four floats, rows 8 apart lie 32 banks apart, and the lanes that one ds_read_b128 lane group serves (quartets 0 / 3 / 5 / 6 and
// 1 / 2 / 4 / 7 of each half wave) are given rows that tile the 64 banks.
// The strips of a frame share most of their input columns, and consecutive workgroups go to different XCDs, each with an L2 of its own:
// the block index is remapped so that a frame's strips run on one XCD (nblk = B * nstrip blocks, bijective for any nblk).
__global__ __launch_bounds__(256) void k_gauss_strip(const float *__restrict__ src, float *__restrict__ dst, const float *__restrict__ kern,
                                                     int ksize, int h, int w, int nstrip, int nblk)
{
    extern __shared__ float4 gs_lds[];
    static_assert(GS_CH == 32 && GS_TX == 32, "four waves of eight rows, eight quads per row");
    constexpr int NL = GS_CH / 4;      // rows a wave owns per chunk
    int b, x0;
    {
        const int i = blockIdx.x, q = nblk >> 3, rem = nblk & 7, g = i & 7;
        const int id = (g < rem ? g * (q + 1) : rem * (q + 1) + (g - rem) * q) + (i >> 3);
        b = id / nstrip;
        x0 = (id - b * nstrip) * GS_TX;
    }
    const int r = ksize / 2, tw = GS_TX + 2 * r, pitch = gs_pitch(ksize);
    float *mid = reinterpret_cast<float *>(gs_lds);      // [h][GS_TX]
    float *tile = mid + (size_t)h * GS_TX;               // [GS_CH][pitch]
    float *ktap = tile + GS_CH * pitch, *kshift = ktap + GS_KPAD;      // the taps k[i], and k[i + 1] (the row pass reads them as aligned float4)
    if (threadIdx.x < GS_KPAD) {
        const int i = threadIdx.x;
        ktap[i] = i < ksize ? kern[i] : 0.0f;
        kshift[i] = i + 1 < ksize ? kern[i + 1] : 0.0f;
    }
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const float *plane = src + (size_t)b * h * w;
    // the lane's (at most two) source columns, reflected once; lanes without a second column repeat their first one (no branch between the loads)
    const bool one = lane < tw, two = lane + 64 < tw;
    const int sx0 = reflect101(x0 + (one ? lane : 0) - r, w), sx1 = reflect101(x0 + (two ? lane + 64 : 0) - r, w);
    // the row this lane filters: quartet pairs (octets) 0..3 of a half wave take rows +0, +16, +8, +24
    const int oct = lane >> 3;
    const int frow = 2 * wv + (oct >> 2) + 8 * (((oct & 1) << 1) | ((oct >> 1) & 1)), tx = (lane & 7) * 4;
    const int nch = (h + GS_CH - 1) / GS_CH;
    float va[NL], vb[NL];
    // all loads of a chunk are issued before the first store (rows past the frame repeat its last row and are not filtered into mid)
#define GS_REQUEST(c)                                                                             \
    _Pragma("unroll") for (int i = 0; i < NL; i++) {                                              \
        const float *row = plane + (size_t)min((c) * GS_CH + 2 * wv + (i & 1) + 8 * (i >> 1), h - 1) * w; \
        va[i] = row[sx0];                                                                         \
        vb[i] = row[sx1];                                                                         \
    }
    GS_REQUEST(0)
    for (int c = 0; c < nch; c++) {
#pragma unroll
        for (int i = 0; i < NL; i++) {
            float *trow = tile + (2 * wv + (i & 1) + 8 * (i >> 1)) * pitch;
            if (one) trow[lane] = va[i];
            if (two) trow[lane + 64] = vb[i];
        }
        __syncthreads();
        if (c + 1 < nch) { GS_REQUEST(c + 1) }
        const int y = c * GS_CH + frow;
        const float4 o = gauss_row4_ahead(reinterpret_cast<const float4 *>(tile + frow * pitch + tx), reinterpret_cast<const float4 *>(kshift), ktap[0], ksize);
        if (y < h) *reinterpret_cast<float4 *>(mid + y * GS_TX + tx) = o;
        __syncthreads();      // the tile is free for the next chunk; after the last chunk: mid is complete
    }
#undef GS_REQUEST
    // column pass: GC_R consecutive rows of one column per thread, 64 rows of the strip per round
    const int col = threadIdx.x & 31, x = x0 + col;
    const float *tc = mid + col;
    float *out = dst + (size_t)b * h * w;
    for (int yb = (threadIdx.x >> 5) * GC_R; yb < h; yb += 8 * GC_R) {
        float acc[GC_R];
        const auto kl = [&](int j) { return ktap[r + j]; };
        if (yb >= r && yb + GC_R - 1 + r < h) gauss_col_symm_ahead([&](int i) { return tc[(yb + i) * GS_TX]; }, kl, r, acc);
        else gauss_col_symm_ahead([&](int i) { return tc[reflect101(yb + i, h) * GS_TX]; }, kl, r, acc);
        if (x < w) {
#pragma unroll
            for (int o = 0; o < GC_R; o++)
                if (yb + o < h) out[(size_t)(yb + o) * w + x] = acc[o];
        }
    }
}

int launch_gauss_blur(const float *src, float *tmp, float *dst, const float *kern, int ksize, int B, int h, int w, hipStream_t st, bool strip, int force)
{
    if (!force && ksize <= GF_MAXK && src != dst) {
        VF_LAUNCH_GAUSS_TILE(k_gauss_fused, ksize, B, h, w, st, src, dst, kern, ksize, h, w);
        return GAUSS_TILE;
    }
    if (force ? force == GAUSS_STRIP : (strip && src != dst && gauss_strip_fits(h, w, ksize))) {
        const int nstrip = (w + GS_TX - 1) / GS_TX, nblk = B * nstrip;
        hipLaunchKernelGGL(k_gauss_strip, dim3(nblk), dim3(256), gauss_strip_lds(h, ksize), st, src, dst, kern, ksize, h, w, nstrip, nblk);
        return GAUSS_STRIP;
    }
    launch_gauss_rows(src, tmp, kern, ksize, B, h, w, st);
    launch_gauss_cols(tmp, dst, kern, ksize, B, h, w, st);
    return GAUSS_TWO;
}

// ------------------------------------------------------------------------------------------------
__global__ void k_illum_norm(const float *__restrict__ img, const float *__restrict__ blur, float *__restrict__ out, size_t n)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = illum_norm_px(img[i], blur[i]);
}
void launch_illum_norm(const float *img, const float *blur, float *out, int B, int P, hipStream_t st)
{
    size_t n = (size_t)B * P;
    hipLaunchKernelGGL(k_illum_norm, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, img, blur, out, n);
}

__global__ void k_mul_static(const float *__restrict__ a, const float *__restrict__ stat, float *__restrict__ out, int P)
{
    int p = blockIdx.x * blockDim.x + threadIdx.x;
    size_t b = blockIdx.y;
    if (p >= P) return;
    out[b * (size_t)P + p] = mul_static_px(a[b * (size_t)P + p], stat[p]);
}
void launch_mul_static(const float *a, const float *stat, float *out, int B, int P, hipStream_t st)
{
    dim3 grid((P + 255) / 256, B);
    hipLaunchKernelGGL(k_mul_static, grid, dim3(256), 0, st, a, stat, out, P);
}

__global__ void k_count_u8(const uint8_t *__restrict__ m, int *__restrict__ counts, int P)
{
    __shared__ int scratch[16];
    size_t b = blockIdx.y;
    int c = 0;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < P; p += gridDim.x * blockDim.x) c += m[b * (size_t)P + p] != 0;
    c = block_sum<int>(c, scratch);
    if (threadIdx.x == 0 && c) atomicAdd(&counts[b], c);
}
void launch_count_u8(const uint8_t *m, int *counts, int B, int P, hipStream_t st)
{
    hipMemsetAsync(counts, 0, sizeof(int) * B, st);
    int gx = (P + 256 * 16 - 1) / (256 * 16);
    if (gx < 1) gx = 1;
    hipLaunchKernelGGL(k_count_u8, dim3(gx, B), dim3(256), 0, st, m, counts, P);
}

}  // namespace vf
