// Camera-native frame layouts onto the gray plane of the FTP path (float32 holding an integral 0..255 per pixel): the definitions of
// include/vistaf_ftp.h, VISTAF_FMT_RGB_U8 .. VISTAF_FMT_BAYER_BGGR_U8.  The reference has no counterpart: it reads frames cv2.imread has
// decoded.  Every kernel is a stream -- no LDS, no atomics; a thread takes the pixels one natural-width load brings:
//   rgb           one pixel, three byte loads (3-byte pixels at 1-byte alignment, as k_to_gray's BGR_U8)
//   bgra / rgba   one pixel, one dword
//   yuyv / uyvy   two pixels, one dword; the two Y bytes leave as one float2
//   nv12          one pixel, one byte of the Y plane; the chroma behind it is never read
//   bayer         one 2 x 2 quad: its 4 x 4 neighbourhood is sixteen byte loads (the cache serves the overlap between quads), and the four
//                 sites of a quad at even (y, x) are the four sites of the pattern, so every lane runs the same arithmetic
// Frames follow each other at frame_layout's stride, which is a multiple of the format's own alignment and of nothing more (NV12 at
// 150 x 202: 45450 = 2 mod 4), so no kernel assumes more than that alignment.
#include "host_util.hpp"

namespace vf {

namespace {

// cv2 RGB2Gray 8u, the fixed point of k_to_gray
__device__ inline float gray_of(int b, int g, int r) { return (float)((b * 3735 + g * 19235 + r * 9798 + (1 << 14)) >> 15); }

__global__ void __launch_bounds__(256) k_gray_rgb(const uint8_t *__restrict__ frames, float *__restrict__ gray, int P)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const size_t i = blockIdx.y * (size_t)P + p;
    const uint8_t *s = frames + 3 * i;
    gray[i] = gray_of(s[2], s[1], s[0]);
}

template <bool RGB>
__global__ void __launch_bounds__(256) k_gray_x4(const uint32_t *__restrict__ frames, float *__restrict__ gray, int P)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const size_t i = blockIdx.y * (size_t)P + p;
    const uint32_t v = frames[i];                               // little endian: byte 0 of the pixel in bits 0..7; byte 3 (alpha) is dropped
    const int c0 = v & 255, c1 = (v >> 8) & 255, c2 = (v >> 16) & 255;
    gray[i] = RGB ? gray_of(c2, c1, c0) : gray_of(c0, c1, c2);
}

// packed 4:2:2, w even: dword q of a frame holds pixels 2q and 2q + 1 (Y0 U Y1 V, or U Y0 V Y1)
template <bool UYVY>
__global__ void __launch_bounds__(256) k_gray_yuv422(const uint32_t *__restrict__ frames, float *__restrict__ gray, int halfP)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= halfP) return;
    const size_t i = blockIdx.y * (size_t)halfP + q;
    const uint32_t v = frames[i] >> (UYVY ? 8 : 0);
    ((float2 *)gray)[i] = make_float2((float)(v & 255), (float)((v >> 16) & 255));
}

// the Y plane of a 4:2:0 frame: P bytes at the head of every `stride` bytes
__global__ void __launch_bounds__(256) k_gray_yplane(const uint8_t *__restrict__ frames, float *__restrict__ gray, int P, size_t stride)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    gray[blockIdx.y * (size_t)P + p] = (float)frames[blockIdx.y * stride + p];
}

// reflect-101 of an index in -1 .. n + 1 (n >= 2); n + 1 is only asked for beside a ragged last row or column, where it is not used
__device__ inline int refl(int i, int n) { return i < 0 ? -i : (i >= n ? max(2 * (n - 1) - i, 0) : i); }

// One quad of a mosaic whose red site of the 2 x 2 block is (RY, RX), blue the opposite corner.  v[j][i] = mosaic(y0 - 1 + j, x0 - 1 + i).
template <int RY, int RX>
__device__ inline float bayer_site(const int (&v)[4][4], int dy, int dx)
{
    const int j = dy + 1, i = dx + 1, C = v[j][i];
    const bool red_row = dy == RY, red_col = dx == RX;
    int r, g, b;
    if (red_row == red_col) {                                    // a red or a blue site
        const int cross = (v[j - 1][i] + v[j + 1][i] + v[j][i - 1] + v[j][i + 1] + 2) >> 2;
        const int diag = (v[j - 1][i - 1] + v[j - 1][i + 1] + v[j + 1][i - 1] + v[j + 1][i + 1] + 2) >> 2;
        g = cross;
        r = red_row ? C : diag;
        b = red_row ? diag : C;
    } else {                                                     // a green site: the row's colour left and right, the other above and below
        const int hor = (v[j][i - 1] + v[j][i + 1] + 1) >> 1, ver = (v[j - 1][i] + v[j + 1][i] + 1) >> 1;
        g = C;
        r = red_row ? hor : ver;
        b = red_row ? ver : hor;
    }
    return gray_of(b, g, r);
}

// vec2: w even and the plane 8-byte aligned, so the two pixels of a quad's row sit on an 8-byte boundary and leave as one float2
template <int RY, int RX>
__global__ void __launch_bounds__(256) k_gray_bayer(const uint8_t *__restrict__ frames, float *__restrict__ gray, int h, int w, int qw, int nquads, int vec2)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nquads) return;
    const int y0 = 2 * (q / qw), x0 = 2 * (q % qw);
    const size_t P = (size_t)h * w;
    const uint8_t *s = frames + blockIdx.y * P;
    int xs[4], v[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++) xs[i] = refl(x0 - 1 + i, w);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint8_t *row = s + (size_t)refl(y0 - 1 + j, h) * w;
#pragma unroll
        for (int i = 0; i < 4; i++) v[j][i] = row[xs[i]];
    }
    float *d = gray + blockIdx.y * P + (size_t)y0 * w + x0;
    const bool right = x0 + 1 < w, below = y0 + 1 < h;
    const float g00 = bayer_site<RY, RX>(v, 0, 0), g01 = bayer_site<RY, RX>(v, 0, 1), g10 = bayer_site<RY, RX>(v, 1, 0), g11 = bayer_site<RY, RX>(v, 1, 1);
    if (vec2) {
        *(float2 *)d = make_float2(g00, g01);
        if (below) *(float2 *)(d + w) = make_float2(g10, g11);
    } else {
        d[0] = g00;
        if (right) d[1] = g01;
        if (below) {
            d[w] = g10;
            if (right) d[w + 1] = g11;
        }
    }
}

template <int RY, int RX>
void launch_bayer(const uint8_t *frames, float *gray, int B, int h, int w, hipStream_t st)
{
    const int qw = (w + 1) / 2, nquads = qw * ((h + 1) / 2);
    hipLaunchKernelGGL((k_gray_bayer<RY, RX>), dim3((nquads + 255) / 256, B), dim3(256), 0, st, frames, gray, h, w, qw, nquads,
                       (int)(w % 2 == 0 && ((uintptr_t)gray & 7) == 0));
}

}  // namespace

void launch_camera_gray(const void *frames, int format, float *gray, int B, int h, int w, hipStream_t st)
{
    const FrameLayout fl = frame_layout(format, h, w);
    const bool yuv422 = format == VISTAF_FMT_YUYV_U8 || format == VISTAF_FMT_UYVY_U8;       // w even, so P even: every frame's plane starts where gray does, mod 8
    assert(!fl.refusal && ((uintptr_t)frames & (uintptr_t)(fl.align - 1)) == 0 && ((uintptr_t)gray & (yuv422 ? 7 : 3)) == 0);
    const int P = h * w;
    const dim3 grid((P + 255) / 256, B), half((P / 2 + 255) / 256, B), block(256);
    const uint8_t *u8 = (const uint8_t *)frames;
    const uint32_t *u32 = (const uint32_t *)frames;
    switch (format) {
    case VISTAF_FMT_RGB_U8: hipLaunchKernelGGL(k_gray_rgb, grid, block, 0, st, u8, gray, P); break;
    case VISTAF_FMT_BGRA_U8: hipLaunchKernelGGL(k_gray_x4<false>, grid, block, 0, st, u32, gray, P); break;
    case VISTAF_FMT_RGBA_U8: hipLaunchKernelGGL(k_gray_x4<true>, grid, block, 0, st, u32, gray, P); break;
    case VISTAF_FMT_YUYV_U8: hipLaunchKernelGGL(k_gray_yuv422<false>, half, block, 0, st, u32, gray, P / 2); break;
    case VISTAF_FMT_UYVY_U8: hipLaunchKernelGGL(k_gray_yuv422<true>, half, block, 0, st, u32, gray, P / 2); break;
    case VISTAF_FMT_NV12_U8: hipLaunchKernelGGL(k_gray_yplane, grid, block, 0, st, u8, gray, P, fl.bytes); break;
    case VISTAF_FMT_BAYER_RGGB_U8: launch_bayer<0, 0>(u8, gray, B, h, w, st); break;
    case VISTAF_FMT_BAYER_GRBG_U8: launch_bayer<0, 1>(u8, gray, B, h, w, st); break;
    case VISTAF_FMT_BAYER_GBRG_U8: launch_bayer<1, 0>(u8, gray, B, h, w, st); break;
    case VISTAF_FMT_BAYER_BGGR_U8: launch_bayer<1, 1>(u8, gray, B, h, w, st); break;
    default: assert(false);
    }
}

}  // namespace vf
