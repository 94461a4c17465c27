// What the five k_unwrap*.hip files share, one definition each: the uint16 rank range and the tiers, the padded index space, the wrap
// rule, the 3 x 3 neighbour slots and the bitmap push of the two LDS floods, the consistency check's planes, and the launchers one of the
// files calls in another.  Private to the family: api.hip and the test hooks see kernels.hpp only.
#pragma once
#include <cstdlib>
#include "host_util.hpp"

namespace vf {

// ---- tiers.  A frame's padded plane holds EN = (h + 2)(w + 2) pixels.  Rank codes start at 3 (0 outside the mask, 1 visited, 2 frontier),
// so a uint16 code plane takes frames of at most 65536 - 3 ranks.
constexpr long UW_RANK16_MAX_EN = 65533;
__host__ __device__ constexpr long padded_pixels(int h, int w) { return (long)(h + 2) * (w + 2); }
inline bool unwrap_ranked_supported(int h, int w) { return padded_pixels(h, w) <= UW_RANK16_MAX_EN; }
inline bool unwrap_big_supported(int h, int w) { return !unwrap_ranked_supported(h, w) && padded_pixels(h, w) < (1L << 26); }
inline int unwrap_tier_of(int h, int w, bool big_handback)      // unwrap_tier of kernels.hpp
{
    if (unwrap_ranked_supported(h, w)) return UWT_RANK16;
    return unwrap_big_supported(h, w) && !big_handback ? UWT_BITMAP : UWT_GENERIC;
}

// ---- padded index space: the frame with one pixel of border on every side, rows of W2 = w + 2
// per-frame stride of the rank-code plane (8 elements: the batched flood copies it into LDS 16 bytes at a time)
__host__ __device__ constexpr long code_stride(long EN) { return (EN + 7) & ~7L; }
__host__ __device__ inline int pad_index(int y, int x, int W2) { return (y + 1) * W2 + x + 1; }
// row = idx / W2 as a multiply-high by magic = floor(2^32 / W2) + 1 = (2^32 + e) / W2 with 0 < e <= W2: the product's high word is
// floor(idx / W2 + idx e / (2^32 W2)), which is idx / W2 rounded down while idx e < 2^32.  padded_magic yields 0 where that is not certain
// for every idx < EN (EN * W2 >= 2^32), and padded_row then divides.  Every frame of the uint16 rank range has a magic.
inline uint32_t padded_magic(int h, int w)
{
    const unsigned long long EN = (unsigned long long)padded_pixels(h, w), W2 = (unsigned long long)w + 2;
    return EN * W2 < 0x100000000ull ? (uint32_t)(0x100000000ull / W2) + 1u : 0u;
}
__host__ __device__ inline int padded_row(int idx, uint32_t magic, int W2)
{
    return magic ? (int)(((unsigned long long)(uint32_t)idx * magic) >> 32) : idx / W2;
}
// the frame index y * w + x of padded index idx (an interior one)
__host__ __device__ inline int unpad_index(int idx, uint32_t magic, int W2)
{
    const int py = padded_row(idx, magic, W2);
    return (py - 1) * (W2 - 2) + (idx - py * W2 - 1);
}
// rule (i) of the two LDS floods: padded pixels a and b lie within Chebyshev distance 2 of each other
__host__ __device__ inline bool within_two(int a, int b, uint32_t magic, int W2)
{
    const int ya = padded_row(a, magic, W2), yb = padded_row(b, magic, W2);
    return abs(ya - yb) <= 2 && abs((a - ya * W2) - (b - yb * W2)) <= 2;
}

// ---- the 3 x 3 block without its centre, slots 0..7 in lexicographic (dy, dx) order: the lowest visited slot is the reference's parent
__host__ __device__ inline void neighbour_slot(int n, int &dy, int &dx)
{
    const int l = n < 4 ? n : n + 1;
    dy = l / 3 - 1;
    dx = l % 3 - 1;
}
__host__ __device__ inline int neighbour_offset(int n, int stride)
{
    int dy, dx;
    neighbour_slot(n, dy, dx);
    return dy * stride + dx;
}

// ---- the wrap rule.  wrap_count(d): the integer k that brings d = w[b] - w[a] into (-pi, pi]; unwrap_value: the plane's final expression
constexpr double UW_TWOPI = 6.283185307179586476925286766559, UW_PI = 3.14159265358979323846;
__host__ __device__ inline int wrap_count(double d)
{
    double k = -rint(d / UW_TWOPI);
    const double dd = d + UW_TWOPI * k;
    if (dd <= -UW_PI) k += 1.0;
    else if (dd > UW_PI) k -= 1.0;
    return (int)k;
}
__host__ __device__ inline float unwrap_value(float w, int k) { return (float)((double)w + UW_TWOPI * (double)k); }

// ---- bitmap over ranks (or rank codes) in LDS, one summary bit per word on each level above L0: set r's bit on LEVELS levels
template <int LEVELS>
__device__ inline void bitmap_push(uint32_t r, unsigned long long *L0, unsigned long long *L1, unsigned long long *L2 = nullptr)
{
    static_assert(LEVELS == 2 || LEVELS == 3, "two or three levels");
    atomicOr(&L0[r >> 6], 1ull << (r & 63u));
    atomicOr(&L1[r >> 12], 1ull << ((r >> 6) & 63u));
    if (LEVELS == 3) atomicOr(&L2[r >> 18], 1ull << ((r >> 12) & 63u));
}

// ---- the consistency check (k_unwrap_fast.hip): its per-frame planes, dead again before the flood kernels of a failed frame start
struct UfPlanes {
    int8_t *kk;                 // [P16] k of the pixel (relative to its run, later absolute); -128 = not in the mask, -127 = never reached
    int32_t *rowbase;           // [hp] first run of each row; rowbase[h] = number of runs
    uint32_t *rstate;           // [rcap] UF_KNOWN | (offset & 0xFFFF)
    uint16_t *ei, *ej;          // [ecap] run above, run below
    int16_t *ed;                // [ecap] offset[below] - offset[above]
    unsigned long long *seedkey;// [B]
    int32_t *ctl;               // [B][UFC_N]
    size_t P16, hp;
    int rcap, ecap;
};
UfPlanes unwrap_fast_planes(ScratchLayout &L, int B, int h, int w);
void launch_unwrap_fast(const float *wrapped, const float *quality, const uint8_t *mask, float *unwrapped, int32_t *need, const UfPlanes &U, int B, int h, int w,
                        hipStream_t st);

// ---- the launchers behind launch_unwrap, each in the file of its kernel
// k_unwrap_rank.hip
void launch_unwrap_ranked(const float *quality, const uint8_t *mask, uint32_t *g0, uint32_t *g2, int32_t *ppar, size_t gstride, uint16_t *rank16,
                          int32_t *seed, int B, int h, int w, hipStream_t st, hipEvent_t ev_flood, const int32_t *need);
void launch_unwrap_rank32(const float *quality, const uint8_t *mask, uint32_t *gA, uint32_t *gB, size_t gstride, uint32_t *rank32, int32_t *seed,
                          int32_t *n_out, int B, int h, int w, hipStream_t st, const int32_t *need);
// k_unwrap_batch.hip
void launch_unwrap_flood_batch(const uint16_t *rank16, const int32_t *seed, const uint32_t *inv, size_t inv_stride, int32_t *ppar, size_t gstride,
                               uint32_t *order, size_t ostride, int B, int h, int w, hipStream_t st, const int32_t *need);
void launch_unwrap_replay(const float *wrapped, const uint32_t *order, size_t ostride, const int32_t *ppar, size_t gstride, int32_t *tree,
                          float *unwrapped, int B, int h, int w, hipStream_t st, const int32_t *need);
// k_unwrap_big.hip
void launch_unwrap_flood_big(uint32_t *code, const int32_t *seed, const int32_t *n, const uint32_t *inv, size_t inv_stride, int32_t *ppar,
                             size_t gstride, int32_t *need_generic, bool force_generic, int B, int h, int w, hipStream_t st, const int32_t *need);

}  // namespace vf
