// Bit planes of a binary mask: one 64-bit word per 64 columns of a row (bit x & 63 of word y * W64 + (x >> 6)), held in LDS by the one
// 1024-thread workgroup that owns the frame.  One definition of each step -- ballot pack, word-shift dilate / erode, unpack, count -- for
// k_morph_bits (k_basic.hip) and the fused mask chains (k_maskchain.hip), and the pure host rules that decide which frames take them
// (tests/diag/maskchain_host_check.hip holds those against brute force).
#pragma once
#include "kernels.hpp"
#include "mask_rules.hpp"

namespace vf {

constexpr int MB_T = 1024;      // 16 waves: packing / unpacking a row is a global-memory round trip, so rows in flight are what counts
constexpr int MB_RB = 2;        // rows per wave and iteration (MB_RB * 4 independent byte loads in flight per lane)
constexpr int MB_MAXOPS = 4;
struct MorphSeq {               // up to MB_MAXOPS operations applied back to back on the packed plane (close = dilate, erode; n-fold dilate)
    int n;
    int dilate[MB_MAXOPS];
    RowSpanSE se[MB_MAXOPS];
};

// ---- pure rules -----------------------------------------------------------------------------------
__host__ __device__ inline int mb_w64(int w) { return (w + 63) >> 6; }
__host__ __device__ inline size_t mb_plane_bytes(int h, int w) { return (size_t)h * mb_w64(w) * 8; }
// columns of a row's last word that exist
__host__ __device__ inline unsigned long long mb_last_valid(int w) { return (w & 63) ? ((1ull << (w & 63)) - 1ull) : ~0ull; }

// the elements the word-shift step takes (symmetric row spans [-a_i, a_i], every cv ELLIPSE / RECT element and every chamfer ball), on
// frames whose two planes fit the default 64 KB of dynamic LDS
inline bool morph_bits_ok(const RowSpanSE &se, int h, int w)
{
    for (int i = 0; i < se.k; i++) {
        if (se.lo[i] > se.hi[i]) { if (se.hi[i] >= 0) return false; continue; }      // empty rows must read hi < 0
        if (se.lo[i] != -se.hi[i] || se.hi[i] > 63) return false;
    }
    return (size_t)h * ((w + 63) >> 6) * 16 <= 64 * 1024;
}
// The kernel launch_morph runs (MorphTier of kernels.hpp): the bit planes where they apply, the row prefix sums for elements of 7 rows and
// more when the caller has scratch for them (uint16 counts: rows shorter than 65536), the span scan otherwise
inline int morph_tier(const RowSpanSE &se, int h, int w, bool have_prefix)
{
    if (morph_bits_ok(se, h, w)) return MORPH_BITS;
    return (have_prefix && se.k >= 7 && w < 65536) ? MORPH_PREFIX : MORPH_GENERIC;
}

// A bit plane read as a mask indexed by pixel, m[p] like the byte plane it stands for (cc_row_contacts, cc_lds_forest).  y = p / w is a
// multiply-high by inv = floor(2^32 / w) + 1: exact for 0 <= p <= 65535 and 2 <= w <= 65535 (inv * w - 2^32 <= w, so the excess
// p * (inv * w - 2^32) / (w * 2^32) stays below 1 / w), which covers every frame the uint16 forest takes; w = 1, whose inv would not fit
// 32 bits, is y = p.
struct BitMask {
    const unsigned long long *A;
    int w, W64;
    uint32_t inv;
    __host__ __device__ BitMask(const unsigned long long *A_, int w_) : A(A_), w(w_), W64(mb_w64(w_)), inv(w_ > 1 ? (uint32_t)(0x100000000ull / (uint32_t)w_) + 1u : 0u) {}
    __host__ __device__ int row_of(int p) const { return w == 1 ? p : (int)(((unsigned long long)(uint32_t)p * inv) >> 32); }
    __host__ __device__ int word_of(int p, int &bit) const { const int y = row_of(p), x = p - y * w; bit = x & 63; return y * W64 + (x >> 6); }
    __host__ __device__ bool operator[](int p) const { int bit; const int i = word_of(p, bit); return (A[i] >> bit) & 1ull; }
};

// Which chains of a session run as one launch (Tiers::fused_masks bits; k_maskchain.hip)
enum MaskChain { MCH_BAD = 1, MCH_RELIABLE = 2, MCH_CONTACT = 4 };
constexpr int MCH_REL_PLANES = 3, MCH_CONTACT_PLANES = 3, MCH_BAD_PLANES = 2;
// dynamic LDS of a chain's kernel: its bit planes, and for the reliable chain the label forest behind them
__host__ __device__ inline size_t mask_chain_lds(int chain, int h, int w)
{
    const size_t pl = mb_plane_bytes(h, w);
    if (chain == MCH_RELIABLE) return MCH_REL_PLANES * pl + cc_lds_forest_bytes(h * w);
    return (chain == MCH_CONTACT ? MCH_CONTACT_PLANES : MCH_BAD_PLANES) * pl;
}
// Whether `chain` takes h x w frames with `nops` operations by `se` (bad: the dilations; reliable: the 2 * iters steps of the closing;
// contact: the dilations) and, for the reliable chain, an erosion by the chamfer ball of `margin` pixels (<= 0: none).  The frame's planes
// (and forest) within LDS_DYN_HEADROOM, uint16 labels, at most MB_MAXOPS operations, every element one the word-shift step takes.
inline bool mask_chain_fits(int chain, int h, int w, const RowSpanSE &se, int nops, float margin = 0.f)
{
    if (chain != MCH_BAD && chain != MCH_RELIABLE && chain != MCH_CONTACT) return false;
    if (h < 1 || w < 1 || nops < 0 || nops > MB_MAXOPS) return false;
    if ((size_t)h * w > 65535 && chain == MCH_RELIABLE) return false;
    if ((size_t)h * mb_w64(w) > 0x7fffffffull / 64) return false;
    if (mask_chain_lds(chain, h, w) > (size_t)LDS_DYN_HEADROOM) return false;
    if (nops > 0 && !morph_bits_ok(se, h, w)) return false;
    if (chain == MCH_RELIABLE && margin > 0.f) {
        RowSpanSE ball;
        if (!chamfer_ball(margin, &ball) || !morph_bits_ok(ball, h, w)) return false;
    }
    return true;
}

#ifdef __HIPCC__
// ---- device steps (all MB_T threads of the frame's workgroup call them) ------------------------------
// Packs px(y, x) != 0 over the image into A.  px is called for pixels inside the image only; the loads of MB_RB rows are independent and
// issued together.  No barrier: the caller synchronises before the plane is read.
template <typename Px>
__device__ inline void mb_pack(unsigned long long *A, int h, int w, Px px)
{
    const int W64 = (w + 63) >> 6;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    for (int y0 = wid * MB_RB; y0 < h; y0 += (MB_T / 64) * MB_RB)
        for (int j0 = 0; j0 < W64; j0 += 4) {
            uint8_t v[MB_RB][4];
#pragma unroll
            for (int rr = 0; rr < MB_RB; rr++)
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int y = y0 + rr, x = (j0 + u) * 64 + lane;
                    v[rr][u] = (y < h && j0 + u < W64 && x < w) ? px(y, x) : (uint8_t)0;
                }
#pragma unroll
            for (int rr = 0; rr < MB_RB; rr++)
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const unsigned long long word = __ballot(v[rr][u] != 0);
                    if (lane == 0 && y0 + rr < h && j0 + u < W64) A[(y0 + rr) * W64 + j0 + u] = word;
                }
        }
}

// One dilation (dil) or erosion of the plane A by se into O, then the two swap: A holds the result on return, and it is visible (the last
// statement is a barrier).  Erosion is the dual: complement inside the image, dilate, complement (out-of-image pixels never erode:
// cv::morphologyDefaultBorderValue).  A must be visible to the workgroup on entry.
__device__ inline void mb_morph_step(unsigned long long *&A, unsigned long long *&O, int h, int W64, const RowSpanSE &se, bool dil,
                                     unsigned long long last_valid)
{
    const int tid = threadIdx.x, nw = h * W64;
    if (!dil) {                                             // erosion = complement inside the image, dilate, complement
        for (int t = tid; t < nw; t += MB_T) { const int j = t % W64; A[t] = ~A[t] & (j == W64 - 1 ? last_valid : ~0ull); }
        __syncthreads();
    }
    const int r = se.k / 2;
    for (int t = tid; t < nw; t += MB_T) {
        const int y = t / W64, j = t - y * W64;
        unsigned long long acc = 0ull;
        for (int i = 0; i < se.k; i++) {
            const int yy = y + i - r, a = se.hi[i];
            if (yy < 0 || yy >= h || a < 0) continue;
            const unsigned long long *row = A + yy * W64;
            const unsigned long long wc = row[j], wl = j > 0 ? row[j - 1] : 0ull, wr = j < W64 - 1 ? row[j + 1] : 0ull;
            unsigned long long m = wc;
            for (int dd = 1; dd <= a; dd++) m |= (wc >> dd) | (wr << (64 - dd)) | (wc << dd) | (wl >> (64 - dd));
            acc |= m;
        }
        const unsigned long long valid = j == W64 - 1 ? last_valid : ~0ull;
        O[t] = dil ? (acc & valid) : (~acc & valid);
    }
    __syncthreads();
    unsigned long long *tmp = A; A = O; O = tmp;
}

// Unpacks A to the frame's byte plane o, ANDed with the optional byte masks ms (static) and mf (the frame's own); the masks of a row are
// loaded together
__device__ inline void mb_unpack(const unsigned long long *A, uint8_t *__restrict__ o, int h, int w, const uint8_t *__restrict__ ms,
                                 const uint8_t *__restrict__ mf)
{
    const int W64 = (w + 63) >> 6;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    for (int y0 = wid * MB_RB; y0 < h; y0 += (MB_T / 64) * MB_RB)
        for (int j0 = 0; j0 < W64; j0 += 4) {
            uint8_t vs[MB_RB][4], vf[MB_RB][4];
#pragma unroll
            for (int rr = 0; rr < MB_RB; rr++)
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int y = y0 + rr, x = (j0 + u) * 64 + lane;
                    const size_t p = (y < h && j0 + u < W64 && x < w) ? (size_t)y * w + x : 0;
                    vs[rr][u] = ms ? ms[p] : (uint8_t)1;
                    vf[rr][u] = mf ? mf[p] : (uint8_t)1;
                }
#pragma unroll
            for (int rr = 0; rr < MB_RB; rr++)
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int y = y0 + rr, x = (j0 + u) * 64 + lane;
                    if (y >= h || j0 + u >= W64 || x >= w) continue;
                    const int v = (int)((A[y * W64 + j0 + u] >> lane) & 1ull);
                    o[(size_t)y * w + x] = (uint8_t)(v && vs[rr][u] && vf[rr][u]);
                }
        }
}

// number of set bits of the plane (bits beyond the image are zero in every plane the steps above produce); valid in all threads
__device__ inline int mb_count(const unsigned long long *A, int nw, int *scratch16)
{
    int c = 0;
    for (int t = threadIdx.x; t < nw; t += MB_T) c += (int)__popcll(A[t]);
    return block_sum<int>(c, scratch16);
}
#endif

}  // namespace vf
