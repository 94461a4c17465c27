// The rules of the mask-topology family (threshold, 8-connected labelling, largest component, chamfer distance tiers, blob peak, fused back
// end), one definition each.  Private to the family: k_cc_dist.hip, backend_device.hpp (cc_lds_build), k_backend.hip, the blob kernels of
// k_post.hip, stages.hip for chamfer_ball.  The pure rules come first and are __host__ __device__ (or host only), so that
// tests/diag/mask_host_check.hip holds them against brute force; the wave-level rules follow.
#pragma once
#include <algorithm>
#include <cmath>
#include "kernels.hpp"

namespace vf {

// ---- dynamic LDS ---------------------------------------------------------------------------------
// A workgroup may ask for 160 KB of dynamic LDS.  The tiers that size their planes by the frame keep to 150 KB: the difference is the room
// for the static LDS of whichever kernel takes the plane and for the alignment of the regions carved behind it.
constexpr int LDS_DYN_MAX = 160 * 1024;
constexpr int LDS_DYN_HEADROOM = 150 * 1024;
// dynamic LDS of cc_lds_build: the forest, and behind it the mask plane when that is staged too (MLDS)
__host__ __device__ inline size_t cc_lds_forest_bytes(int P) { return (size_t)((P + 2 + 7) & ~7) * 2; }
__host__ __device__ inline size_t cc_lds_bytes(int P) { return cc_lds_forest_bytes(P) + (size_t)P + 16; }

// ---- contacts between runs of adjacent rows -------------------------------------------------------
// Every mask pixel already belongs to the tree of its horizontal run, so what is left to unite for pixel p = (x, y) of mask plane m are
// the runs of row y - 1 that touch it: a pixel whose left neighbour is set leaves the run above-left / above to that neighbour, and the
// pixel above-right starts a new contact only where the pixel above is clear -- a couple of unions per run instead of three per pixel.
// left: x > 0 && m[p - 1], from the caller (k_cc_merge has it for its own union, and a second read of it behind that union's atomics
// cost the kernel two registers and 4 % of its time).  unite(a, b) joins the components of pixels a and b.  m is the byte plane, or anything
// indexed like it (BitMask of mask_bits.hpp: the bit plane in LDS).
template <typename Mask, typename Unite>
__host__ __device__ inline void cc_row_contacts(Mask m, int p, int x, int y, int w, bool left, Unite unite)
{
    if (y == 0) return;
    const bool ul = x > 0 && m[p - w - 1], up = m[p - w] != 0, ur = x < w - 1 && m[p - w + 1];
    if ((ul || up) && !left) unite(p, ul ? p - w - 1 : p - w);
    if (ur && !up) unite(p, p - w + 1);
}

// ---- the largest root ----------------------------------------------------------------------------
// Key of root pixel p with `area` pixels: the larger area wins, among equal areas the smaller root index = first in raster order =
// smallest OpenCV label.  Key 0 is "no component"; ccl_root of it is -2, which no label equals (-1 marks a pixel outside the mask).
__host__ __device__ inline unsigned long long ccl_key(int area, int p) { return ((unsigned long long)(unsigned int)area << 32) | (unsigned int)(0x7fffffff - p); }
__host__ __device__ inline int ccl_root(unsigned long long key) { return (key >> 32) ? (0x7fffffff - (int)(key & 0xffffffffu)) : -2; }

// ---- the 3x3 chamfer metric (cv::distanceTransform DIST_L2, 3x3 mask) in 1/65536 units --------------
constexpr int CH_HV = 62587;    // cvRound(0.955  * 65536)
constexpr int CH_DG = 89738;    // cvRound(1.3693 * 65536)
constexpr int CH_DIST_MAX = 0x7fffffff >> 2;     // cv DIST_MAX: "no zero pixel", border / initial value of the two-pass planes
__host__ __device__ inline int chamfer_metric(int dx, int dy)
{
    const int mn = dx < dy ? dx : dy, mx = dx < dy ? dy : dx;
    return CH_HV * (mx - mn) + CH_DG * mn;
}
__host__ __device__ inline float chamfer_to_float(int c) { return (float)c * (1.0f / 65536.0f); }

// rows either side of a pixel that the closed form looks at: every zero pixel within cap_px + 2 of it lies that close
__host__ __device__ inline int chamfer_cap_rows(int h, int cap_px)
{
    const int cap = (int)((cap_px + 2) / 0.955) + 2;
    return cap > h ? h : cap;
}
// k_chamfer_lds keeps a uint16 row distance per pixel in LDS
__host__ __device__ inline bool chamfer_lds_fits(int h, int w) { return (size_t)h * w * 2 <= (size_t)LDS_DYN_HEADROOM; }

// d(x, y) = min over rows y' of metric(g(y', x), |y - y'|), g = horizontal distance to the nearest zero pixel of row y': the two-pass 3x3
// chamfer result in closed form (the metric grows with |dx| for a fixed |dy|), exact up to `cap` rows either side.  rowdist(yy, g) sets
// g for this column and returns whether row yy has a zero pixel at all (a test on the plane's own "none" value, so that the callers keep
// the branch they had: with "none" folded into a negative distance k_chamfer_cols came out 4 % slower).  Rows further away than the best
// distance so far cannot improve it.
template <typename RowDist>
__host__ __device__ inline int chamfer_col_min(RowDist rowdist, int y, int h, int cap)
{
    int best = CH_DIST_MAX;
    for (int dy = 0; dy <= cap; dy++) {
        if ((long long)dy * CH_HV >= best) break;
#pragma unroll
        for (int s = 0; s < 2; s++) {
            if (s && !dy) break;
            const int yy = s ? y + dy : y - dy;
            if (yy < 0 || yy >= h) continue;
            int gx;
            if (!rowdist(yy, gx)) continue;
            const int c = chamfer_metric(gx, dy);
            if (c < best) best = c;
        }
    }
    return best;
}

// Row spans of the set { (dx, dy) : metric <= margin } (dist = c / 65536 as float, exact, so "dist <= margin" is "c <= margin * 65536").
// false: too large for a structuring element.
inline bool chamfer_ball(float margin, RowSpanSE *se)
{
    const long long M = (long long)std::floor((double)margin * 65536.0);
    if (M < 0) return false;
    const int R = (int)(M / CH_HV);
    if (2 * R + 1 > 33 || R > 63) return false;
    se->k = std::max(3, 2 * R + 1);
    const int r = se->k / 2;
    for (int i = 0; i < se->k; i++) {
        const int dy = std::abs(i - r);
        int a = -1;
        for (int dx = 0; dx <= 63; dx++) {
            if (chamfer_metric(dx, dy) <= M) a = dx; else break;
        }
        if (a < 0) { se->lo[i] = 1; se->hi[i] = -1; }       // empty row
        else { se->lo[i] = (int8_t)-a; se->hi[i] = (int8_t)a; }
    }
    return true;
}

// ---- wave-level rules ----------------------------------------------------------------------------
// Position of the last zero pixel at or before column x of a row that a wave walks 64 columns at a time, left to right: a prefix maximum
// over the chunk and the carry of the chunks before it (the value lane 63 left; the caller's "none yet" to start with, which is also what
// a row without a zero so far returns).
constexpr int ROW_NO_ZERO = (int)0x80000000;
__device__ inline int row_last_zero(bool zero, int x, int &carry)
{
    int lz = wave_scan_max_i32(zero ? x : ROW_NO_ZERO, ROW_NO_ZERO);
    lz = lz > carry ? lz : carry;
    carry = __builtin_amdgcn_readlane(lz, 63);
    return lz;
}

// Run-length area count of a wave: consecutive 64-pixel tiles mostly belong to the same (large) component, and an atomic per tile on one
// address serialises the whole frame in L2.  ccl_run_count takes the roots of one tile (negative: no pixel), extends the current run or
// flushes it with one atomicAdd and starts the next; ccl_run_flush after the last tile.
__device__ inline void ccl_run_flush(int run_root, int run_cnt, int32_t *A, int lane)
{
    if (run_root >= 0 && lane == 0) atomicAdd(&A[run_root], run_cnt);
}
__device__ inline void ccl_run_count(int root, int &run_root, int &run_cnt, int32_t *A, int lane)
{
    unsigned long long active = __ballot(root >= 0);
    while (active) {
        const int leader = __ffsll((long long)active) - 1;
        const int r0 = __builtin_amdgcn_readlane(root, leader);
        const unsigned long long same = __ballot(root == r0);
        if (r0 == run_root) run_cnt += (int)__popcll(same);
        else {
            ccl_run_flush(run_root, run_cnt, A, lane);
            run_root = r0; run_cnt = (int)__popcll(same);
        }
        active &= ~same;
    }
}

// Per-root peak of a wave's 64 pixels: one atomicMax per root among them, of the largest v (float bits of a value >= 0) of its lanes
__device__ inline void wave_root_max(int root, unsigned int v, unsigned int *peak, int lane)
{
    unsigned long long active = __ballot(root >= 0);
    while (active) {
        const int leader = __ffsll((long long)active) - 1;
        const int r0 = __shfl(root, leader, 64);
        const bool same = root == r0;
        const unsigned int mx = wave_max_u32(same ? v : 0u);
        if (lane == leader) atomicMax(&peak[r0], mx);
        active &= ~__ballot(same);
    }
}

}  // namespace vf
