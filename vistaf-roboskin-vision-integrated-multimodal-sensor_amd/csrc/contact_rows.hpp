// What the kernels with one workgroup per (frame, row) of the contacts table share: k_shape, k_thermal_contacts, k_motion, k_pressure_rows, and
// the read-outs with a workspace of the caller's, k_texture_*, k_match_*, k_outline_*, k_centreline_*, k_lobes_*.  The reading of a row's box, the
// walk over it, the prologues of an unused row and of a row without a pixel; for the last three also the capacity rule of their polylines, the
// LDS a row's tables may take and the -1 fill of an int8 plane.  Inline code, and one kernel template with its launcher.
#pragma once
#include "../../include/vistaf_ftp.h"
#include "common.hpp"

namespace vf {

// a box value of the table: finite and within +-1e9 (so that it, and it +- a margin, is an int), else no box
__device__ inline bool box_value(double v, int &o)
{
    if (!finitef(v) || v < -1.0e9 || v > 1.0e9) return false;
    o = (int)v;
    return true;
}

// The box of a table row: the table's own bx0..by1 (the values behind the first unreadable one stay 0, 0, -1, -1), whether all four were
// readable, and the part x0..x1, y0..y1 inside the h x w frame with its size bw x bh (0 where there is none).  An inverted box is empty here
// as well: clipping moves x0 up and x1 down only.
struct ContactBox {
    int bx0 = 0, by0 = 0, bx1 = -1, by1 = -1;
    bool ok;
    int x0, y0, x1, y1, bw, bh;
    __device__ inline ContactBox(const double *row, int h, int w)
    {
        ok = box_value(row[VISTAF_CONTACT_BBOX_X0], bx0) && box_value(row[VISTAF_CONTACT_BBOX_Y0], by0) &&
             box_value(row[VISTAF_CONTACT_BBOX_X1], bx1) && box_value(row[VISTAF_CONTACT_BBOX_Y1], by1);
        clip(h, w);
    }
    // a box derived from another (grown by a margin): the same clipping
    __device__ inline ContactBox(int ax0, int ay0, int ax1, int ay1, bool aok, int h, int w) : bx0(ax0), by0(ay0), bx1(ax1), by1(ay1), ok(aok) { clip(h, w); }
    __device__ inline int total() const { return bw * bh; }       // <= h * w < 2^31

private:
    __device__ inline void clip(int h, int w)
    {
        x0 = bx0 < 0 ? 0 : bx0; y0 = by0 < 0 ? 0 : by0; x1 = bx1 > w - 1 ? w - 1 : bx1; y1 = by1 > h - 1 ? h - 1 : by1;
        bw = ok && x1 >= x0 ? x1 - x0 + 1 : 0;
        bh = ok && y1 >= y0 ? y1 - y0 + 1 : 0;
    }
};

// The walk over a box: its pixels in row-major order, pixel i to thread i mod NT, f(x, y) for each.  Built once per box -- the thread's
// first pixel and the step of NT pixels, the only divisions -- so that every sweep over the box steps (x, y) without one.  Every float64
// sum of these kernels is formed in this order (pixel -> lane -> wave -> workgroup), which the headers promise.  f must hold no barrier:
// threads leave at different times.
template <int NT>
struct BoxWalk {
    int x0, y0, bw, total, tid, sx, sy, step_x, step_y;
    __device__ inline BoxWalk(const ContactBox &b, int t) : x0(b.x0), y0(b.y0), bw(b.bw), total(b.total()), tid(t)
    {
        step_y = bw ? NT / bw : 0;
        step_x = bw ? NT - step_y * bw : 0;
        sy = bw ? tid / bw : 0;
        sx = bw ? tid - sy * bw : 0;
    }
    template <typename F>
    __device__ inline void each(F f) const
    {
        int x = sx, y = sy;
        for (int i = tid; i < total; i += NT) {
            f(x0 + x, y0 + y);
            x += step_x;
            y += step_y;
            if (x >= bw) { x -= bw; y++; }
        }
    }
};

// count[b] as the number of rows in use
__device__ inline int clamp_count(int c, int K) { return c < 0 ? 0 : (c > K ? K : c); }

// The prologue of a row kernel: `unused` must be workgroup-uniform.  An unused row is written as n NaN (n <= the workgroup's threads) and
// the caller returns.
__device__ inline bool nan_row(bool unused, double *out, int n)
{
    if (unused && (int)threadIdx.x < n) out[threadIdx.x] = nan64();
    return unused;
}

// A row in use without a pixel (k_centreline_rows, k_lobes_rows): n fields (n <= the workgroup's threads), 0 before the status field, `status`
// in it, NaN behind it
__device__ inline void empty_row(double *out, int n, int status_field, int status)
{
    const int t = threadIdx.x;
    if (t < n) out[t] = t < status_field ? 0.0 : (t == status_field ? (double)status : nan64());
}

// The capacity rule of a frame's polylines (k_outline_poly over CORNERS, k_centreline_poly over STATIONS): row k of the kk rows in use is
// written when the counts of the rows up to it, table[(b * K + j) * stride + field], sum to at most `capacity`.  before: the elements of the
// written rows in front of k, where k's start; written: k's own count, or 0.  The totals only grow, so the rows up to k pass together and no
// row behind the first that does not fit is written.
struct RowCapacity { int before, written; };
__host__ __device__ inline RowCapacity row_capacity(const double *table, int stride, int field, int b, int K, int k, int kk, int capacity)
{
    long long cum = 0;
    int before = 0, mine = 0;
    for (int j = 0; j <= k && j < kk; j++) {
        const int c = (int)table[((size_t)b * K + j) * stride + field];
        cum += c;
        if (j < k && cum <= capacity) before = (int)cum;
        if (j == k) mine = c;
    }
    return {before, k < kk && cum <= capacity ? mine : 0};
}

// The LDS the tables of a row's box may take in a kernel that falls back to the caller's workspace for a larger box (k_centreline_rows,
// k_lobes_rows).  60 KB keeps the launch within the 64 KB every kernel may ask for without an attribute (the static reduction scratch and
// chunk arrays come on top) and lets two workgroups share a CU's 160 KB at the limit.
constexpr int ROW_LDS_BUDGET = 60 * 1024;

// v over an int8 plane of n elements (the skeleton plane, the lobe plane): 256 threads, 16 elements each, at most 65 536 workgroups
template <int V>
__global__ __launch_bounds__(256) void k_fill_i8(int8_t *__restrict__ plane, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) plane[i] = (int8_t)V;
}
inline dim3 fill_grid(size_t n)
{
    const size_t blocks = (n + 256 * 16 - 1) / (256 * 16);
    return dim3((unsigned)(blocks < 65536 ? blocks : 65536));
}
template <int V>
inline void launch_fill_i8(int8_t *plane, size_t n, hipStream_t st) { hipLaunchKernelGGL(k_fill_i8<V>, fill_grid(n), dim3(256), 0, st, plane, n); }

}  // namespace vf
