// What the kernels with one workgroup per (frame, row) of the contacts table share: k_shape, k_thermal_contacts, k_motion, k_pressure_rows, k_texture_*.
// The reading of a row's box, the walk over it and the prologue of an unused row.  Device inline code only.
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

}  // namespace vf
