// Per-contact shape read-out (include/vistaf_shape.h): footprint ellipse, boundary count and the quadric cap of every contact, from the depth
// plane of a predict and the index plane, table and counts vistaf_ftp_contacts wrote.  An extension, as the table and the tracker: the
// reference has no counterpart.  The definition is in the header; tests/shapes_helpers.py restates it in NumPy.
//
//   k_shape  ONE launch per call, one workgroup per (frame, row).  A contact is compact and its box is in the table, so the workgroup walks
//            the box, not the frame: the box's pixels in row-major order, pixel i to thread i mod SH_NT (consecutive lanes read consecutive
//            bytes of the int8 plane and consecutive floats of the depth plane until a box row ends; a box wider than the workgroup is
//            simply several strides).  Every thread keeps its partial sums in registers -- three counts, five exact integer moment sums,
//            the 14 monomial sums beside the pixel count and the 6 right-hand sides of the normal equations in float64 -- and the workgroup adds them up with the DPP
//            tree inside a wave and in wave order across waves.  Thread 0 runs chol_solve<6> and the two 2 x 2 eigen-decompositions and
//            leaves the coefficients in LDS; the workgroup walks the box a second time (it sits in L2) for the residual sum and thread 0
//            writes the row.  The boundary test reads the four neighbours from the planes, frame-edge neighbours counting as outside.
// No memset, no atomics, no workspace: every float64 sum is formed in an order fixed by the box and the launch geometry (pixel -> lane ->
// wave -> workgroup), so two calls give the same bits and a frame's rows do not depend on the batch it is measured in.
#include <string>

#include "../../include/vistaf_shape.h"
#include "contact_rows.hpp"
#include "form_fit.hpp"
#include "host_util.hpp"

using namespace vf;

namespace {

constexpr int SH_NT = 512, SH_NW = SH_NT / 64;
constexpr int SH_NF = FIT_NF, SH_NI = 8;                // float64 sums (form_fit.hpp); integer sums (n, boundary, m, Sx, Sy, Sxx, Syy, Sxy)
constexpr double SH_HALF_PI = 1.5707963267948966;

// 0.5 * atan2(p, q) as a direction in (-pi/2, pi/2]; 0 when both are 0
__device__ inline double sh_half_angle(double p, double q)
{
    if (p == 0.0 && q == 0.0) return 0.0;
    const double t = 0.5 * atan2(p, q);
    return t <= -SH_HALF_PI ? SH_HALF_PI : t;
}

struct ShapeFrame {
    const float *depth;
    const int8_t *index;
    int h, w, k;
    float eps;
    __device__ inline bool contact(int x, int y, float &d) const       // is (x, y), inside the frame, a contact pixel of row k; d = its depth
    {
        const size_t p = (size_t)y * w + x;
        const int idx = index[p];
        d = depth[p];
        if (d != d) d = 0.0f;
        return idx == k && d > eps;
    }
    __device__ inline bool contact_inside(int x, int y) const      // false outside the frame
    {
        float d;
        return x >= 0 && x < w && y >= 0 && y < h && contact(x, y, d);
    }
};

__global__ __launch_bounds__(SH_NT) void k_shape(const float *__restrict__ depth, const int8_t *__restrict__ index, const double *__restrict__ contacts,
                                                 const int32_t *__restrict__ count, const double *__restrict__ mm_per_px, float eps, double fit_frac,
                                                 int h, int w, int K, double *__restrict__ shapes)
{
    __shared__ double wf[SH_NW][SH_NF + 1], tf[SH_NF + 1];
    __shared__ unsigned long long wi[SH_NW][SH_NI], ti[SH_NI];
    __shared__ double coef[6];
    __shared__ int fit_status;
    const int b = blockIdx.x / K, k = blockIdx.x - b * K;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    double *out = shapes + (size_t)blockIdx.x * VISTAF_NSHAPE;
    int kk = count[b];
    kk = kk < 0 ? 0 : (kk > K ? K : kk);
    if (k >= kk) {
        if (tid < VISTAF_NSHAPE) out[tid] = nan64();
        return;
    }
    const double *row = contacts + (size_t)blockIdx.x * VISTAF_NCONTACT;
    const size_t P = (size_t)h * w;
    const ShapeFrame fr{depth + b * P, index + b * P, h, w, k, eps};
    // the box: u, v from the table's own, the walk over its part inside the frame
    int bx0 = 0, by0 = 0, bx1 = -1, by1 = -1;
    const bool box_ok = box_value(row[VISTAF_CONTACT_BBOX_X0], bx0) && box_value(row[VISTAF_CONTACT_BBOX_Y0], by0) &&
                        box_value(row[VISTAF_CONTACT_BBOX_X1], bx1) && box_value(row[VISTAF_CONTACT_BBOX_Y1], by1);
    const FitCoords uv(bx0, by0, bx1, by1);
    const double xc = uv.xc, yc = uv.yc, hx = uv.hx, hy = uv.hy;
    const int x0 = bx0 < 0 ? 0 : bx0, y0 = by0 < 0 ? 0 : by0, x1 = bx1 > w - 1 ? w - 1 : bx1, y1 = by1 > h - 1 ? h - 1 : by1;
    const int bw = box_ok && x1 >= x0 ? x1 - x0 + 1 : 0, bh = box_ok && y1 >= y0 ? y1 - y0 + 1 : 0;
    const int total = bw * bh;                                      // <= h * w < 2^31
    const int step_y = bw ? SH_NT / bw : 0, step_x = bw ? SH_NT - step_y * bw : 0;
    const float fit_thr = (float)(fit_frac * row[VISTAF_CONTACT_MAX_DEPTH_MM]);
    const bool fit_all = fit_frac == 0.0;

    // ---- sweep 1: counts, integer moments, normal equations
    unsigned int n = 0, nb = 0, m = 0;
    unsigned long long sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
    double f[SH_NF];
#pragma unroll
    for (int j = 0; j < SH_NF; j++) f[j] = 0.0;
    {
        int x = bw ? tid % bw : 0, y = bw ? tid / bw : 0;
        for (int i = tid; i < total; i += SH_NT) {
            const int px = x0 + x, py = y0 + y;
            float d;
            if (fr.contact(px, py, d)) {
                n++;
                const bool inner = fr.contact_inside(px - 1, py) && fr.contact_inside(px + 1, py) && fr.contact_inside(px, py - 1) &&
                                   fr.contact_inside(px, py + 1);
                nb += inner ? 0u : 1u;
                const unsigned long long ux = (unsigned long long)px, uy = (unsigned long long)py;
                sx += ux; sy += uy; sxx += ux * ux; syy += uy * uy; sxy += ux * uy;
                if (fit_all || d >= fit_thr) {
                    m++;
                    fit_accumulate(f, uv.u(px), uv.v(py), (double)d);
                }
            }
            x += step_x;
            y += step_y;
            if (x >= bw) { x -= bw; y++; }
        }
    }
    // workgroup sums: DPP tree in a wave, waves in order
    const unsigned long long iv[SH_NI] = {n, nb, m, sx, sy, sxx, syy, sxy};
#pragma unroll
    for (int j = 0; j < SH_NI; j++) {
        const unsigned long long s = wave_sum(iv[j]);
        if (lane == 0) wi[wid][j] = s;
    }
#pragma unroll
    for (int j = 0; j < SH_NF; j++) {
        const double s = wave_sum(f[j]);
        if (lane == 0) wf[wid][j] = s;
    }
    __syncthreads();
    if (tid < SH_NI) {
        unsigned long long s = 0;
        for (int q = 0; q < SH_NW; q++) s += wi[q][tid];
        ti[tid] = s;
    } else if (tid >= 64 && tid < 64 + SH_NF) {
        double s = 0.0;
        for (int q = 0; q < SH_NW; q++) s += wf[q][tid - 64];
        tf[tid - 64] = s;
    }
    __syncthreads();

    // ---- thread 0: footprint, solve, curvatures
    const double s = mm_per_px[b];
    if (tid == 0) {
        const double dn = (double)ti[0], dm = (double)ti[2];
        for (int j = 0; j < VISTAF_NSHAPE; j++) out[j] = nan64();
        out[VISTAF_SHAPE_CONTACT_PIXELS] = dn;
        out[VISTAF_SHAPE_BOUNDARY_PIXELS] = (double)ti[1];
        out[VISTAF_SHAPE_FIT_PIXELS] = dm;
        if (ti[0]) {
            const double cx = (double)ti[3] / dn, cy = (double)ti[4] / dn;
            const double mu20 = (double)ti[5] / dn - cx * cx, mu02 = (double)ti[6] / dn - cy * cy, mu11 = (double)ti[7] / dn - cx * cy;
            const double hd = (mu20 - mu02) / 2.0, r = sqrt(hd * hd + mu11 * mu11), mean = (mu20 + mu02) / 2.0;
            const double l1 = fmax(mean + r, 0.0), l2 = fmax(mean - r, 0.0);
            out[VISTAF_SHAPE_FOOTPRINT_CX] = cx;
            out[VISTAF_SHAPE_FOOTPRINT_CY] = cy;
            out[VISTAF_SHAPE_MAJOR_AXIS_MM] = 4.0 * sqrt(l1) * s;
            out[VISTAF_SHAPE_MINOR_AXIS_MM] = 4.0 * sqrt(l2) * s;
            out[VISTAF_SHAPE_ORIENTATION_RAD] = sh_half_angle(2.0 * mu11, mu20 - mu02);
        }
        int status = VISTAF_SHAPEFIT_NONE;
        if (ti[2] >= 6) {
            double c[6];
            if (fit_solve<6>(tf, dm, c)) {
                const double ax = hx * s, ay = hy * s;
                const double q3 = c[3] / (ax * ax), q4 = c[4] / (ax * ay), q5 = c[5] / (ay * ay);
                const double mean = q3 + q5, dev = sqrt((q3 - q5) * (q3 - q5) + q4 * q4);
                const bool low = mean <= 0.0;                      // curvature_1 = mean - dev
                const double k1 = low ? mean - dev : mean + dev, k2 = low ? mean + dev : mean - dev;
                status = mean + dev < 0.0 ? VISTAF_SHAPEFIT_OK : VISTAF_SHAPEFIT_NOT_A_CAP;
                out[VISTAF_SHAPE_CURVATURE_1_PER_MM] = k1;
                out[VISTAF_SHAPE_CURVATURE_2_PER_MM] = k2;
                out[VISTAF_SHAPE_CURVATURE_AXIS_RAD] = low ? sh_half_angle(-q4, q5 - q3) : sh_half_angle(q4, q3 - q5);
                if (status == VISTAF_SHAPEFIT_OK) {
                    const double det = 4.0 * c[3] * c[5] - c[4] * c[4];
                    const double ua = (c[4] * c[2] - 2.0 * c[5] * c[1]) / det, va = (c[4] * c[1] - 2.0 * c[3] * c[2]) / det;
                    out[VISTAF_SHAPE_APEX_X] = xc + ua * hx;
                    out[VISTAF_SHAPE_APEX_Y] = yc + va * hy;
                    out[VISTAF_SHAPE_APEX_DEPTH_MM] = fit_poly(c, ua, va);
                    out[VISTAF_SHAPE_RADIUS_1_MM] = -1.0 / k1;
                    out[VISTAF_SHAPE_RADIUS_2_MM] = -1.0 / k2;
                }
                for (int j = 0; j < 6; j++) coef[j] = c[j];
            }
        }
        out[VISTAF_SHAPE_FIT_STATUS] = (double)status;
        fit_status = status;
    }
    __syncthreads();
    if (fit_status == VISTAF_SHAPEFIT_NONE) return;

    // ---- sweep 2: residuals of the fit pixels with the solved coefficients
    double c[6], r2 = 0.0;
#pragma unroll
    for (int j = 0; j < 6; j++) c[j] = coef[j];
    {
        int x = tid % bw, y = tid / bw;                            // m >= 6: the box is not empty
        for (int i = tid; i < total; i += SH_NT) {
            const int px = x0 + x, py = y0 + y;
            float d;
            if (fr.contact(px, py, d) && (fit_all || d >= fit_thr)) {
                const double r = (double)d - fit_poly(c, uv.u(px), uv.v(py));
                r2 += r * r;
            }
            x += step_x;
            y += step_y;
            if (x >= bw) { x -= bw; y++; }
        }
    }
    r2 = wave_sum(r2);
    if (lane == 0) wf[wid][SH_NF] = r2;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int q = 0; q < SH_NW; q++) t += wf[q][SH_NF];
        out[VISTAF_SHAPE_FIT_RMS_MM] = sqrt(t / (double)ti[2]);
    }
}

}  // namespace

struct vistaf_shape_handle {
    int h = 0, w = 0, maxB = 0, K = 0;
    double fit_min_fraction = 0.0;
};

extern "C" {

void vistaf_shape_destroy(vistaf_shape_handle *sh) { delete sh; }

int vistaf_shape_create(int h, int w, int max_batch, int max_contacts, double fit_min_fraction, vistaf_shape_handle **out)
{
    if (!out) return set_error(VISTAF_E_INVALID, "null argument");
    *out = nullptr;
    if (h < 1 || w < 1 || (long long)h * w > 0x7fffffffll) return set_error(VISTAF_E_INVALID, "frame size must be >= 1 x 1 and below 2^31 pixels");
    if (max_batch < 1 || (long long)max_batch * VISTAF_MAX_CONTACTS > 0x7fffffffll) return set_error(VISTAF_E_INVALID, "max_batch must be 1..2^25");
    if (max_contacts < 1 || max_contacts > VISTAF_MAX_CONTACTS) return set_error(VISTAF_E_INVALID, "max_contacts must be 1..64");
    if (!(fit_min_fraction >= 0.0) || !(fit_min_fraction < 1.0)) return set_error(VISTAF_E_INVALID, "fit_min_fraction must be in [0, 1)");
    Created<vistaf_shape_handle> sh(new vistaf_shape_handle(), vistaf_shape_destroy);
    sh->h = h; sh->w = w; sh->maxB = max_batch; sh->K = max_contacts; sh->fit_min_fraction = fit_min_fraction;
    *out = sh.release();
    return 0;
}

int vistaf_shape_measure(vistaf_shape_handle *sh, const float *d_depth_mm, const int8_t *d_contact_index, const double *d_contacts,
                         const int32_t *d_count, const double *d_mm_per_px, float depth_eps_mm, int B, double *d_shapes, void *stream)
{
    if (!sh || !d_depth_mm || !d_contact_index || !d_contacts || !d_count || !d_mm_per_px || !d_shapes) return set_error(VISTAF_E_INVALID, "null argument");
    if (B < 1 || B > sh->maxB) return set_error(VISTAF_E_INVALID, "batch must be 1..max_batch");
    if (!std::isfinite(depth_eps_mm)) return set_error(VISTAF_E_INVALID, "depth_eps_mm must be finite");
    hipLaunchKernelGGL(k_shape, dim3((unsigned)(B * sh->K)), dim3(SH_NT), 0, (hipStream_t)stream, d_depth_mm, d_contact_index, d_contacts, d_count,
                       d_mm_per_px, depth_eps_mm, sh->fit_min_fraction, sh->h, sh->w, sh->K, d_shapes);
    return launch_ok("k_shape");
}

}  // extern "C"
