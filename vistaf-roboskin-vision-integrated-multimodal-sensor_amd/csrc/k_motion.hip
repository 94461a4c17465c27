// Contact motion read-out (include/vistaf_motion.h): slide, twist and lift of every tracked contact, by an inverse-compositional Gauss-Newton
// registration of the depth surface the parent left in the frame before onto the current depth plane.  An extension, as the tracker and the
// shape read-out: the reference has no counterpart.  The definition is in the header; tests/motion_helpers.py restates it in NumPy.
//
//   k_motion         ONE launch registers every (frame, row): grid (K, B), one workgroup per pair.  All pairs are independent -- frame b > 0
//                    reads frame b - 1 of the same batch, frame 0 the planes the handle carried over.  The workgroup walks the parent's box
//                    as k_shape does (pixel i to thread i mod MO_NT, consecutive lanes on consecutive bytes of the int8 plane) and keeps the
//                    whole Gauss-Newton loop inside the kernel: sweep 0 counts the template pixels and sums their coordinates (exact
//                    integers), sweep 1 forms the nine sums of H, then `iterations` + 1 sweeps form b and rss with the current warp.  Sums go
//                    lane -> wave over the DPP tree and wave -> workgroup in wave order through LDS; after ONE barrier every thread adds the
//                    wave partials in the same order, solves the 4 x 4 system with chol_solve<4> and composes the warp, so every thread holds
//                    the same state bit for bit, every exit is workgroup-uniform and no step goes back to the host.  The partials ping-pong
//                    between two LDS slots, which is what makes one barrier per sweep enough.  The template (T, its four neighbours, the
//                    index byte) is re-read from L2 in every sweep: a box is a few KB and stays resident, see DESIGN.md.
//   k_motion_frames  one wave per frame, lane = row: stages what the frame row needs in LDS, lane 0 goes through the rows in ascending order.
//   k_motion_carry   copies the last frame's depth plane, index plane, table and count into the carried buffers, after k_motion read them
//                    (stream order).
// No memset, no atomics: every float64 sum is formed in an order fixed by the box and the launch geometry, so two updates, two handles or
// another position in a batch give the same bits.
#include <string>

#include "../../include/vistaf_motion.h"
#include "../../include/vistaf_track.h"
#include "chol.hpp"
#include "contact_rows.hpp"
#include "host_util.hpp"

using namespace vf;

namespace {

constexpr int MO_NT = 256, MO_NW = MO_NT / 64;
constexpr int MO_NH = 9, MO_NB = 5;                     // float64 sums of H beside n; of a sweep (b0..b3, rss)
constexpr double MO_PIVOT_FLOOR = 1.0 / 4294967296.0;   // 2^-32 of the diagonal (header, step 2)

// the carried frame and nothing else: the one device buffer of a handle
struct MoBufs {
    float *depth;
    int8_t *index;
    double *table;
    int32_t *count;
};

// base == nullptr sizes the buffer the first update allocates, the same call with the pointer carves it
MoBufs motion_scratch(ScratchLayout &L, size_t P, int K)
{
    MoBufs bf;
    bf.depth = L.take<float>(P, 256, "carry_depth");
    bf.index = L.take<int8_t>(P, 256, "carry_index");
    bf.table = L.take<double>((size_t)K * VISTAF_NCONTACT, 256, "carry_table");
    bf.count = L.take<int32_t>(1, 256, "carry_count");
    return bf;
}

__device__ inline int mo_clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

struct MoPlane {
    const float *d;
    int h, w;
    __device__ inline float at32(int x, int y) const       // inside the frame; a value that is not finite counts as 0
    {
        const float v = d[(size_t)y * w + x];
        return finitef(v) ? v : 0.0f;
    }
    __device__ inline double at(int x, int y) const { return (double)at32(mo_clampi(x, w - 1), mo_clampi(y, h - 1)); }
    __device__ inline double sample(double wx, double wy) const       // header, step 3
    {
        const double mx = (double)(w - 1), my = (double)(h - 1);
        const double qx = wx >= 0.0 ? (wx <= mx ? wx : mx) : 0.0, qy = wy >= 0.0 ? (wy <= my ? wy : my) : 0.0;
        const int x0 = (int)qx, y0 = (int)qy;
        const int x1 = x0 + 1 > w - 1 ? w - 1 : x0 + 1, y1 = y0 + 1 > h - 1 ? h - 1 : y0 + 1;
        const double fx = qx - (double)x0, fy = qy - (double)y0;
        const double top = (1.0 - fx) * (double)at32(x0, y0) + fx * (double)at32(x1, y0);
        const double bot = (1.0 - fx) * (double)at32(x0, y1) + fx * (double)at32(x1, y1);
        return (1.0 - fy) * top + fy * bot;
    }
};

struct MoState { double tx, ty, theta, beta; };

// workgroup sums of N doubles: DPP tree in a wave, waves in order; every thread returns with the totals.  One barrier: `slot` alternates
template <int N>
__device__ inline void mo_reduce(double (&v)[N], double (*slot)[MO_NH], int lane, int wid)
{
#pragma unroll
    for (int j = 0; j < N; j++) {
        const double s = wave_sum(v[j]);
        if (lane == 0) slot[wid][j] = s;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < N; j++) {
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < MO_NW; q++) s += slot[q][j];
        v[j] = s;
    }
}

__global__ __launch_bounds__(MO_NT) void k_motion(const float *__restrict__ depth, const int8_t *__restrict__ index, const double *__restrict__ contacts,
                                                  const int32_t *__restrict__ count, const double *__restrict__ tracks, const double *__restrict__ mm_per_px,
                                                  const float *__restrict__ carry_depth, const int8_t *__restrict__ carry_index,
                                                  const double *__restrict__ carry_table, const int32_t *__restrict__ carry_count, int have_carry,
                                                  float eps, int h, int w, int K, int iterations, double tol_px, int min_pixels, int init_centroid,
                                                  double *__restrict__ motion)
{
    __shared__ double part[2][MO_NW][MO_NH];
    __shared__ unsigned long long wi[MO_NW][3];
    const int k = blockIdx.x, t = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    double *out = motion + ((size_t)t * K + k) * VISTAF_NMOTION;
    if (nan_row(k >= clamp_count(count[t], K), out, VISTAF_NMOTION)) return;
    const int m = clamp_count(t ? count[t - 1] : (have_carry ? carry_count[0] : 0), K);
    const double *trow = tracks + ((size_t)t * K + k) * VISTAF_NTRACK;
    const double pr = trow[VISTAF_TRACK_PARENT_ROW], DX = trow[VISTAF_TRACK_DX], DY = trow[VISTAF_TRACK_DY];
    if (!finitef(pr) || pr < 0.0 || pr >= (double)m) {
        if (tid < VISTAF_NMOTION) {
            double v = nan64();
            if (tid == VISTAF_MOTION_PARENT_ROW) v = finitef(pr) ? pr : -1.0;
            if (tid == VISTAF_MOTION_TEMPLATE_PIXELS || tid == VISTAF_MOTION_ITERATIONS) v = 0.0;
            if (tid == VISTAF_MOTION_STATUS) v = (double)VISTAF_MOTIONST_NO_PARENT;
            out[tid] = v;
        }
        return;
    }
    const int p = (int)pr;
    const size_t P = (size_t)h * w;
    const MoPlane T{t ? depth + (size_t)(t - 1) * P : carry_depth, h, w}, I{depth + (size_t)t * P, h, w};
    const int8_t *pidx = t ? index + (size_t)(t - 1) * P : carry_index;
    const double *prow = (t ? contacts + (size_t)(t - 1) * K * VISTAF_NCONTACT : carry_table) + (size_t)p * VISTAF_NCONTACT;
    const ContactBox box(prow, h, w);                       // the parent's
    const double R = 0.5 * sqrt((double)box.bw * (double)box.bw + (double)box.bh * (double)box.bh);
    const BoxWalk<MO_NT> walk(box, tid);
    // is (x, y), inside the frame, a template pixel; d = its depth
    auto templ = [&](int x, int y, float &d) {
        d = T.at32(x, y);
        return (int)pidx[(size_t)y * w + x] == p && d > eps;
    };

    // ---- sweep 0: n and the centre, exact integers
    unsigned long long n = 0, sx = 0, sy = 0;
    walk.each([&](int x, int y) {
        float d;
        if (templ(x, y, d)) { n++; sx += (unsigned long long)x; sy += (unsigned long long)y; }
    });
    n = wave_sum(n); sx = wave_sum(sx); sy = wave_sum(sy);
    if (lane == 0) { wi[wid][0] = n; wi[wid][1] = sx; wi[wid][2] = sy; }
    __syncthreads();
    n = sx = sy = 0;
#pragma unroll
    for (int q = 0; q < MO_NW; q++) { n += wi[q][0]; sx += wi[q][1]; sy += wi[q][2]; }
    const double dn = (double)n, cx = (double)sx / dn, cy = (double)sy / dn;
    auto head = [&](int status, int iters) {               // thread 0: the fields every status has, the rest NaN
        for (int j = 0; j < VISTAF_NMOTION; j++) out[j] = nan64();
        out[VISTAF_MOTION_PARENT_ROW] = (double)p;
        out[VISTAF_MOTION_TEMPLATE_PIXELS] = dn;
        out[VISTAF_MOTION_STATUS] = (double)status;
        out[VISTAF_MOTION_ITERATIONS] = (double)iters;
        if (n) { out[VISTAF_MOTION_CENTRE_X] = cx; out[VISTAF_MOTION_CENTRE_Y] = cy; }
    };
    if (n < (unsigned long long)min_pixels) {
        if (tid == 0) head(VISTAF_MOTIONST_TOO_FEW, 0);
        return;
    }

    // ---- sweep 1: H
    double hs[MO_NH];
#pragma unroll
    for (int j = 0; j < MO_NH; j++) hs[j] = 0.0;
    walk.each([&](int x, int y) {
        float d;
        if (!templ(x, y, d)) return;
        const double Tx = (T.at(x + 1, y) - T.at(x - 1, y)) / 2.0, Ty = (T.at(x, y + 1) - T.at(x, y - 1)) / 2.0;
        const double ux = (double)x - cx, uy = (double)y - cy, g2 = ux * Ty - uy * Tx;
        hs[0] += Tx * Tx; hs[1] += Tx * Ty; hs[2] += Tx * g2; hs[3] += Tx; hs[4] += Ty * Ty; hs[5] += Ty * g2; hs[6] += Ty;
        hs[7] += g2 * g2; hs[8] += g2;
    });
    mo_reduce<MO_NH>(hs, part[0], lane, wid);
    double H[6][6] = {}, H2[6][6] = {}, rhs[6] = {0, 0, 0, 0, 0, 0};
    H[0][0] = hs[0]; H[0][1] = H[1][0] = hs[1]; H[0][2] = H[2][0] = hs[2]; H[0][3] = H[3][0] = hs[3];
    H[1][1] = hs[4]; H[1][2] = H[2][1] = hs[5]; H[1][3] = H[3][1] = hs[6];
    H[2][2] = hs[7]; H[2][3] = H[3][2] = hs[8]; H[3][3] = dn;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) H2[i][j] = i == j ? H[i][j] - MO_PIVOT_FLOOR * H[i][j] : H[i][j];
    if (!(chol_solve<4>(H2, rhs) && chol_solve<4>(H, rhs))) {
        if (tid == 0) head(VISTAF_MOTIONST_SINGULAR, 0);
        return;
    }

    // ---- the Gauss-Newton loop: `iterations` steps and the final sweep
    MoState st{0.0, 0.0, 0.0, 0.0};
    if (init_centroid && finitef(DX) && finitef(DY)) { st.tx = DX; st.ty = DY; }
    double c = cos(st.theta), sn = sin(st.theta), rss_before = 0.0, rss_after = 0.0, last_step = 0.0;
    for (int it = 0; it <= iterations; it++) {
        double bs[MO_NB];
#pragma unroll
        for (int j = 0; j < MO_NB; j++) bs[j] = 0.0;
        walk.each([&](int x, int y) {
            float d;
            if (!templ(x, y, d)) return;
            const double Tx = (T.at(x + 1, y) - T.at(x - 1, y)) / 2.0, Ty = (T.at(x, y + 1) - T.at(x, y - 1)) / 2.0;
            const double ux = (double)x - cx, uy = (double)y - cy, g2 = ux * Ty - uy * Tx;
            const double wx = ((cx + c * ux) - sn * uy) + st.tx, wy = ((cy + sn * ux) + c * uy) + st.ty;
            const double r = (I.sample(wx, wy) - st.beta) - (double)d;
            bs[0] += Tx * r; bs[1] += Ty * r; bs[2] += g2 * r; bs[3] += r; bs[4] += r * r;
        });
        mo_reduce<MO_NB>(bs, part[(it + 1) & 1], lane, wid);
        if (it == 0) rss_before = bs[4];
        if (it == iterations) { rss_after = bs[4]; break; }
        double dl[6] = {bs[0], bs[1], bs[2], bs[3], 0, 0};
        chol_solve<4>(H, dl);                              // H passed the test above: the same pivots, it succeeds
        st.theta = st.theta - dl[2];
        c = cos(st.theta); sn = sin(st.theta);
        st.tx = st.tx - (c * dl[0] - sn * dl[1]);
        st.ty = st.ty - (sn * dl[0] + c * dl[1]);
        st.beta = st.beta + dl[3];
        last_step = fmax(fmax(fabs(dl[0]), fabs(dl[1])), fabs(dl[2]) * R);
        if (dl[0] != dl[0] || dl[1] != dl[1] || dl[2] != dl[2]) last_step = nan64();       // fmax drops a NaN
    }
    if (tid != 0) return;
    const double s = mm_per_px[t];
    head(last_step <= tol_px ? VISTAF_MOTIONST_OK : VISTAF_MOTIONST_NOT_CONVERGED, iterations);
    out[VISTAF_MOTION_TX_PX] = st.tx;
    out[VISTAF_MOTION_TY_PX] = st.ty;
    out[VISTAF_MOTION_THETA_RAD] = st.theta;
    out[VISTAF_MOTION_BETA_MM] = st.beta;
    out[VISTAF_MOTION_TX_MM] = st.tx * s;
    out[VISTAF_MOTION_TY_MM] = st.ty * s;
    out[VISTAF_MOTION_RMS_BEFORE_MM] = sqrt(rss_before / dn);
    out[VISTAF_MOTION_RMS_AFTER_MM] = sqrt(rss_after / dn);
    out[VISTAF_MOTION_LAST_STEP_PX] = last_step;
    const double dof = n > 5 ? (double)(n - 4) : 1.0, var = rss_after / dof;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        double e[6] = {0, 0, 0, 0, 0, 0};
        e[i] = 1.0;
        chol_solve<4>(H, e);
        out[VISTAF_MOTION_SE_TX_PX + i] = sqrt(e[i] * var);
    }
    const double fx = st.tx - DX, fy = st.ty - DY;
    out[VISTAF_MOTION_TX_MINUS_DX] = fx != fx ? nan64() : fx;
    out[VISTAF_MOTION_TY_MINUS_DY] = fy != fy ? nan64() : fy;
}

__global__ __launch_bounds__(64) void k_motion_frames(const double *__restrict__ motion, const int32_t *__restrict__ count, int K, double *__restrict__ frame)
{
    __shared__ double sn[64], stx[64], sty[64], sth[64], srms[64];
    __shared__ int sok[64];
    const int b = blockIdx.x, lane = threadIdx.x;
    double *o = frame + (size_t)b * VISTAF_NMOTIONFRAME;
    const int kk = clamp_count(count[b], K);
    if (kk == 0) {
        if (lane < VISTAF_NMOTIONFRAME) o[lane] = nan64();
        return;
    }
    sok[lane] = 0;
    if (lane < kk) {
        const double *r = motion + ((size_t)b * K + lane) * VISTAF_NMOTION;
        sok[lane] = r[VISTAF_MOTION_STATUS] == (double)VISTAF_MOTIONST_OK;
        sn[lane] = r[VISTAF_MOTION_TEMPLATE_PIXELS];
        stx[lane] = r[VISTAF_MOTION_TX_MM];
        sty[lane] = r[VISTAF_MOTION_TY_MM];
        sth[lane] = r[VISTAF_MOTION_THETA_RAD];
        srms[lane] = r[VISTAF_MOTION_RMS_AFTER_MM];
    }
    __syncthreads();
    if (lane != 0) return;
    int ok = 0, slide_row = -1, twist_row = -1;
    double slide = 0.0, twist = 0.0, wn = 0.0, wx = 0.0, wy = 0.0, wr = 0.0;
    for (int k = 0; k < kk; k++) {
        if (!sok[k]) continue;
        ok++;
        const double sl = sqrt(stx[k] * stx[k] + sty[k] * sty[k]), tw = fabs(sth[k]);
        if (slide_row < 0 || sl > slide) { slide = sl; slide_row = k; }
        if (twist_row < 0 || tw > twist) { twist = tw; twist_row = k; }
        wn += sn[k]; wx += sn[k] * stx[k]; wy += sn[k] * sty[k]; wr += sn[k] * srms[k];
    }
    o[VISTAF_MOTIONFRAME_REGISTERED] = (double)ok;
    o[VISTAF_MOTIONFRAME_MAX_SLIDE_MM] = ok ? slide : nan64();
    o[VISTAF_MOTIONFRAME_MAX_SLIDE_ROW] = ok ? (double)slide_row : nan64();
    o[VISTAF_MOTIONFRAME_MAX_TWIST_RAD] = ok ? twist : nan64();
    o[VISTAF_MOTIONFRAME_MAX_TWIST_ROW] = ok ? (double)twist_row : nan64();
    o[VISTAF_MOTIONFRAME_MEAN_TX_MM] = ok ? wx / wn : nan64();
    o[VISTAF_MOTIONFRAME_MEAN_TY_MM] = ok ? wy / wn : nan64();
    o[VISTAF_MOTIONFRAME_MEAN_RMS_AFTER_MM] = ok ? wr / wn : nan64();
}

__global__ __launch_bounds__(256) void k_motion_carry(const float *__restrict__ depth, const int8_t *__restrict__ index, const double *__restrict__ table,
                                                      const int32_t *__restrict__ count, unsigned P, unsigned ntab, float *__restrict__ carry_depth,
                                                      int8_t *__restrict__ carry_index, double *__restrict__ carry_table, int32_t *__restrict__ carry_count)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i < P) { carry_depth[i] = depth[i]; carry_index[i] = index[i]; }
    if (i < ntab) carry_table[i] = table[i];
    if (i == 0) carry_count[0] = count[0];
}

}  // namespace

struct vistaf_motion_handle {
    int h = 0, w = 0, maxB = 0, K = 0, iterations = 0, min_pixels = 0, init_centroid = 0;
    double tol_px = 0.0;
    bool have_carry = false;               // false after create and reset: frame 0 of the next update has no frame before it
    void *buf = nullptr;
    MoBufs bf = {};
    DeviceAllocs mem;
};

extern "C" {

void vistaf_motion_destroy(vistaf_motion_handle *mo)
{
    if (!mo) return;
    mo->mem.free_all();
    delete mo;
}

int vistaf_motion_create(int h, int w, int max_batch, int max_contacts, int iterations, double tol_px, int min_pixels, int init_from_centroid,
                         vistaf_motion_handle **out)
{
    if (!out) return set_error(VISTAF_E_INVALID, "null argument: out");
    *out = nullptr;
    if (h < 1 || w < 1 || (long long)h * w > 0x7fffffffll) return set_error(VISTAF_E_INVALID, "frame size must be >= 1 x 1 and below 2^31 pixels");
    if (max_batch < 1 || max_batch > 65535) return set_error(VISTAF_E_INVALID, "max_batch must be 1..65535");
    if (max_contacts < 1 || max_contacts > VISTAF_MAX_CONTACTS) return set_error(VISTAF_E_INVALID, "max_contacts must be 1..64");
    if (iterations < 1 || iterations > 16) return set_error(VISTAF_E_INVALID, "iterations must be 1..16");
    if (!(tol_px >= 0.0) || !std::isfinite(tol_px)) return set_error(VISTAF_E_INVALID, "tol_px must be finite and >= 0");
    if (min_pixels < 1) return set_error(VISTAF_E_INVALID, "min_pixels must be >= 1");
    if (init_from_centroid != 0 && init_from_centroid != 1) return set_error(VISTAF_E_INVALID, "init_from_centroid must be 0 or 1");
    Created<vistaf_motion_handle> mo(new vistaf_motion_handle(), vistaf_motion_destroy);
    mo->h = h; mo->w = w; mo->maxB = max_batch; mo->K = max_contacts; mo->iterations = iterations; mo->tol_px = tol_px;
    mo->min_pixels = min_pixels; mo->init_centroid = init_from_centroid;
    *out = mo.release();
    return 0;
}

int vistaf_motion_reset(vistaf_motion_handle *mo)
{
    if (!mo) return set_error(VISTAF_E_INVALID, "null argument: handle");
    mo->have_carry = false;
    return 0;
}

int vistaf_motion_update(vistaf_motion_handle *mo, const float *d_depth_mm, const int8_t *d_contact_index, const double *d_contacts,
                         const int32_t *d_count, const double *d_tracks, const double *d_mm_per_px, float depth_eps_mm, int B, double *d_motion,
                         double *d_frame, void *stream)
{
    if (!mo) return set_error(VISTAF_E_INVALID, "null argument: handle");
    if (!d_depth_mm) return set_error(VISTAF_E_INVALID, "null argument: depth_mm");
    if (!d_contact_index) return set_error(VISTAF_E_INVALID, "null argument: contact_index");
    if (!d_contacts) return set_error(VISTAF_E_INVALID, "null argument: contacts");
    if (!d_count) return set_error(VISTAF_E_INVALID, "null argument: count");
    if (!d_tracks) return set_error(VISTAF_E_INVALID, "null argument: tracks");
    if (!d_mm_per_px) return set_error(VISTAF_E_INVALID, "null argument: mm_per_px");
    if (!d_motion) return set_error(VISTAF_E_INVALID, "null argument: motion");
    if (!d_frame) return set_error(VISTAF_E_INVALID, "null argument: frame");
    if (B < 1 || B > mo->maxB) return set_error(VISTAF_E_INVALID, "batch must be 1..max_batch");
    if (!std::isfinite(depth_eps_mm)) return set_error(VISTAF_E_INVALID, "depth_eps_mm must be finite");
    if (((uintptr_t)d_depth_mm & 3u) || ((uintptr_t)d_count & 3u))
        return set_error(VISTAF_E_INVALID, "depth_mm and count must be 4-byte aligned");
    if (((uintptr_t)d_contacts & 7u) || ((uintptr_t)d_tracks & 7u) || ((uintptr_t)d_mm_per_px & 7u) || ((uintptr_t)d_motion & 7u) || ((uintptr_t)d_frame & 7u))
        return set_error(VISTAF_E_INVALID, "contacts, tracks, mm_per_px, motion and frame must be 8-byte aligned");
    const size_t P = (size_t)mo->h * mo->w;
    const int K = mo->K;
    TRY(ensure_carved(mo->mem, mo->buf, &mo->bf, [&](ScratchLayout &L) { return motion_scratch(L, P, K); }));
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_motion, dim3((unsigned)K, (unsigned)B), dim3(MO_NT), 0, st, d_depth_mm, d_contact_index, d_contacts, d_count, d_tracks, d_mm_per_px,
                       mo->bf.depth, mo->bf.index, mo->bf.table, mo->bf.count, mo->have_carry ? 1 : 0, depth_eps_mm, mo->h, mo->w, K, mo->iterations,
                       mo->tol_px, mo->min_pixels, mo->init_centroid, d_motion);
    hipLaunchKernelGGL(k_motion_frames, dim3((unsigned)B), dim3(64), 0, st, d_motion, d_count, K, d_frame);
    const unsigned ntab = (unsigned)(K * VISTAF_NCONTACT), ncopy = (unsigned)P > ntab ? (unsigned)P : ntab;
    hipLaunchKernelGGL(k_motion_carry, dim3((ncopy + 255u) / 256u), dim3(256), 0, st, d_depth_mm + (size_t)(B - 1) * P, d_contact_index + (size_t)(B - 1) * P,
                       d_contacts + (size_t)(B - 1) * K * VISTAF_NCONTACT, d_count + (B - 1), (unsigned)P, ntab, mo->bf.depth, mo->bf.index, mo->bf.table,
                       mo->bf.count);
    if (int rc = launch_ok("k_motion / k_motion_frames / k_motion_carry")) return rc;
    mo->have_carry = true;
    return 0;
}

}  // extern "C"
