// Thermal read-out (include/vistaf_thermal.h): a temperature map of the photograph's frame registered into the aligned ROI crop with the record
// the aligner wrote, and reduced over the rows of the contacts table.  An extension, as the table, the tracker, the shapes and the taxels: the
// reference has no counterpart.  The definition is in the header; tests/thermal_helpers.py restates it in NumPy.
//
// vistaf_thermal_register: ONE launch.
//   k_thermal_register  grid (ceil(h*w / 256), B), one thread per crop pixel, consecutive lanes on consecutive x.  Threads 0..7 put the frame's
//                       eight transform doubles (shift, 2 x 3 warp) into LDS, one read per workgroup; every thread forms (u, v) in float64
//                       and gathers its four neighbours from the map -- neighbouring lanes read neighbouring floats as long as the warp is
//                       near the identity, which is what the aligner produces -- and stores one float32.
// vistaf_thermal_measure: TWO launches.
//   k_thermal_contacts  one workgroup per (frame, row), the box walk of k_shape: the pixels of the GROWN box in row-major order, pixel i to
//                       thread i mod TH_NT.  A pixel inside the table's own box can be a contact pixel of k, a pixel anywhere in the grown
//                       box can belong to the surround.  Three counts, four float64 sums and the two order keys of min / max stay in
//                       registers and are combined with the DPP tree inside a wave, then in wave order across waves.  Thread 0 finishes
//                       the mean; the workgroup walks the table's own box a second time (it sits in L2) for STD_C and thread 0 writes the row.
//   k_thermal_frame     one workgroup per frame, pixel i to thread i mod TF_NT over the whole frame, the same combination; thread 0 then reads
//                       the MEAN_C of the frame's rows, which the launch before it wrote, for the hottest and the coldest contact.  A frame
//                       is not split among workgroups: that would need a workspace, and neither call allocates.
// No memset, no atomics, no workspace: every float64 sum is formed in an order fixed by the box (or the frame) and the launch geometry (pixel ->
// lane -> wave -> workgroup), so two calls give the same bits and a frame's rows do not depend on the batch it is measured in.
#include <string>

#include "../../include/vistaf_align.h"
#include "../../include/vistaf_thermal.h"
#include "contact_rows.hpp"
#include "host_util.hpp"

using namespace vf;

namespace {

constexpr int TR_NT = 256;
constexpr int TH_NT = 512, TH_NW = TH_NT / 64;
constexpr int TF_NT = 1024, TF_NW = TF_NT / 64;

__global__ __launch_bounds__(TR_NT) void k_thermal_register(const float *__restrict__ map, const double *__restrict__ info, int use_shift, int h, int w,
                                                            int H, int W, int crop_x1, int crop_y1, float *__restrict__ crop)
{
    __shared__ double tr[8];                                         // sx, sy, M00, M01, M02, M10, M11, M12
    const int b = blockIdx.y, tid = threadIdx.x;
    if (tid < 8) {
        double v = (tid == 2 || tid == 6) ? 1.0 : 0.0;               // NULL info: no shift, identity
        if (info) {
            const double *row = info + (size_t)b * VISTAF_ALIGN_NINFO;
            if (tid >= 2) v = row[VISTAF_AI_WARP + tid - 2];
            else if (use_shift) v = row[tid == 0 ? VISTAF_AI_SHIFT_X : VISTAF_AI_SHIFT_Y];
        }
        tr[tid] = v;
    }
    __syncthreads();
    const size_t P = (size_t)h * w, i = (size_t)blockIdx.x * TR_NT + tid;
    if (i >= P) return;
    const int y = (int)(i / (size_t)w), x = (int)(i - (size_t)y * w);
    const double dx = (double)x, dy = (double)y;
    const double u = ((tr[2] * dx + tr[3] * dy) + tr[4]) + (double)crop_x1 - tr[0];
    const double v = ((tr[5] * dx + tr[6] * dy) + tr[7]) + (double)crop_y1 - tr[1];
    float t = nanf32();
    if (finitef(u) && finitef(v) && u >= 0.0 && u <= (double)(W - 1) && v >= 0.0 && v <= (double)(H - 1)) {
        int x0 = (int)floor(u), y0 = (int)floor(v);                  // 0 .. W-1, 0 .. H-1
        x0 = x0 > W - 2 ? W - 2 : x0;
        y0 = y0 > H - 2 ? H - 2 : y0;
        const double fx = u - (double)x0, fy = v - (double)y0;
        const float *p = map + (size_t)b * H * W + (size_t)y0 * W + x0;      // x0 + 1 <= W-1, y0 + 1 <= H-1
        const float t00 = p[0], t01 = p[1], t10 = p[W], t11 = p[W + 1];
        if (finitef(t00) && finitef(t01) && finitef(t10) && finitef(t11))
            t = (float)((1.0 - fy) * ((1.0 - fx) * (double)t00 + fx * (double)t01) + fy * ((1.0 - fx) * (double)t10 + fx * (double)t11));
    }
    crop[(size_t)b * P + i] = t;
}

__global__ __launch_bounds__(TH_NT) void k_thermal_contacts(const float *__restrict__ temp, const float *__restrict__ depth, const int8_t *__restrict__ index,
                                                            const double *__restrict__ contacts, const int32_t *__restrict__ count,
                                                            const int32_t *__restrict__ status, float eps, int margin, int h, int w, int K,
                                                            double *__restrict__ thermal)
{
    __shared__ double wf[TH_NW][4], tf[4];
    __shared__ uint32_t wi[TH_NW][5], ti[5];
    __shared__ double mean_s;
    const int b = blockIdx.x / K, k = blockIdx.x - b * K;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    double *out = thermal + (size_t)blockIdx.x * VISTAF_NTHERMAL;
    const int kk = clamp_count(count[b], K);
    if (nan_row(k >= kk || (status && status[b] != 0), out, VISTAF_NTHERMAL)) return;
    const double *row = contacts + (size_t)blockIdx.x * VISTAF_NCONTACT;
    const size_t P = (size_t)h * w;
    const float *tp = temp + b * P, *dp = depth + b * P;
    const int8_t *ip = index + b * P;
    // the box and the grown box, each clipped to the frame (|b..| <= 1e9, margin <= 4096: no overflow).  An inverted box is no box: it must
    // not grow into one
    const ContactBox box(row, h, w);
    const ContactBox grown(box.bx0 - margin, box.by0 - margin, box.bx1 + margin, box.by1 + margin, box.ok && box.bx1 >= box.bx0 && box.by1 >= box.by0, h, w);

    // ---- sweep 1 over the grown box: counts, sums, min / max keys
    uint32_t n = 0, nv = 0, ns = 0, kmax = 0, kmin = 0;             // kmin holds ~key: 0 = none for both
    double st = 0.0, sd = 0.0, sdt = 0.0, ss = 0.0;
    BoxWalk<TH_NT>(grown, tid).each([&](int px, int py) {
        const size_t p = (size_t)py * w + px;
        const int idx = ip[p];
        const float t = tp[p];
        const bool fin = finitef(t);
        if (idx == k && px >= box.x0 && px <= box.x1 && py >= box.y0 && py <= box.y1) {       // no pixel passes for a box outside the frame
            float d = dp[p];
            if (d != d) d = 0.0f;
            if (d > eps) {
                n++;
                if (fin) {
                    const double td = (double)t, dd = (double)d;
                    const uint32_t key = f2key(t);
                    nv++;
                    st += td; sd += dd; sdt += dd * td;
                    kmax = key > kmax ? key : kmax;
                    kmin = ~key > kmin ? ~key : kmin;
                }
            }
        } else if ((idx < 0 || idx >= kk) && fin) {
            ns++;
            ss += (double)t;
        }
    });
    // workgroup results: DPP tree in a wave, waves in order
    {
        const uint32_t c0 = wave_sum(n), c1 = wave_sum(nv), c2 = wave_sum(ns), c3 = wave_max_u32(kmax), c4 = wave_max_u32(kmin);
        const double f0 = wave_sum(st), f1 = wave_sum(sd), f2 = wave_sum(sdt), f3 = wave_sum(ss);
        if (lane == 0) {
            wi[wid][0] = c0; wi[wid][1] = c1; wi[wid][2] = c2; wi[wid][3] = c3; wi[wid][4] = c4;
            wf[wid][0] = f0; wf[wid][1] = f1; wf[wid][2] = f2; wf[wid][3] = f3;
        }
    }
    __syncthreads();
    if (tid < 5) {
        uint32_t s = 0;
        for (int q = 0; q < TH_NW; q++) s = tid < 3 ? s + wi[q][tid] : (wi[q][tid] > s ? wi[q][tid] : s);
        ti[tid] = s;
    } else if (tid >= 64 && tid < 68) {
        double s = 0.0;
        for (int q = 0; q < TH_NW; q++) s += wf[q][tid - 64];
        tf[tid - 64] = s;
    }
    __syncthreads();
    const uint32_t tn = ti[0], tnv = ti[1], tns = ti[2];
    if (tid == 0) {
        for (int j = 0; j < VISTAF_NTHERMAL; j++) out[j] = nan64();
        out[VISTAF_THERMAL_CONTACT_PIXELS] = (double)tn;
        out[VISTAF_THERMAL_VALID_PIXELS] = (double)tnv;
        out[VISTAF_THERMAL_SURROUND_PIXELS] = (double)tns;
        if (tn) out[VISTAF_THERMAL_COVERAGE] = (double)tnv / (double)tn;
        const double mean = tnv ? tf[0] / (double)tnv : nan64(), smean = tns ? tf[3] / (double)tns : nan64();
        if (tnv) {
            out[VISTAF_THERMAL_MEAN_C] = mean;
            out[VISTAF_THERMAL_WEIGHTED_MEAN_C] = tf[2] / tf[1];
            out[VISTAF_THERMAL_MAX_C] = (double)key2f(ti[3]);
            out[VISTAF_THERMAL_MIN_C] = (double)key2f(~ti[4]);
        }
        if (tns) out[VISTAF_THERMAL_SURROUND_MEAN_C] = smean;
        if (tnv && tns) out[VISTAF_THERMAL_CONTRAST_C] = mean - smean;
        const double a = row[VISTAF_CONTACT_ARGMAX_INDEX];
        if (finitef(a) && a >= 0.0 && a < (double)P) {
            const float t = tp[(size_t)a];
            if (finitef(t)) out[VISTAF_THERMAL_PEAK_TEMP_C] = (double)t;
        }
        mean_s = mean;
    }
    __syncthreads();
    if (!tnv) return;

    // ---- sweep 2 over the table's own box: squared deviations from the finished mean
    const double mean = mean_s;
    double s2 = 0.0;
    BoxWalk<TH_NT>(box, tid).each([&](int px, int py) {
        const size_t p = (size_t)py * w + px;
        const float t = tp[p];
        if (ip[p] == k && finitef(t)) {
            float d = dp[p];
            if (d != d) d = 0.0f;
            if (d > eps) {
                const double r = (double)t - mean;
                s2 += r * r;
            }
        }
    });
    s2 = wave_sum(s2);
    if (lane == 0) wf[wid][0] = s2;                                  // every read of wf[][0] lies before the barrier above
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int q = 0; q < TH_NW; q++) t += wf[q][0];
        out[VISTAF_THERMAL_STD_C] = sqrt(t / (double)tnv);
    }
}

__global__ __launch_bounds__(TF_NT) void k_thermal_frame(const float *__restrict__ temp, const float *__restrict__ depth, const int8_t *__restrict__ index,
                                                         const int32_t *__restrict__ count, const int32_t *__restrict__ status, float eps, int h, int w, int K,
                                                         const double *__restrict__ thermal, double *__restrict__ frame)
{
    __shared__ double wf[TF_NW][2];
    __shared__ uint32_t wi[TF_NW][3];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    double *out = frame + (size_t)b * VISTAF_NTHERMALFRAME;
    if (status && status[b] != 0) {
        if (tid < VISTAF_NTHERMALFRAME) out[tid] = nan64();
        return;
    }
    const int kk = clamp_count(count[b], K);
    const size_t P = (size_t)h * w;
    const float *tp = temp + b * P, *dp = depth + b * P;
    const int8_t *ip = index + b * P;
    uint32_t nreg = 0, nskin = 0, ncon = 0;                          // < 2^31 pixels in a frame
    double sskin = 0.0, scon = 0.0;
    for (size_t p = tid; p < P; p += TF_NT) {
        const float t = tp[p];
        if (!finitef(t)) continue;
        nreg++;
        const int idx = ip[p];
        if (idx < 0 || idx >= kk) {
            nskin++;
            sskin += (double)t;
        } else {
            float d = dp[p];
            if (d != d) d = 0.0f;
            if (d > eps) {
                ncon++;
                scon += (double)t;
            }
        }
    }
    {
        const uint32_t c0 = wave_sum(nreg), c1 = wave_sum(nskin), c2 = wave_sum(ncon);
        const double f0 = wave_sum(sskin), f1 = wave_sum(scon);
        if (lane == 0) {
            wi[wid][0] = c0; wi[wid][1] = c1; wi[wid][2] = c2;
            wf[wid][0] = f0; wf[wid][1] = f1;
        }
    }
    __syncthreads();
    if (tid != 0) return;
    uint32_t c[3] = {0, 0, 0};
    double f[2] = {0.0, 0.0};
    for (int q = 0; q < TF_NW; q++) {
        c[0] += wi[q][0]; c[1] += wi[q][1]; c[2] += wi[q][2];
        f[0] += wf[q][0]; f[1] += wf[q][1];
    }
    for (int j = 0; j < VISTAF_NTHERMALFRAME; j++) out[j] = nan64();
    out[VISTAF_THERMALFRAME_REGISTERED_PIXELS] = (double)c[0];
    out[VISTAF_THERMALFRAME_CONTACT_PIXELS] = (double)c[2];
    const double skin = c[1] ? f[0] / (double)c[1] : nan64(), con = c[2] ? f[1] / (double)c[2] : nan64();
    if (c[1]) out[VISTAF_THERMALFRAME_SKIN_MEAN_C] = skin;
    if (c[2]) out[VISTAF_THERMALFRAME_CONTACT_MEAN_C] = con;
    if (c[1] && c[2]) out[VISTAF_THERMALFRAME_CONTRAST_C] = con - skin;
    // the rows of this frame, written by k_thermal_contacts in the launch before
    int hot = -1, cold = -1;
    double vhot = 0.0, vcold = 0.0;
    for (int k = 0; k < kk; k++) {
        const double m = thermal[((size_t)b * K + k) * VISTAF_NTHERMAL + VISTAF_THERMAL_MEAN_C];
        if (m != m) continue;
        if (hot < 0 || m > vhot) { hot = k; vhot = m; }
        if (cold < 0 || m < vcold) { cold = k; vcold = m; }
    }
    if (hot >= 0) {
        out[VISTAF_THERMALFRAME_HOTTEST_CONTACT] = (double)hot;
        out[VISTAF_THERMALFRAME_COLDEST_CONTACT] = (double)cold;
    }
}

}  // namespace

struct vistaf_thermal_handle {
    int h = 0, w = 0, H = 0, W = 0, crop_x1 = 0, crop_y1 = 0, use_shift = 0, maxB = 0, K = 0, margin = 0;
};

extern "C" {

void vistaf_thermal_destroy(vistaf_thermal_handle *th) { delete th; }

int vistaf_thermal_create(int h, int w, int H, int W, int crop_x1, int crop_y1, int apply_global_shift, int max_batch, int max_contacts,
                          int surround_margin_px, vistaf_thermal_handle **out)
{
    if (!out) return set_error(VISTAF_E_INVALID, "null argument: out");
    *out = nullptr;
    if (h < 1 || w < 1 || h > 65536 || w > 65536 || (long long)h * w >= 0x80000000ll)
        return set_error(VISTAF_E_INVALID, "crop size h, w must be 1..65536 each way and below 2^31 pixels");
    if (H < 2 || W < 2 || (long long)H * W >= 0x80000000ll) return set_error(VISTAF_E_INVALID, "photograph size H, W must be >= 2 each way and below 2^31 pixels");
    if (crop_x1 < -(1 << 20) || crop_x1 > (1 << 20) || crop_y1 < -(1 << 20) || crop_y1 > (1 << 20))
        return set_error(VISTAF_E_INVALID, "crop_x1, crop_y1 must be within +-2^20");
    if (max_batch < 1 || max_batch > 65535) return set_error(VISTAF_E_INVALID, "max_batch must be 1..65535");
    if (max_contacts < 1 || max_contacts > VISTAF_MAX_CONTACTS) return set_error(VISTAF_E_INVALID, "max_contacts must be 1..64");
    if (surround_margin_px < 0 || surround_margin_px > 4096) return set_error(VISTAF_E_INVALID, "surround_margin_px must be 0..4096");
    Created<vistaf_thermal_handle> th(new vistaf_thermal_handle(), vistaf_thermal_destroy);
    th->h = h; th->w = w; th->H = H; th->W = W; th->crop_x1 = crop_x1; th->crop_y1 = crop_y1; th->use_shift = apply_global_shift != 0;
    th->maxB = max_batch; th->K = max_contacts; th->margin = surround_margin_px;
    *out = th.release();
    return 0;
}

#define TH_NOT_NULL(p)                                                                      \
    do {                                                                                    \
        if (!(p)) return set_error(VISTAF_E_INVALID, std::string("null argument: ") + #p); \
    } while (0)

int vistaf_thermal_register(vistaf_thermal_handle *th, const float *d_temp_map, const double *d_align_info, int batch, float *d_temp_crop, void *stream)
{
    TH_NOT_NULL(th);
    TH_NOT_NULL(d_temp_map);
    TH_NOT_NULL(d_temp_crop);
    if (batch < 1 || batch > th->maxB) return set_error(VISTAF_E_INVALID, "batch must be 1..max_batch");
    const size_t P = (size_t)th->h * th->w;
    hipLaunchKernelGGL(k_thermal_register, dim3((unsigned)((P + TR_NT - 1) / TR_NT), (unsigned)batch), dim3(TR_NT), 0, (hipStream_t)stream, d_temp_map,
                       d_align_info, th->use_shift, th->h, th->w, th->H, th->W, th->crop_x1, th->crop_y1, d_temp_crop);
    return launch_ok("k_thermal_register");
}

int vistaf_thermal_measure(vistaf_thermal_handle *th, const float *d_temp_crop, const float *d_depth_mm, const int8_t *d_contact_index,
                           const double *d_contacts, const int32_t *d_count, const int32_t *d_status, float depth_eps_mm, int batch,
                           double *d_thermal, double *d_frame, void *stream)
{
    TH_NOT_NULL(th);
    TH_NOT_NULL(d_temp_crop);
    TH_NOT_NULL(d_depth_mm);
    TH_NOT_NULL(d_contact_index);
    TH_NOT_NULL(d_contacts);
    TH_NOT_NULL(d_count);
    TH_NOT_NULL(d_thermal);
    TH_NOT_NULL(d_frame);
    if (batch < 1 || batch > th->maxB) return set_error(VISTAF_E_INVALID, "batch must be 1..max_batch");
    if (!std::isfinite(depth_eps_mm)) return set_error(VISTAF_E_INVALID, "depth_eps_mm must be finite");
    hipLaunchKernelGGL(k_thermal_contacts, dim3((unsigned)(batch * th->K)), dim3(TH_NT), 0, (hipStream_t)stream, d_temp_crop, d_depth_mm, d_contact_index,
                       d_contacts, d_count, d_status, depth_eps_mm, th->margin, th->h, th->w, th->K, d_thermal);
    hipLaunchKernelGGL(k_thermal_frame, dim3((unsigned)batch), dim3(TF_NT), 0, (hipStream_t)stream, d_temp_crop, d_depth_mm, d_contact_index, d_count,
                       d_status, depth_eps_mm, th->h, th->w, th->K, (const double *)d_thermal, d_frame);
    return launch_ok("k_thermal_measure");
}

}  // extern "C"
