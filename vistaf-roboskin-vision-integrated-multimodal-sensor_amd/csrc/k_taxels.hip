// Taxel read-out (include/vistaf_taxel.h): a depth plane reduced to a fixed array of cells -- pixels, area, volume, mean and peak depth,
// centroid, a share of the frame's force and a pressure per taxel -- and to the frame's wrench.  An extension, as the contacts table, the
// tracker and the shape read-out: the reference has no counterpart.  The definition is in the header; tests/taxels_helpers.py restates it.
//
// The layout is an arbitrary label map, and the float64 sums of a taxel must not depend on the order in which pixels arrive, so the frame is
// not scanned into per-taxel accumulators.  vistaf_taxel_create inverts the map once, on the host: the pixels sorted by (taxel, index), each
// packed as y << 16 | x, and start[T + 1]; and it lays out the launch, one SLOT per wave: a taxel of at most TX_WAVE_PIXELS pixels gets
// one slot, a larger one 2, 4 or all TX_NW slots of one workgroup, slots handed out in taxel order (a workgroup is padded with idle slots
// when the next taxel does not fit).  The lists go to the device at the first measure.
//
//   k_taxel_sums   grid (workgroups of the slot table, B).  The wave of slot (t, part of parts) strides over the taxel's list from
//                  start[t] + 64*part + lane in steps of 64*parts, four pixels in flight, and gathers depth[b*P + y*w + x]: the list is shared
//                  by every frame of the batch and stays in L2, a grid cell's list is runs of consecutive pixels, so the gathers coalesce.
//                  Every lane keeps n, S, Sx, Sy and the (depth, lowest index) maximum as one ordered 64-bit key; the wave reduces them on
//                  the DPP network, leaves them in LDS, and after one barrier lane 0 of a taxel's part 0 adds the parts in order and writes
//                  the row.  S, Sx and Sy are parked in fields 8, 10 and 11 of the row for the second kernel.
//   k_taxel_frame  one wave per frame.  It walks the T rows in taxel order, 64 rows per step -- each lane loads one row's S, Sx, Sy, the wave
//                  adds them lane by lane through readlane, so the sums are the sequential sums of the definition -- then walks the rows
//                  again, a row per lane, for the force share and the pressure, restores the reserved fields to NaN and writes the frame row.
// Two launches, no memset, no atomics, nothing allocated after the first call: every sum is formed in an order fixed by the layout and the
// launch geometry (pixel -> lane -> wave part -> taxel), so two calls give the same bits and a frame's rows do not depend on its batch.
// Every address is guarded by the handle's own numbers: the lists are validated at create, T, P and the slot table never come from device data.
#include <string>
#include <vector>

#include "../../include/vistaf_taxel.h"
#include "host_util.hpp"

using namespace vf;

namespace {

constexpr int TX_NW = 8, TX_NT = TX_NW * 64;            // waves (slots) and threads of a workgroup of k_taxel_sums
constexpr unsigned TX_WAVE_PIXELS = 1024;               // a taxel gets a second slot beyond this many pixels (16 per lane)
constexpr int TX_S = VISTAF_TAXEL_FORCE_N, TX_SX = 10, TX_SY = 11;      // where k_taxel_sums parks S, Sx, Sy for k_taxel_frame

struct TxSlot { int32_t taxel; int32_t part; };         // taxel < 0: idle; part = index | parts << 8

struct TxAcc {
    double S = 0.0, Sx = 0.0, Sy = 0.0;
    unsigned long long key = 0;                         // largest (depth, -index); 0 is below the key of every contact pixel's
    unsigned n = 0;
    __device__ inline void add(unsigned xy, float d, float eps, unsigned w)
    {
        if (d != d) d = 0.0f;
        d += 0.0f;                                      // -0 counts as +0
        if (d > eps) {
            const unsigned x = xy & 0xffffu, y = xy >> 16;
            const double dd = (double)d;
            n++;
            S += dd;
            Sx += (double)x * dd;
            Sy += (double)y * dd;
            const unsigned long long k = argmax_key(d, y * w + x);
            key = k > key ? k : key;
        }
    }
};

__global__ __launch_bounds__(TX_NT) void k_taxel_sums(const float *__restrict__ depth, const uint32_t *__restrict__ pixels, const uint32_t *__restrict__ start,
                                                      const TxSlot *__restrict__ slots, const double *__restrict__ mm_per_px,
                                                      const int32_t *__restrict__ status, float eps, unsigned P, unsigned w, int T,
                                                      double *__restrict__ taxels)
{
    __shared__ double ws[TX_NW], wsx[TX_NW], wsy[TX_NW];
    __shared__ unsigned long long wk[TX_NW];
    __shared__ unsigned wn[TX_NW];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const TxSlot sl = slots[blockIdx.x * TX_NW + wid];                  // the table holds gridDim.x * TX_NW slots
    const int t = sl.taxel, part = sl.part & 0xff, parts = sl.part >> 8;
    const bool ok = !status || status[b] == 0;
    TxAcc a;
    unsigned L = 0;
    if (t >= 0) {
        const unsigned beg = start[t], end = start[t + 1], step = 64u * (unsigned)parts;
        L = end - beg;
        if (ok) {
            const float *fr = depth + (size_t)b * P;
            unsigned i = beg + 64u * (unsigned)part + (unsigned)lane;
            for (; i < end && 3u * step < end - i; i += 4u * step) {                 // i + 3 * step < end: four gathers in flight
                const unsigned q0 = pixels[i], q1 = pixels[i + step], q2 = pixels[i + 2u * step], q3 = pixels[i + 3u * step];
                const float d0 = fr[(q0 >> 16) * w + (q0 & 0xffffu)], d1 = fr[(q1 >> 16) * w + (q1 & 0xffffu)];
                const float d2 = fr[(q2 >> 16) * w + (q2 & 0xffffu)], d3 = fr[(q3 >> 16) * w + (q3 & 0xffffu)];
                a.add(q0, d0, eps, w);
                a.add(q1, d1, eps, w);
                a.add(q2, d2, eps, w);
                a.add(q3, d3, eps, w);
            }
            for (; i < end; i += step) {
                const unsigned q = pixels[i];
                a.add(q, fr[(q >> 16) * w + (q & 0xffffu)], eps, w);
            }
        }
    }
    // wave sums on the DPP network, parts in order through LDS
    const double S = wave_sum(a.S), Sx = wave_sum(a.Sx), Sy = wave_sum(a.Sy);
    const unsigned long long key = wave_max_u64(a.key);
    const unsigned n = wave_sum(a.n);
    if (lane == 0) { ws[wid] = S; wsx[wid] = Sx; wsy[wid] = Sy; wk[wid] = key; wn[wid] = n; }
    __syncthreads();
    if (t < 0 || part != 0 || lane != 0) return;
    double *row = taxels + ((size_t)b * T + t) * VISTAF_NTAXEL;
    if (!ok) {
        for (int j = 0; j < VISTAF_NTAXEL; j++) row[j] = nan64();
        return;
    }
    double tS = ws[wid], tSx = wsx[wid], tSy = wsy[wid];
    unsigned long long tk = wk[wid];
    unsigned tn = wn[wid];
    for (int q = 1; q < parts; q++) {                   // parts <= TX_NW - wid: a taxel's slots share a workgroup
        tS += ws[wid + q]; tSx += wsx[wid + q]; tSy += wsy[wid + q];
        tk = wk[wid + q] > tk ? wk[wid + q] : tk;
        tn += wn[wid + q];
    }
    const double s = mm_per_px[b], px = s * s;
    row[VISTAF_TAXEL_CONTACT_PIXELS] = (double)tn;
    row[VISTAF_TAXEL_CONTACT_AREA_MM2] = (double)tn * px;
    row[VISTAF_TAXEL_VOLUME_CM3] = tS * px / 1000.0;
    row[VISTAF_TAXEL_MEAN_DEPTH_MM] = L ? tS / (double)L : nan64();
    row[VISTAF_TAXEL_MAX_DEPTH_MM] = tn ? (double)key2f((uint32_t)(tk >> 32)) : 0.0;
    row[VISTAF_TAXEL_ARGMAX_INDEX] = tn ? (double)(0xffffffffu - (uint32_t)tk) : nan64();
    row[VISTAF_TAXEL_CENTROID_X] = tn ? tSx / tS : nan64();
    row[VISTAF_TAXEL_CENTROID_Y] = tn ? tSy / tS : nan64();
    row[TX_S] = tS;
    row[VISTAF_TAXEL_PRESSURE_KPA] = nan64();
    row[TX_SX] = tSx;
    row[TX_SY] = tSy;
}

// lane j's value in every lane (j uniform)
__device__ inline double tx_lane_value(double v, int j)
{
    const long long u = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, j), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), j);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

__global__ __launch_bounds__(64) void k_taxel_frame(const uint32_t *__restrict__ start, const double *__restrict__ mm_per_px,
                                                    const double *__restrict__ force, const int32_t *__restrict__ status, double ox, double oy,
                                                    int T, double *__restrict__ taxels, double *__restrict__ frame)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    double *rows = taxels + (size_t)b * T * VISTAF_NTAXEL, *fr = frame + (size_t)b * VISTAF_NTAXELFRAME;
    if (status && status[b] != 0) {                     // the rows are NaN already
        if (lane < VISTAF_NTAXELFRAME) fr[lane] = nan64();
        return;
    }
    const double s = mm_per_px[b], px = s * s, F = force ? force[b] : nan64();
    double Sf = 0.0, Sxf = 0.0, Syf = 0.0;
    unsigned active = 0;
    unsigned long long peak = 0;
    for (int base = 0; base < T; base += 64) {
        const int t = base + lane;
        double S = 0.0, Sx = 0.0, Sy = 0.0;
        if (t < T) {
            const double *row = rows + (size_t)t * VISTAF_NTAXEL;
            S = row[TX_S]; Sx = row[TX_SX]; Sy = row[TX_SY];
            if (row[VISTAF_TAXEL_CONTACT_PIXELS] > 0.0) {
                active++;
                const unsigned long long k = argmax_key((float)row[VISTAF_TAXEL_MAX_DEPTH_MM], (unsigned)t);
                peak = k > peak ? k : peak;
            }
        }
#pragma unroll
        for (int j = 0; j < 64; j++) {                  // taxel order; the lanes past T hold +0
            Sf += tx_lane_value(S, j);
            Sxf += tx_lane_value(Sx, j);
            Syf += tx_lane_value(Sy, j);
        }
    }
    for (int t = lane; t < T; t += 64) {
        double *row = rows + (size_t)t * VISTAF_NTAXEL;
        const unsigned L = start[t + 1] - start[t];
        const double share = !force ? nan64() : (Sf == 0.0 ? 0.0 : F * (row[TX_S] / Sf));
        row[VISTAF_TAXEL_FORCE_N] = share;
        row[VISTAF_TAXEL_PRESSURE_KPA] = L ? 1000.0 * share / ((double)L * px) : nan64();
        row[TX_SX] = nan64();
        row[TX_SY] = nan64();
    }
    active = wave_sum(active);
    peak = wave_max_u64(peak);
    if (lane == 0) {
        const double cx = Sf == 0.0 ? nan64() : Sxf / Sf, cy = Sf == 0.0 ? nan64() : Syf / Sf;
        fr[VISTAF_TAXELFRAME_ACTIVE_TAXELS] = (double)active;
        fr[VISTAF_TAXELFRAME_VOLUME_CM3] = Sf * px / 1000.0;
        fr[VISTAF_TAXELFRAME_FORCE_N] = F;
        fr[VISTAF_TAXELFRAME_COP_X] = cx;
        fr[VISTAF_TAXELFRAME_COP_Y] = cy;
        fr[VISTAF_TAXELFRAME_MOMENT_X_NMM] = F * (cy - oy) * s;
        fr[VISTAF_TAXELFRAME_MOMENT_Y_NMM] = -(F * (cx - ox) * s);
        fr[VISTAF_TAXELFRAME_PEAK_TAXEL] = active ? (double)(0xffffffffu - (uint32_t)peak) : nan64();
    }
}

}  // namespace

struct vistaf_taxel_handle {
    int h = 0, w = 0, maxB = 0, T = 0;
    double ox = 0.0, oy = 0.0;
    std::vector<uint32_t> pixels, start;                // host lists: y << 16 | x sorted by (taxel, index); start[T + 1]
    std::vector<TxSlot> slots;                          // a multiple of TX_NW
    std::vector<double> info;                           // [T, 4]
    bool uploaded = false;
    uint32_t *d_pixels = nullptr, *d_start = nullptr;
    TxSlot *d_slots = nullptr;
    DeviceAllocs mem;
};

static int taxel_upload(vistaf_taxel_handle *tx)
{
    if (tx->uploaded) return 0;
    if (tx->mem.alloc(&tx->d_pixels, tx->pixels.size() + 1) || tx->mem.alloc(&tx->d_start, tx->start.size()) ||
        tx->mem.alloc(&tx->d_slots, tx->slots.size())) {
        tx->mem.free_all();
        return VISTAF_E_HIP;
    }
    hipError_t e = hipSuccess;
    if (!tx->pixels.empty()) e = hipMemcpy(tx->d_pixels, tx->pixels.data(), tx->pixels.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(tx->d_start, tx->start.data(), tx->start.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(tx->d_slots, tx->slots.data(), tx->slots.size() * sizeof(TxSlot), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        tx->mem.free_all();
        return set_error(VISTAF_E_HIP, std::string("hipMemcpy: ") + hipGetErrorString(e));
    }
    tx->uploaded = true;
    return 0;
}

extern "C" {

void vistaf_taxel_destroy(vistaf_taxel_handle *tx)
{
    if (!tx) return;
    tx->mem.free_all();
    delete tx;
}

int vistaf_taxel_create(int h, int w, int max_batch, const uint16_t *layout, int n_taxels, double origin_x, double origin_y,
                        vistaf_taxel_handle **out)
{
    if (!out) return set_error(VISTAF_E_INVALID, "null argument");
    *out = nullptr;
    if (!layout) return set_error(VISTAF_E_INVALID, "null argument");
    if (h < 1 || w < 1 || h > 65536 || w > 65536 || (long long)h * w > 0x7fffffffll)
        return set_error(VISTAF_E_INVALID, "frame size must be 1..65536 each way and below 2^31 pixels");
    if (max_batch < 1 || max_batch > 65535) return set_error(VISTAF_E_INVALID, "max_batch must be 1..65535");
    if (n_taxels < 1 || n_taxels > 65535) return set_error(VISTAF_E_INVALID, "n_taxels must be 1..65535");
    if (!std::isfinite(origin_x) || !std::isfinite(origin_y)) return set_error(VISTAF_E_INVALID, "origin must be finite");
    const size_t P = (size_t)h * w;
    const int T = n_taxels;
    std::vector<uint32_t> start((size_t)T + 1, 0u);
    for (size_t p = 0; p < P; p++) {
        const unsigned v = layout[p];
        if (v == VISTAF_TAXEL_NONE) continue;
        if (v >= (unsigned)T) return set_error(VISTAF_E_INVALID, "layout value " + std::to_string(v) + " is neither below n_taxels nor VISTAF_TAXEL_NONE");
        start[v + 1]++;
    }
    for (int t = 0; t < T; t++) start[t + 1] += start[t];
    Created<vistaf_taxel_handle> tx(new vistaf_taxel_handle(), vistaf_taxel_destroy);
    tx->h = h; tx->w = w; tx->maxB = max_batch; tx->T = T; tx->ox = origin_x; tx->oy = origin_y;
    tx->pixels.resize(start[T]);
    // counting sort in row-major order: within a taxel the indices ascend
    std::vector<uint32_t> fill(start.begin(), start.end() - 1);
    std::vector<unsigned long long> sx((size_t)T, 0ull), sy((size_t)T, 0ull);
    size_t p = 0;
    for (unsigned y = 0; y < (unsigned)h; y++)
        for (unsigned x = 0; x < (unsigned)w; x++, p++) {
            const unsigned v = layout[p];
            if (v == VISTAF_TAXEL_NONE) continue;
            tx->pixels[fill[v]++] = (y << 16) | x;
            sx[v] += x;
            sy[v] += y;
        }
    tx->info.resize((size_t)T * 4);
    const double nan = std::nan("");
    for (int t = 0; t < T; t++) {
        const unsigned L = start[t + 1] - start[t];
        tx->info[(size_t)t * 4 + 0] = (double)L;
        tx->info[(size_t)t * 4 + 1] = L ? (double)sx[t] / (double)L : nan;
        tx->info[(size_t)t * 4 + 2] = L ? (double)sy[t] / (double)L : nan;
        tx->info[(size_t)t * 4 + 3] = nan;
        // the taxel's slots: 1, 2, 4 or TX_NW waves of one workgroup
        const unsigned need = (L + TX_WAVE_PIXELS - 1) / TX_WAVE_PIXELS;
        int parts = 1;
        while ((unsigned)parts < need && parts < TX_NW) parts *= 2;
        while (tx->slots.size() % TX_NW + parts > (size_t)TX_NW) tx->slots.push_back(TxSlot{-1, 1 << 8});
        for (int q = 0; q < parts; q++) tx->slots.push_back(TxSlot{t, q | (parts << 8)});
    }
    while (tx->slots.size() % TX_NW) tx->slots.push_back(TxSlot{-1, 1 << 8});
    tx->start = std::move(start);
    *out = tx.release();
    return 0;
}

int vistaf_taxel_layout_info(vistaf_taxel_handle *tx, double *info)
{
    if (!tx || !info) return set_error(VISTAF_E_INVALID, "null argument");
    std::copy(tx->info.begin(), tx->info.end(), info);
    return 0;
}

int vistaf_taxel_measure(vistaf_taxel_handle *tx, const float *d_depth_mm, const double *d_mm_per_px, const double *d_frame_force_N,
                         const int32_t *d_status, float depth_eps_mm, int B, double *d_taxels, double *d_frame, void *stream)
{
    if (!tx || !d_depth_mm || !d_mm_per_px || !d_taxels || !d_frame) return set_error(VISTAF_E_INVALID, "null argument");
    if (B < 1 || B > tx->maxB) return set_error(VISTAF_E_INVALID, "batch must be 1..max_batch");
    if (!std::isfinite(depth_eps_mm)) return set_error(VISTAF_E_INVALID, "depth_eps_mm must be finite");
    if (const int rc = taxel_upload(tx)) return rc;
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_taxel_sums, dim3((unsigned)(tx->slots.size() / TX_NW), (unsigned)B), dim3(TX_NT), 0, st, d_depth_mm, tx->d_pixels, tx->d_start,
                       tx->d_slots, d_mm_per_px, d_status, depth_eps_mm, (unsigned)tx->h * (unsigned)tx->w, (unsigned)tx->w, tx->T, d_taxels);
    hipLaunchKernelGGL(k_taxel_frame, dim3((unsigned)B), dim3(64), 0, st, tx->d_start, d_mm_per_px, d_frame_force_N, d_status, tx->ox, tx->oy, tx->T,
                       d_taxels, d_frame);
    return launch_ok("k_taxel_sums / k_taxel_frame");
}

}  // extern "C"
