// Point-cloud read-out (include/vistaf_cloud.h): the surface pixels of a batch of depth planes as metric points with a unit normal, mean and
// Gaussian curvature each, compacted in pixel order, and per frame the areas, the mean normal and the steepest slope.  An extension, as the
// contacts table and the other read-outs: the reference has no counterpart.  The definition is in the header; tests/cloud_helpers.py
// restates it in NumPy.
//
// A deterministic ordered compaction with a 3 x 3 stencil at the survivors:
//
//   k_cloud_count<V>   a workgroup of CL_NT threads owns a CHUNK of CL_NT * V consecutive pixels of one frame (V = 4 with 16-byte loads when
//                  h * w is a multiple of 4, so that every frame base is 16-byte aligned; V = 1 otherwise; nothing else selects a path).
//                  Per wave, V ballots and their popcounts count the points; the four waves meet in LDS; one count per (frame, chunk).
//                  The status is a workgroup-uniform branch: a skipped frame is not read and counts 0.
//   k_cloud_offsets    one workgroup of CL_SCAN threads scans the B * chunks counts, CL_SCAN a round: wave_scan_add in the wave, the wave
//                  totals through LDS (double-buffered by round parity: one barrier a round), a 64-bit carry from round to round; the
//                  next round's counts are loaded before this round's barrier.  A round sums to at most CL_SCAN * CHUNK < 2^32, so only
//                  the carry and the stored bases are 64-bit.  Writes the number of the first point of every chunk, offsets[b] (the base
//                  of a frame's chunk 0) and offsets[B].
//   k_cloud_emit<V>    the geometry of k_cloud_count.  A point's number is the chunk base + the points of the earlier waves (LDS) + those of
//                  the lower lanes (popcounts of the ballots below the lane) + those of the lane's own earlier pixels.  A surface pixel
//                  loads its eight neighbours (points are sparse, the neighbours come out of L1 / L2), evaluates the definition in
//                  float64, and, when it is a point with a number below max_points, writes its record as two 16-byte stores and the side
//                  values.  The frame sums run over ALL surface pixels of the chunk -- the stride and the capacity do not enter -- and
//                  reduce lane -> wave (the DPP tree) -> chunk (wave order, in LDS): one 48-byte record per (frame, chunk).  A wave
//                  without a surface pixel skips stencil and reductions.
//   k_cloud_rows       one wave per frame: lane l adds the records of chunks l, l + 64, ... in ascending order (CL_RU loads in flight a round
//                  of its loop, added in that order), the wave adds the lanes on the
//                  DPP network, lane 0 writes the frame row; POINTS and POINTS_WRITTEN come from the offsets and max_points.
// Four launches, no memset, no atomics, nothing allocated after the first measure.  The steepest slope q is a float64 and is compared as
// one: its bits (q >= 0: the bit pattern is monotone) reduce with wave_max_u64, then ~index among the lanes that hold the maximum -- a
// float32 key would tie slopes that differ and name the wrong pixel.  Every address is guarded by the handle's own numbers and by
// max_points; the only values read from device data that reach an address are the chunk bases, and every store they lead to is guarded.
#include <string>

#include "../../include/vistaf_cloud.h"
#include "host_util.hpp"

using namespace vf;

namespace {

constexpr int CL_NT = VISTAF_CLOUD_CHUNK_THREADS, CL_NW = CL_NT / 64;   // threads and waves of a workgroup of k_cloud_count / k_cloud_emit
constexpr int CL_SCAN = VISTAF_CLOUD_SCAN_THREADS, CL_SW = CL_SCAN / 64;
constexpr int CL_RU = VISTAF_CLOUD_ROW_UNROLL;                         // records a lane of k_cloud_rows has in flight
static_assert(VISTAF_CLOUD_ROW_LANES == 64, "k_cloud_rows is one wave");

// what a chunk (in LDS: a wave) contributes to a frame row; identity: all zero (idx of the identity is never looked at: n == 0)
struct alignas(16) ClPart {
    double srt, snx, sny, snz;
    unsigned long long q;                               // bits of the largest dx * dx + dy * dy
    uint32_t n, nidx;                                   // surface pixels; ~index of the first pixel that attains q
};
static_assert(sizeof(ClPart) == 48, "one record is three 16-byte words");
struct ClGeom { unsigned P, w, h, stride; };
struct ClBufs { uint32_t *counts; long long *bases; ClPart *parts; };

__device__ inline void cl_combine(ClPart &a, const ClPart &b)
{
    a.srt += b.srt; a.snx += b.snx; a.sny += b.sny; a.snz += b.snz;
    if (b.n && (!a.n || b.q > a.q || (b.q == a.q && b.nidx > a.nidx))) { a.q = b.q; a.nidx = b.nidx; }
    a.n += b.n;
}

template <int V>
__device__ inline void cl_load(const float *p, float (&x)[V])
{
    if constexpr (V == 4) {
        const float4 q = *reinterpret_cast<const float4 *>(p);
        x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
    } else {
        x[0] = *p;
    }
}

// the cleaned depths of a thread's V pixels and which of them are surface pixels / points (bit j of the masks)
template <int V>
__device__ inline void cl_classify(const float *__restrict__ frame, unsigned p0, bool valid, const ClGeom &g, float eps, float (&d)[V], uint32_t &surf,
                                   uint32_t &pts)
{
    float x[V];
    cl_load<V>(frame + (valid ? p0 : 0u), x);           // a thread past the end loads pixel 0 and counts nothing
    surf = 0u; pts = 0u;
#pragma unroll
    for (int j = 0; j < V; j++) {
        d[j] = finitef(x[j]) ? x[j] : 0.0f;
        if (valid && d[j] > eps) {
            surf |= 1u << j;
            bool on = true;
            if (g.stride != 1u) {
                const unsigned p = p0 + (unsigned)j, y = p / g.w, xx = p - y * g.w;
                on = xx % g.stride == 0u && y % g.stride == 0u;
            }
            if (on) pts |= 1u << j;
        }
    }
}

template <int V>
__global__ __launch_bounds__(CL_NT) void k_cloud_count(const float *__restrict__ depth, const int32_t *__restrict__ status, ClGeom g, float eps,
                                                       unsigned nchunks, uint32_t *__restrict__ counts)
{
    __shared__ uint32_t wc[CL_NW];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    uint32_t *out = counts + (size_t)b * nchunks + blockIdx.x;
    if (status && status[b] != 0) {                     // uniform in the workgroup
        if (threadIdx.x == 0) *out = 0u;
        return;
    }
    const unsigned p0 = (blockIdx.x * (unsigned)CL_NT + threadIdx.x) * (unsigned)V;
    float d[V];
    uint32_t surf, pts;
    cl_classify<V>(depth + (size_t)b * g.P, p0, p0 < g.P, g, eps, d, surf, pts);
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < V; j++) c += (uint32_t)__popcll(__ballot((pts >> j) & 1u));
    if (lane == 0) wc[wid] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int q = 0; q < CL_NW; q++) t += wc[q];
        *out = t;
    }
}

__global__ __launch_bounds__(CL_SCAN) void k_cloud_offsets(const uint32_t *__restrict__ counts, unsigned N, unsigned nchunks, long long *__restrict__ bases,
                                                           long long *__restrict__ offsets)
{
    __shared__ uint32_t wt[2][CL_SW];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    long long carry = 0;
    int par = 0;
    uint32_t c = threadIdx.x < N ? counts[threadIdx.x] : 0u;
    for (unsigned t0 = 0; t0 < N; t0 += (unsigned)CL_SCAN, par ^= 1) {
        const unsigned i = t0 + threadIdx.x, in = i + (unsigned)CL_SCAN;
        const uint32_t cn = in < N ? counts[in] : 0u;  // the next round's count is in flight over this round
        const uint32_t incl = wave_scan_add(c);
        if (lane == 63) wt[par][wid] = incl;
        __syncthreads();                                // the next round writes the other half: one barrier orders both
        uint32_t before = 0, total = 0;
        for (int q = 0; q < CL_SW; q++) {
            const uint32_t v = wt[par][q];
            before += q < wid ? v : 0u;
            total += v;
        }
        if (i < N) {
            const long long base = carry + (long long)(before + (incl - c));
            bases[i] = base;
            if (i % nchunks == 0u) offsets[i / nchunks] = base;
        }
        carry += (long long)total;
        c = cn;
    }
    if (threadIdx.x == 0) offsets[N / nchunks] = carry;
}

__device__ inline double cl_at(const float *__restrict__ frame, unsigned w, unsigned x, unsigned y)
{
    const float v = frame[(size_t)y * w + x];
    return (double)(finitef(v) ? v : 0.0f);
}

template <int V>
__global__ __launch_bounds__(CL_NT) void k_cloud_emit(const float *__restrict__ depth, const double *__restrict__ mm_per_px, const int32_t *__restrict__ status,
                                                      const int8_t *__restrict__ cindex, ClGeom g, float eps, double ox, double oy, unsigned nchunks,
                                                      const long long *__restrict__ bases, long long max_points, float *__restrict__ points,
                                                      int32_t *__restrict__ pixel, int8_t *__restrict__ label, ClPart *__restrict__ parts)
{
    __shared__ uint32_t wc[CL_NW];
    __shared__ ClPart wp[CL_NW];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (status && status[b] != 0) return;               // uniform in the workgroup; k_cloud_rows does not read a skipped frame's records
    const float *frame = depth + (size_t)b * g.P;
    const long long base = bases[(size_t)b * nchunks + blockIdx.x];   // asked for first: it is not needed before the barrier
    const unsigned p0 = (blockIdx.x * (unsigned)CL_NT + threadIdx.x) * (unsigned)V;
    float d[V];
    uint32_t surf, pts;
    cl_classify<V>(frame, p0, p0 < g.P, g, eps, d, surf, pts);
    uint32_t below = 0, wave_pts = 0;                   // points of the lower lanes; of the wave
    const unsigned long long lt = (1ull << lane) - 1ull;
#pragma unroll
    for (int j = 0; j < V; j++) {
        const unsigned long long m = __ballot((pts >> j) & 1u);
        below += (uint32_t)__popcll(m & lt);
        wave_pts += (uint32_t)__popcll(m);
    }
    if (lane == 0) wc[wid] = wave_pts;
    __syncthreads();
    uint32_t prior = 0;
    for (int q = 0; q < CL_NW; q++) prior += q < wid ? wc[q] : 0u;
    long long rank = base + (long long)(prior + below);

    ClPart a = {};
    if (__ballot(surf != 0u)) {                         // wave-uniform: most waves of a frame see no surface pixel
        const double s = mm_per_px[b];
        const double s2 = 2.0 * s, ss = s * s, ss4 = 4.0 * ss;
        double q = 0.0;
        uint32_t qn = 0;
#pragma unroll
        for (int j = 0; j < V; j++) {
            if (!((surf >> j) & 1u)) continue;
            const unsigned p = p0 + (unsigned)j, y = p / g.w, x = p - y * g.w;
            const unsigned xl = x ? x - 1u : 0u, xr = x + 1u < g.w ? x + 1u : x, yu = y ? y - 1u : 0u, yd = y + 1u < g.h ? y + 1u : y;
            const double c = (double)d[j];
            const double l = cl_at(frame, g.w, xl, y), r = cl_at(frame, g.w, xr, y), u = cl_at(frame, g.w, x, yu), dn = cl_at(frame, g.w, x, yd);
            const double ul = cl_at(frame, g.w, xl, yu), ur = cl_at(frame, g.w, xr, yu), bl = cl_at(frame, g.w, xl, yd), br = cl_at(frame, g.w, xr, yd);
            const double dx = (r - l) / s2, dy = (dn - u) / s2;
            const double dxx = ((r - c) - (c - l)) / ss, dyy = ((dn - c) - (c - u)) / ss;
            const double dxy = ((br - bl) - (ur - ul)) / ss4;
            const double ax = 1.0 + dx * dx, ay = 1.0 + dy * dy;
            const double gg = ax + dy * dy, rt = sqrt(gg);
            const double nx = dx / rt, ny = dy / rt, nz = 1.0 / rt;
            const double Hc = ((ay * dxx - (2.0 * (dx * dy)) * dxy) + ax * dyy) / (2.0 * (gg * rt));
            const double Kc = (dxx * dyy - dxy * dxy) / (gg * gg);
            const double qq = dx * dx + dy * dy;
            a.srt += rt; a.snx += nx; a.sny += ny; a.snz += nz;
            if (!a.n || qq > q) { q = qq; qn = ~p; }    // ascending pixels: the first one that attains it stays
            a.n++;
            if ((pts >> j) & 1u) {
                if (rank < max_points) {
                    float4 *rec = reinterpret_cast<float4 *>(points + (size_t)rank * VISTAF_NCLOUD_POINT);
                    rec[0] = make_float4((float)(((double)x - ox) * s), (float)(((double)y - oy) * s), (float)(-c), (float)nx);
                    rec[1] = make_float4((float)ny, (float)nz, (float)Hc, (float)Kc);
                    pixel[rank] = (int32_t)p;
                    if (label && cindex) label[rank] = cindex[(size_t)b * g.P + p];
                }
                rank++;
            }
        }
        const uint32_t n = wave_sum(a.n);
        const unsigned long long qb = a.n ? (unsigned long long)__double_as_longlong(q) : 0ull;
        const unsigned long long qmax = wave_max_u64(qb);
        const uint32_t nidx = wave_max_u32(a.n && qb == qmax ? qn : 0u);
        a.srt = wave_sum(a.srt); a.snx = wave_sum(a.snx); a.sny = wave_sum(a.sny); a.snz = wave_sum(a.snz);
        a.n = n; a.q = qmax; a.nidx = nidx;
    }
    if (lane == 0) wp[wid] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        ClPart t = wp[0];
        for (int q = 1; q < CL_NW; q++) cl_combine(t, wp[q]);
        parts[(size_t)b * nchunks + blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(64) void k_cloud_rows(const ClPart *__restrict__ parts, const double *__restrict__ mm_per_px, const int32_t *__restrict__ status,
                                                   unsigned nchunks, const long long *__restrict__ offsets, long long max_points, double *__restrict__ rows)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    double *row = rows + (size_t)b * VISTAF_NCLOUD_FRAME;
    if (status && status[b] != 0) {
        if (lane < VISTAF_NCLOUD_FRAME) row[lane] = nan64();
        return;
    }
    ClPart a = {};
    for (unsigned c0 = (unsigned)lane; c0 < nchunks; c0 += 64u * (unsigned)CL_RU) {    // CL_RU records in flight, added in ascending order
        ClPart r[CL_RU];
#pragma unroll
        for (int k = 0; k < CL_RU; k++) {
            const unsigned c = c0 + 64u * (unsigned)k;
            r[k] = parts[(size_t)b * nchunks + (c < nchunks ? c : c0)];
        }
#pragma unroll
        for (int k = 0; k < CL_RU; k++)
            if (c0 + 64u * (unsigned)k < nchunks) cl_combine(a, r[k]);
    }
    const uint32_t n = wave_sum(a.n);
    const unsigned long long qmax = wave_max_u64(a.n ? a.q : 0ull);
    const uint32_t nidx = wave_max_u32(a.n && a.q == qmax ? a.nidx : 0u);
    const double srt = wave_sum(a.srt), sx = wave_sum(a.snx), sy = wave_sum(a.sny), sz = wave_sum(a.snz);
    if (lane != 0) return;
    const double s = mm_per_px[b], ss = s * s;
    const long long o0 = offsets[b], o1 = offsets[b + 1];
    const long long w0 = o0 < max_points ? o0 : max_points, w1 = o1 < max_points ? o1 : max_points;
    row[VISTAF_CLOUDFRAME_SURFACE_PIXELS] = (double)n;
    row[VISTAF_CLOUDFRAME_POINTS] = (double)(o1 - o0);
    row[VISTAF_CLOUDFRAME_POINTS_WRITTEN] = (double)(w1 - w0);
    row[VISTAF_CLOUDFRAME_PROJECTED_AREA_MM2] = n ? (double)n * ss : 0.0;
    row[VISTAF_CLOUDFRAME_SURFACE_AREA_MM2] = n ? srt * ss : 0.0;
    row[VISTAF_CLOUDFRAME_RESERVED] = nan64();
    if (!n) {
        for (int i = VISTAF_CLOUDFRAME_MEAN_NORMAL_X; i <= VISTAF_CLOUDFRAME_MAX_SLOPE_INDEX; i++) row[i] = nan64();
        return;
    }
    const double len = sqrt((sx * sx + sy * sy) + sz * sz);
    const double mx = sx / len, my = sy / len, mz = sz / len;
    const double deg = 180.0 / 3.14159265358979323846;
    row[VISTAF_CLOUDFRAME_MEAN_NORMAL_X] = mx;
    row[VISTAF_CLOUDFRAME_MEAN_NORMAL_Y] = my;
    row[VISTAF_CLOUDFRAME_MEAN_NORMAL_Z] = mz;
    row[VISTAF_CLOUDFRAME_TILT_DEG] = atan2(hypot(mx, my), mz) * deg;
    row[VISTAF_CLOUDFRAME_MAX_SLOPE_DEG] = atan(sqrt(__longlong_as_double((long long)qmax))) * deg;
    row[VISTAF_CLOUDFRAME_MAX_SLOPE_INDEX] = (double)(~nidx);
}

// the one device buffer of a handle: the counts and bases of max_batch * chunks chunks and their partial records; base == nullptr sizes it
ClBufs cloud_scratch(ScratchLayout &L, int maxB, unsigned nchunks)
{
    ClBufs bf;
    const size_t N = (size_t)maxB * nchunks;
    bf.counts = L.take<uint32_t>(N, 256, "counts");
    bf.bases = L.take<long long>(N, 256, "bases");
    bf.parts = L.take<ClPart>(N, 256, "parts");
    return bf;
}

}  // namespace

struct vistaf_cloud_handle {
    int maxB = 0, V = 1;
    ClGeom g = {};
    unsigned nchunks = 0;
    long long max_points = 0;
    double ox = 0.0, oy = 0.0;
    void *buf = nullptr;
    ClBufs bf = {};
    DeviceAllocs mem;
};

extern "C" {

void vistaf_cloud_destroy(vistaf_cloud_handle *cl)
{
    if (!cl) return;
    cl->mem.free_all();
    delete cl;
}

int vistaf_cloud_create(int h, int w, int max_batch, int64_t max_points, int stride, double origin_x, double origin_y, vistaf_cloud_handle **out)
{
    if (!out) return set_error(VISTAF_E_INVALID, "null argument: out");
    *out = nullptr;
    if (h < 1 || w < 1 || h > 65536 || w > 65536 || (long long)h * w > 0x7fffffffll)
        return set_error(VISTAF_E_INVALID, "frame size: h and w must be 1..65536 each and below 2^31 pixels");
    if (max_batch < 1 || max_batch > 65535) return set_error(VISTAF_E_INVALID, "max_batch must be 1..65535");
    if (max_points < 1) return set_error(VISTAF_E_INVALID, "max_points must be >= 1");
    if (stride < 1 || stride > 64) return set_error(VISTAF_E_INVALID, "stride must be 1..64");
    if (!std::isfinite(origin_x)) return set_error(VISTAF_E_INVALID, "origin_x must be finite");
    if (!std::isfinite(origin_y)) return set_error(VISTAF_E_INVALID, "origin_y must be finite");
    Created<vistaf_cloud_handle> cl(new vistaf_cloud_handle(), vistaf_cloud_destroy);
    cl->maxB = max_batch;
    cl->g = ClGeom{(unsigned)h * (unsigned)w, (unsigned)w, (unsigned)h, (unsigned)stride};
    cl->V = cl->g.P % 4u == 0u ? 4 : 1;
    cl->nchunks = (cl->g.P + (unsigned)(CL_NT * cl->V) - 1u) / (unsigned)(CL_NT * cl->V);
    if ((unsigned long long)max_batch * cl->nchunks > 0x7fffffffull)                     // the scan indexes the counts with 32 bits
        return set_error(VISTAF_E_INVALID, "max_batch times the chunks of a frame must be below 2^31");
    cl->max_points = (long long)max_points;
    cl->ox = origin_x; cl->oy = origin_y;
    *out = cl.release();
    return 0;
}

int vistaf_cloud_measure(vistaf_cloud_handle *cl, const float *d_depth_mm, const double *d_mm_per_px, const int32_t *d_status,
                         const int8_t *d_contact_index, float depth_eps_mm, int B, float *d_points, int32_t *d_pixel, int8_t *d_label,
                         int64_t *d_offsets, double *d_frame, void *stream)
{
    if (!cl) return set_error(VISTAF_E_INVALID, "null argument: handle");
    if (!d_depth_mm) return set_error(VISTAF_E_INVALID, "null argument: depth_mm");
    if (!d_mm_per_px) return set_error(VISTAF_E_INVALID, "null argument: mm_per_px");
    if (!d_points) return set_error(VISTAF_E_INVALID, "null argument: points");
    if (!d_pixel) return set_error(VISTAF_E_INVALID, "null argument: pixel");
    if (!d_offsets) return set_error(VISTAF_E_INVALID, "null argument: offsets");
    if (!d_frame) return set_error(VISTAF_E_INVALID, "null argument: frame");
    if (B < 1 || B > cl->maxB) return set_error(VISTAF_E_INVALID, "batch must be 1..max_batch");
    if ((uintptr_t)d_points & 15u) return set_error(VISTAF_E_INVALID, "points must be 16-byte aligned");
    if (((uintptr_t)d_pixel & 3u) || ((uintptr_t)d_offsets & 7u) || ((uintptr_t)d_frame & 7u))
        return set_error(VISTAF_E_INVALID, "pixel must be 4-byte aligned, offsets and frame 8-byte aligned");
    if (cl->V == 4 && ((uintptr_t)d_depth_mm & 15u)) return set_error(VISTAF_E_INVALID, "h * w is a multiple of 4: depth_mm must be 16-byte aligned");
    TRY(ensure_carved(cl->mem, cl->buf, &cl->bf, [&](ScratchLayout &L) { return cloud_scratch(L, cl->maxB, cl->nchunks); }));
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid(cl->nchunks, (unsigned)B);
    const unsigned N = (unsigned)B * cl->nchunks;
    long long *offsets = reinterpret_cast<long long *>(d_offsets);
    if (cl->V == 4) hipLaunchKernelGGL(k_cloud_count<4>, grid, dim3(CL_NT), 0, st, d_depth_mm, d_status, cl->g, depth_eps_mm, cl->nchunks, cl->bf.counts);
    else hipLaunchKernelGGL(k_cloud_count<1>, grid, dim3(CL_NT), 0, st, d_depth_mm, d_status, cl->g, depth_eps_mm, cl->nchunks, cl->bf.counts);
    hipLaunchKernelGGL(k_cloud_offsets, dim3(1), dim3(CL_SCAN), 0, st, cl->bf.counts, N, cl->nchunks, cl->bf.bases, offsets);
    if (cl->V == 4)
        hipLaunchKernelGGL(k_cloud_emit<4>, grid, dim3(CL_NT), 0, st, d_depth_mm, d_mm_per_px, d_status, d_contact_index, cl->g, depth_eps_mm, cl->ox, cl->oy,
                           cl->nchunks, cl->bf.bases, cl->max_points, d_points, d_pixel, d_label, cl->bf.parts);
    else
        hipLaunchKernelGGL(k_cloud_emit<1>, grid, dim3(CL_NT), 0, st, d_depth_mm, d_mm_per_px, d_status, d_contact_index, cl->g, depth_eps_mm, cl->ox, cl->oy,
                           cl->nchunks, cl->bf.bases, cl->max_points, d_points, d_pixel, d_label, cl->bf.parts);
    hipLaunchKernelGGL(k_cloud_rows, dim3((unsigned)B), dim3(64), 0, st, cl->bf.parts, d_mm_per_px, d_status, cl->nchunks, offsets, cl->max_points, d_frame);
    return launch_ok("k_cloud_count / k_cloud_offsets / k_cloud_emit / k_cloud_rows");
}

}  // extern "C"
