// Temporal read-out (include/vistaf_temporal.h): every pixel of a stream of depth planes followed through time -- an exponential filter,
// its rate, a Schmitt-trigger touch bit, the dwell of that bit and the peak raw depth of the running touch -- and per frame the counts,
// extremes and events of the touching pixels.  An extension, as the contacts table, the tracker and the other read-outs: the reference has
// no counterpart.  The definition is in the header; tests/temporal_helpers.py restates it in NumPy.
//
// The recurrence is serial in frames and parallel in pixels, so the frames are a loop inside one kernel and the B * P floats are read once.
//
//   k_temporal_scan<V>  a thread owns V consecutive pixels (V = 4 with 16-byte loads and stores when h * w is a multiple of 4, so that
//                  every frame base is 16-byte aligned; V = 1 otherwise) and keeps their five state values in registers across the
//                  loop over the B frames; a workgroup of TP_NT threads owns a CHUNK of TP_NT * V pixels.  The load addresses do not depend
//                  on the state: the frames go in tiles of TP_FT, and the loads of the next tile are issued before the current one is worked
//                  on.  A skipped frame (status != 0, a wave-uniform branch) is not read -- its load is pointed at the thread's own
//                  filt state, so the loads stay unconditional -- and leaves the state alone.  Per accepted frame a lane gathers its
//                  pixels' five counts (packed into two words), the float64 sum, three ordered 64-bit keys (float bits made monotone,
//                  then ~index, as k_taxel_sums) and the dwell maximum; a wave without a touching or released pixel skips the rest, the
//                  others reduce on the DPP network and leave a record in LDS; after ONE barrier per tile a thread per frame adds the
//                  waves in wave order and writes the (frame, chunk) record.  LDS is double-buffered by tile parity.
//   k_temporal_rows     one wave per frame: lane l adds the records of chunks l, l + 64, ... in ascending order, the wave adds the lanes
//                  on the DPP network, lane 0 writes every field that needs no other frame.
//   k_temporal_events   the only serial dependence, the previous ACCEPTED frame, in one wave, 64 frames a step: a ballot of the accepted
//                  frames gives every lane its predecessor (or the carry), a shuffle its touch pixels and volume: EVENTS, DVOLUME,
//                  GAP_FRAMES, and the stream scalars for the next update.
// Three launches, no memset, no atomics, nothing allocated after the first update.  HAZARD: every workgroup of the scan reads the stream
// scalars (primed, gap), so the scan must never write them -- a late workgroup would see another's update.  Only k_temporal_events, which
// runs after every workgroup of the scan is done, writes them; a reset is a kernel argument (the state is then not read at all), not a memset.
// Sum order: pixel -> lane -> wave -> chunk -> lane of k_temporal_rows, fixed by h * w and the launch geometry, independent of B and of
// how a stream is cut into updates.  Every address is guarded by the handle's own numbers; none comes from device data.
#include <string>

#include "../../include/vistaf_temporal.h"
#include "host_util.hpp"

using namespace vf;

namespace {

constexpr int TP_NW = 4, TP_NT = TP_NW * 64;            // waves and threads of a workgroup of k_temporal_scan
constexpr int TP_FT = 8;                                // frames of a tile: loads in flight per thread, frames per barrier

struct TpStream { double prev_volume, prev_touch; int32_t primed; uint32_t gap; };
// what a chunk (in LDS: a wave) contributes to a frame; identity: all zero
struct alignas(16) TpPart {
    double sum;
    unsigned long long kf, kx, kn;                      // largest (f, ~index), largest (rate, ~index), largest (~rate, ~index)
    uint32_t touch, onset, release, loading, unloading, dwell, pad[2];
};
static_assert(sizeof(TpPart) == 64, "one record is four 16-byte words");
struct TpParams { float alpha, on, off; double period; };
struct TpPlanes { float *filt, *rate, *hold; int32_t *dwell; uint8_t *touch; TpStream *stream; TpPart *parts; };

template <int V>
__device__ inline void tp_load(const float *p, float (&x)[V])
{
    if constexpr (V == 4) {
        const float4 q = *reinterpret_cast<const float4 *>(p);
        x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
    } else {
        x[0] = *p;
    }
}
template <int V>
__device__ inline void tp_store(float *p, const float (&x)[V])
{
    if constexpr (V == 4) *reinterpret_cast<float4 *>(p) = make_float4(x[0], x[1], x[2], x[3]);
    else *p = x[0];
}
template <int V>
__device__ inline void tp_store_bits(uint8_t *p, const uint32_t (&x)[V])
{
    if constexpr (V == 4) *reinterpret_cast<uint32_t *>(p) = x[0] | (x[1] << 8) | (x[2] << 16) | (x[3] << 24);
    else *p = (uint8_t)x[0];
}

__device__ inline void tp_combine(TpPart &a, const TpPart &b)
{
    a.sum += b.sum;
    a.kf = b.kf > a.kf ? b.kf : a.kf;
    a.kx = b.kx > a.kx ? b.kx : a.kx;
    a.kn = b.kn > a.kn ? b.kn : a.kn;
    a.touch += b.touch; a.onset += b.onset; a.release += b.release; a.loading += b.loading; a.unloading += b.unloading;
    a.dwell = b.dwell > a.dwell ? b.dwell : a.dwell;
}

template <int V>
__global__ __launch_bounds__(TP_NT) void k_temporal_scan(const float *__restrict__ depth, const int32_t *__restrict__ status, int B, unsigned P, TpParams prm,
                                                         int reset, TpPlanes st, unsigned nchunks, float *__restrict__ o_filt,
                                                         uint8_t *__restrict__ o_touch)
{
    __shared__ TpPart lds[2][TP_FT][TP_NW];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const unsigned p0 = (blockIdx.x * (unsigned)TP_NT + threadIdx.x) * (unsigned)V;
    const bool valid = p0 < P;                          // V == 4: P is a multiple of 4, the four pixels are inside together
    const unsigned q0 = valid ? p0 : 0u;                // what a thread past the end loads; it counts and stores nothing
    float filt[V], rate[V], hold[V];
    uint32_t touch[V];
    int32_t dwell[V];
#pragma unroll
    for (int j = 0; j < V; j++) { filt[j] = 0.0f; rate[j] = 0.0f; hold[j] = 0.0f; touch[j] = 0u; dwell[j] = 0; }
    int primed = 0;
    uint32_t gap = 0;
    if (!reset) {
        primed = __builtin_amdgcn_readfirstlane(st.stream->primed);         // wave-uniform, and kept so
        gap = (uint32_t)__builtin_amdgcn_readfirstlane((int)st.stream->gap);
        if (valid) {
            tp_load<V>(st.filt + p0, filt);
            tp_load<V>(st.rate + p0, rate);
            tp_load<V>(st.hold + p0, hold);
            if constexpr (V == 4) {
                const uint32_t tb = *reinterpret_cast<const uint32_t *>(st.touch + p0);
                const int4 dw = *reinterpret_cast<const int4 *>(st.dwell + p0);
                touch[0] = tb & 1u; touch[1] = (tb >> 8) & 1u; touch[2] = (tb >> 16) & 1u; touch[3] = (tb >> 24) & 1u;
                dwell[0] = dw.x; dwell[1] = dw.y; dwell[2] = dw.z; dwell[3] = dw.w;
            } else {
                touch[0] = st.touch[p0] & 1u;
                dwell[0] = st.dwell[p0];
            }
        }
    }
    const float *idle = st.filt + q0;                   // where the load of a frame that is not read goes
    float cur[TP_FT][V], nxt[TP_FT][V];
    auto issue = [&](float (&dst)[TP_FT][V], int t0) {
#pragma unroll
        for (int f = 0; f < TP_FT; f++) {
            const int t = t0 + f;
            const bool ok = t < B && (!status || status[t] == 0);
            tp_load<V>(ok ? depth + (size_t)t * P + q0 : idle, dst[f]);
        }
    };
    issue(cur, 0);
    for (int t0 = 0; t0 < B; t0 += TP_FT) {
        const int buf = (t0 / TP_FT) & 1;
        if (t0 + TP_FT < B) issue(nxt, t0 + TP_FT);
#pragma unroll
        for (int f = 0; f < TP_FT; f++) {
            const int t = t0 + f;
            if (t >= B) break;
            if (!status || status[t] == 0) {
                const double den = (double)(gap + 1u) * prm.period;
                uint32_t cA = 0, cB = 0, dmax = 0;      // touch | onset << 10 | release << 20; loading | unloading << 10
                double S = 0.0;
                unsigned long long kf = 0, kx = 0, kn = 0;
#pragma unroll
                for (int j = 0; j < V; j++) {
                    const float x = cur[f][j];
                    const float d = (valid && finitef(x)) ? x : 0.0f;
                    const float fp = primed ? filt[j] : d;
                    const float fl = fp + prm.alpha * (d - fp);
                    const float r = (float)((double)(fl - fp) / den);
                    const uint32_t was = touch[j];
                    const uint32_t now = was ? (fl > prm.off ? 1u : 0u) : (fl >= prm.on ? 1u : 0u);
                    const float base = was ? hold[j] : 0.0f;
                    dwell[j] = now == was ? dwell[j] + 1 : 0;
                    hold[j] = now ? (d > base ? d : base) : 0.0f;
                    filt[j] = fl;
                    rate[j] = r;
                    touch[j] = now;
                    cA += now | ((now & ~was) << 10) | ((was & ~now & 1u) << 20);
                    if (now) {
                        const uint32_t ni = ~(p0 + (unsigned)j);
                        cB += (fl > fp ? 1u : 0u) | ((fl < fp ? 1u : 0u) << 10);
                        S += (double)fl;
                        const unsigned long long a = ((unsigned long long)f2key(fl) << 32) | ni;
                        const unsigned long long b = ((unsigned long long)f2key(r) << 32) | ni;
                        const unsigned long long c = ((unsigned long long)(~f2key(r)) << 32) | ni;
                        kf = a > kf ? a : kf;
                        kx = b > kx ? b : kx;
                        kn = c > kn ? c : kn;
                        dmax = (uint32_t)dwell[j] > dmax ? (uint32_t)dwell[j] : dmax;
                    }
                }
                primed = 1;
                gap = 0;
                TpPart w = {};
                if (__ballot(cA != 0u)) {               // wave-uniform: most waves of a frame see no touching or released pixel
                    const uint32_t A = wave_sum(cA), Bc = wave_sum(cB);
                    w.sum = wave_sum(S);
                    w.kf = wave_max_u64(kf);
                    w.kx = wave_max_u64(kx);
                    w.kn = wave_max_u64(kn);
                    w.dwell = wave_max_u32(dmax);
                    w.touch = A & 1023u; w.onset = (A >> 10) & 1023u; w.release = A >> 20;
                    w.loading = Bc & 1023u; w.unloading = Bc >> 10;
                }
                if (lane == 0) lds[buf][f][wid] = w;
            } else {
                gap++;
            }
            if (valid) {                                // the state after the frame; a skipped frame's planes hold the held state
                if (o_filt) tp_store<V>(o_filt + (size_t)t * P + p0, filt);
                if (o_touch) tp_store_bits<V>(o_touch + (size_t)t * P + p0, touch);
            }
        }
        __syncthreads();
        {
            const int t = t0 + (int)threadIdx.x;
            if (threadIdx.x < TP_FT && t < B && (!status || status[t] == 0)) {
                TpPart a = lds[buf][threadIdx.x][0];
                for (int q = 1; q < TP_NW; q++) tp_combine(a, lds[buf][threadIdx.x][q]);
                st.parts[(size_t)t * nchunks + blockIdx.x] = a;
            }
        }
        if (t0 + TP_FT < B) {
#pragma unroll
            for (int f = 0; f < TP_FT; f++)
#pragma unroll
                for (int j = 0; j < V; j++) cur[f][j] = nxt[f][j];
        }
    }
    if (!valid) return;
    tp_store<V>(st.filt + p0, filt);
    tp_store<V>(st.rate + p0, rate);
    tp_store<V>(st.hold + p0, hold);
    tp_store_bits<V>(st.touch + p0, touch);
    if constexpr (V == 4) *reinterpret_cast<int4 *>(st.dwell + p0) = make_int4(dwell[0], dwell[1], dwell[2], dwell[3]);
    else st.dwell[p0] = dwell[0];
}

__global__ __launch_bounds__(64) void k_temporal_rows(const TpPart *__restrict__ parts, const double *__restrict__ mm_per_px,
                                                      const int32_t *__restrict__ status, unsigned nchunks, double *__restrict__ rows)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    double *row = rows + (size_t)b * VISTAF_NTEMPORAL;
    if (status && status[b] != 0) {                     // GAP_FRAMES is k_temporal_events'
        if (lane < VISTAF_NTEMPORAL) row[lane] = nan64();
        return;
    }
    TpPart a = {};
    for (unsigned c = (unsigned)lane; c < nchunks; c += 64u) tp_combine(a, parts[(size_t)b * nchunks + c]);
    const double S = wave_sum(a.sum);
    const unsigned long long kf = wave_max_u64(a.kf), kx = wave_max_u64(a.kx), kn = wave_max_u64(a.kn);
    const uint32_t n = wave_sum(a.touch), onset = wave_sum(a.onset), release = wave_sum(a.release);
    const uint32_t loading = wave_sum(a.loading), unloading = wave_sum(a.unloading), dw = wave_max_u32(a.dwell);
    if (lane != 0) return;
    const double s = mm_per_px[b];
    row[VISTAF_TEMPORAL_TOUCH_PIXELS] = (double)n;
    row[VISTAF_TEMPORAL_ONSET_PIXELS] = (double)onset;
    row[VISTAF_TEMPORAL_RELEASE_PIXELS] = (double)release;
    row[VISTAF_TEMPORAL_LOADING_PIXELS] = (double)loading;
    row[VISTAF_TEMPORAL_UNLOADING_PIXELS] = (double)unloading;
    row[VISTAF_TEMPORAL_FILTERED_VOLUME_CM3] = n ? S * (s * s) / 1000.0 : 0.0;
    row[VISTAF_TEMPORAL_DVOLUME_CM3_PER_S] = nan64();   // k_temporal_events'; so are EVENTS and GAP_FRAMES
    row[VISTAF_TEMPORAL_MAX_FILTERED_MM] = n ? (double)key2f((uint32_t)(kf >> 32)) : nan64();
    row[VISTAF_TEMPORAL_ARGMAX_INDEX] = n ? (double)(~(uint32_t)kf) : nan64();
    row[VISTAF_TEMPORAL_MAX_RATE_MM_PER_S] = n ? (double)key2f((uint32_t)(kx >> 32)) : nan64();
    row[VISTAF_TEMPORAL_MAX_RATE_INDEX] = n ? (double)(~(uint32_t)kx) : nan64();
    row[VISTAF_TEMPORAL_MIN_RATE_MM_PER_S] = n ? (double)key2f(~(uint32_t)(kn >> 32)) : nan64();
    row[VISTAF_TEMPORAL_MIN_RATE_INDEX] = n ? (double)(~(uint32_t)kn) : nan64();
    row[VISTAF_TEMPORAL_LONGEST_DWELL_FRAMES] = n ? (double)dw : nan64();
}

__global__ __launch_bounds__(64) void k_temporal_events(const int32_t *__restrict__ status, int B, double period, int reset, TpStream *__restrict__ stream,
                                                        double *__restrict__ rows)
{
    const int lane = threadIdx.x;
    double c_touch = 0.0, c_vol = nan64();              // the carry: the last accepted frame so far
    int c_primed = 0;
    uint32_t c_gap = 0;
    if (!reset) { c_touch = stream->prev_touch; c_vol = stream->prev_volume; c_primed = stream->primed; c_gap = stream->gap; }
    for (int t0 = 0; t0 < B; t0 += 64) {
        const int t = t0 + lane;
        const bool in = t < B, ok = in && (!status || status[t] == 0);
        double *row = rows + (size_t)(in ? t : 0) * VISTAF_NTEMPORAL;
        const unsigned long long acc = __ballot(ok), below = acc & ((1ull << lane) - 1ull);
        const int pl = below ? 63 - __clzll((long long)below) : -1;         // the accepted frame before this one, if this step holds it
        const double touch = ok ? row[VISTAF_TEMPORAL_TOUCH_PIXELS] : 0.0, vol = ok ? row[VISTAF_TEMPORAL_FILTERED_VOLUME_CM3] : 0.0;
        double p_touch = __shfl(touch, pl < 0 ? 0 : pl, 64), p_vol = __shfl(vol, pl < 0 ? 0 : pl, 64);      // by every lane: the sources must be active
        int p_primed = 1;
        uint32_t g = (uint32_t)(lane - pl - 1);
        if (pl < 0) { p_touch = c_touch; p_vol = c_vol; p_primed = c_primed; g = c_gap + (uint32_t)lane; }
        if (in) row[VISTAF_TEMPORAL_GAP_FRAMES] = (double)g;
        if (ok) {
            row[VISTAF_TEMPORAL_DVOLUME_CM3_PER_S] = p_primed ? (vol - p_vol) / ((double)(g + 1u) * period) : nan64();
            row[VISTAF_TEMPORAL_EVENTS] = (double)((p_touch == 0.0 && touch > 0.0 ? VISTAF_TEMPEV_TOUCH_BEGAN : 0) |
                                                   (p_touch > 0.0 && touch == 0.0 ? VISTAF_TEMPEV_TOUCH_ENDED : 0));
        }
        const int nin = B - t0 < 64 ? B - t0 : 64;
        if (acc) {
            const int last = 63 - __clzll((long long)acc);
            c_touch = __shfl(touch, last, 64);
            c_vol = __shfl(vol, last, 64);
            c_primed = 1;
            c_gap = (uint32_t)(nin - 1 - last);
        } else {
            c_gap += (uint32_t)nin;
        }
    }
    if (lane == 0) { stream->prev_touch = c_touch; stream->prev_volume = c_vol; stream->primed = c_primed; stream->gap = c_gap; }
}

// the one device buffer of a handle: state planes, stream scalars, partial records; base == nullptr sizes it
TpPlanes temporal_scratch(ScratchLayout &L, size_t P, int maxB, unsigned nchunks)
{
    TpPlanes pl;
    pl.filt = L.take<float>(P, 256, "filt");
    pl.rate = L.take<float>(P, 256, "rate");
    pl.hold = L.take<float>(P, 256, "hold");
    pl.dwell = L.take<int32_t>(P, 256, "dwell");
    pl.touch = L.take<uint8_t>(P, 256, "touch");
    pl.stream = L.take<TpStream>(1, 256, "stream");
    pl.parts = L.take<TpPart>((size_t)maxB * nchunks, 256, "parts");
    return pl;
}

}  // namespace

struct vistaf_temporal_handle {
    int h = 0, w = 0, maxB = 0, V = 1;
    unsigned P = 0, nchunks = 0;
    TpParams prm = {};
    bool reset_pending = true;                          // the state is not read by the next update: it starts from zero
    void *buf = nullptr;
    TpPlanes pl = {};
    DeviceAllocs mem;
};

extern "C" {

void vistaf_temporal_destroy(vistaf_temporal_handle *tp)
{
    if (!tp) return;
    tp->mem.free_all();
    delete tp;
}

int vistaf_temporal_create(int h, int w, int max_batch, double alpha, double on_mm, double off_mm, double frame_period_s,
                           vistaf_temporal_handle **out)
{
    if (!out) return set_error(VISTAF_E_INVALID, "null argument: out");
    *out = nullptr;
    if (h < 1 || w < 1 || h > 65536 || w > 65536 || (long long)h * w > 0x7fffffffll)
        return set_error(VISTAF_E_INVALID, "frame size: h and w must be 1..65536 each and below 2^31 pixels");
    if (max_batch < 1 || max_batch > 65535) return set_error(VISTAF_E_INVALID, "max_batch must be 1..65535");
    const float a = (float)alpha, on = (float)on_mm, off = (float)off_mm;
    if (!std::isfinite(alpha) || !(a > 0.0f) || !(a <= 1.0f)) return set_error(VISTAF_E_INVALID, "alpha must be in (0, 1]");
    if (!std::isfinite(on_mm) || !std::isfinite(on)) return set_error(VISTAF_E_INVALID, "on_mm must be finite");
    if (!std::isfinite(off_mm) || !(off >= 0.0f)) return set_error(VISTAF_E_INVALID, "off_mm must be finite and >= 0");
    if (!(on > off)) return set_error(VISTAF_E_INVALID, "on_mm must be greater than off_mm");
    if (!std::isfinite(frame_period_s) || !(frame_period_s > 0.0)) return set_error(VISTAF_E_INVALID, "frame_period_s must be finite and > 0");
    Created<vistaf_temporal_handle> tp(new vistaf_temporal_handle(), vistaf_temporal_destroy);
    tp->h = h; tp->w = w; tp->maxB = max_batch;
    tp->P = (unsigned)h * (unsigned)w;
    tp->V = tp->P % 4u == 0u ? 4 : 1;
    tp->nchunks = (tp->P + (unsigned)(TP_NT * tp->V) - 1u) / (unsigned)(TP_NT * tp->V);
    tp->prm = TpParams{a, on, off, frame_period_s};
    *out = tp.release();
    return 0;
}

int vistaf_temporal_reset(vistaf_temporal_handle *tp)
{
    if (!tp) return set_error(VISTAF_E_INVALID, "null argument: handle");
    tp->reset_pending = true;
    return 0;
}

int vistaf_temporal_update(vistaf_temporal_handle *tp, const float *d_depth, const double *d_mm_per_px, const int32_t *d_status, int B,
                           double *d_rows, float *d_filtered, uint8_t *d_touch, void *stream)
{
    if (!tp) return set_error(VISTAF_E_INVALID, "null argument: handle");
    if (!d_depth) return set_error(VISTAF_E_INVALID, "null argument: depth");
    if (!d_mm_per_px) return set_error(VISTAF_E_INVALID, "null argument: mm_per_px");
    if (!d_rows) return set_error(VISTAF_E_INVALID, "null argument: rows");
    if (B < 1 || B > tp->maxB) return set_error(VISTAF_E_INVALID, "batch must be 1..max_batch");
    if (tp->V == 4 && ((((uintptr_t)d_depth | (uintptr_t)d_filtered) & 15u) || ((uintptr_t)d_touch & 3u)))
        return set_error(VISTAF_E_INVALID, "h * w is a multiple of 4: depth and filtered must be 16-byte aligned, touch 4-byte aligned");
    TRY(ensure_carved(tp->mem, tp->buf, &tp->pl, [&](ScratchLayout &L) { return temporal_scratch(L, tp->P, tp->maxB, tp->nchunks); }));
    const hipStream_t st = (hipStream_t)stream;
    const int reset = tp->reset_pending ? 1 : 0;
    if (tp->V == 4)
        hipLaunchKernelGGL(k_temporal_scan<4>, dim3(tp->nchunks), dim3(TP_NT), 0, st, d_depth, d_status, B, tp->P, tp->prm, reset, tp->pl, tp->nchunks,
                           d_filtered, d_touch);
    else
        hipLaunchKernelGGL(k_temporal_scan<1>, dim3(tp->nchunks), dim3(TP_NT), 0, st, d_depth, d_status, B, tp->P, tp->prm, reset, tp->pl, tp->nchunks,
                           d_filtered, d_touch);
    hipLaunchKernelGGL(k_temporal_rows, dim3((unsigned)B), dim3(64), 0, st, tp->pl.parts, d_mm_per_px, d_status, tp->nchunks, d_rows);
    hipLaunchKernelGGL(k_temporal_events, dim3(1), dim3(64), 0, st, d_status, B, tp->prm.period, reset, tp->pl.stream, d_rows);
    if (const int rc = launch_ok("k_temporal_scan / k_temporal_rows / k_temporal_events")) return rc;
    tp->reset_pending = false;
    return 0;
}

int vistaf_temporal_state(vistaf_temporal_handle *tp, float *d_filt, float *d_rate, uint8_t *d_touch, int32_t *d_dwell, float *d_hold, void *stream)
{
    if (!tp) return set_error(VISTAF_E_INVALID, "null argument: handle");
    const hipStream_t st = (hipStream_t)stream;
    const size_t P = tp->P;
    const bool zero = tp->reset_pending;                // no update since create or reset: the planes are 0, whatever the buffer holds
    struct { void *dst; const void *src; size_t bytes; } planes[5] = {
        {d_filt, tp->pl.filt, P * sizeof(float)}, {d_rate, tp->pl.rate, P * sizeof(float)}, {d_touch, tp->pl.touch, P},
        {d_dwell, tp->pl.dwell, P * sizeof(int32_t)}, {d_hold, tp->pl.hold, P * sizeof(float)}};
    for (const auto &p : planes) {
        if (!p.dst) continue;
        if (zero) HIPCHK(hipMemsetAsync(p.dst, 0, p.bytes, st));
        else HIPCHK(hipMemcpyAsync(p.dst, p.src, p.bytes, hipMemcpyDeviceToDevice, st));
    }
    return 0;
}

}  // extern "C"
