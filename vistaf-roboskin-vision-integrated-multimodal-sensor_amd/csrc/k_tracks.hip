// Contact tracker (include/vistaf_track.h): links the rows of the per-contact tables of consecutive frames, from the int8 index planes and
// the tables vistaf_ftp_contacts writes.  An extension, as that table: the reference has no counterpart.  The definition of the link is in
// the header; tests/tracks_helpers.py restates it in NumPy.
//
//   k_tr_overlap  ONE pass over the two index planes of every frame pair (pair 0 reads the plane the tracker carried over).  Both planes
//                 are -1 over almost every pixel: a lane takes 16 pixels of the current plane with one aligned 16-byte load, fetches the
//                 same 16 pixels of the previous plane only when one of its own is a contact pixel, and a wave goes on after one ballot
//                 when no lane holds a pair.  Pairs are counted into a K x K uint32 histogram in LDS with integer atomics, runs of equal
//                 pairs inside a lane's 16 pixels with one add.  The frame bases are not 16-byte aligned when h*w is no multiple of 16: the
//                 vectors are aligned on the current plane, the (at most 15 + 15) pixels before and after them go one by one, and the
//                 previous plane is read with an unaligned 16-byte load.  Two tiers, the ones of launch_contacts: one 1024-thread workgroup
//                 per frame, or 256-thread workgroups over TR_CHUNK pixels that add their histograms up with integer global atomics.
//   k_tr_link     one wave per frame pair, lane = row: best_next / best_prev from the histogram (staged in LDS, padded rows), the overlap
//                 links, the gate stage (every lane keeps its nearest remaining candidate; a wave-wide lexicographic minimum picks the
//                 pair), events, fate, and every field of the output rows that needs no id.
//   k_tr_ids      the only serial dependence, frame after frame, in one wave: the link rows of a tile of frames are staged in LDS, so a
//                 frame costs a few LDS / cross-lane operations and no global round trip; births take their ids from a ballot prefix.  It
//                 writes TRACK_ID / AGE_FRAMES / ORIGIN_TRACK_ID and leaves the last frame's rows, ids, ages and next_id as the carry.
// No float atomics and no float sums: every number is an integer or the result of one float64 operation, so two updates from the same
// state give the same bits.
#include <string>

#include "../../include/vistaf_track.h"
#include "host_util.hpp"

using namespace vf;

namespace {

constexpr int TR_MAXK = VISTAF_MAX_CONTACTS, TR_CHUNK = 8192, TR_LDS_ROW = TR_MAXK + 1, TR_TILE = 64;
constexpr int TR_PARENT_BORN = -1, TR_PARENT_UNUSED = -2;
static_assert(TR_MAXK == 64, "lane = row: one wave covers a table");

// what the tracker carries from the last frame of an update to the first of the next (device memory)
struct TrackState {
    long long next_id;
    int m, pad;                                  // rows of the carried frame
    long long ids[TR_MAXK], ages[TR_MAXK];
    double rows[TR_MAXK * VISTAF_NCONTACT];      // its contacts table
};

__device__ inline double tr_sub(double a, double b) { const double d = a - b; return d != d ? nan64() : d; }      // one subtraction; one NaN
__device__ inline unsigned int tr_nonneg(uint4 v) { return (~v.x | ~v.y | ~v.z | ~v.w) & 0x80808080u; }           // some byte >= 0

template <int NT>
__global__ __launch_bounds__(NT) void k_tr_overlap(const int8_t *__restrict__ index, const int8_t *__restrict__ carry, int K, int P, int chunk_vec,
                                                   unsigned int *__restrict__ ovl)
{
    __shared__ unsigned int hist[TR_MAXK * TR_MAXK];
    const size_t t = blockIdx.y;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int8_t *cur = index + t * (size_t)P;
    const int8_t *prev = t ? cur - P : carry;
    const int KK = K * K;
    for (int i = threadIdx.x; i < KK; i += NT) hist[i] = 0;
    __syncthreads();
    int head = (int)((16 - ((uintptr_t)cur & 15)) & 15);          // pixels before the first 16-byte boundary of the current plane
    if (head > P) head = P;
    const int nvec = (P - head) >> 4, tail0 = head + (nvec << 4);
    if (blockIdx.x == 0 && (int)threadIdx.x < head + (P - tail0)) {            // at most 15 + 15 pixels, one by one
        const int p = (int)threadIdx.x < head ? (int)threadIdx.x : tail0 + ((int)threadIdx.x - head);
        const int i = prev[p], j = cur[p];
        if ((unsigned int)i < (unsigned int)K && (unsigned int)j < (unsigned int)K) atomicAdd(&hist[i * K + j], 1u);
    }
    const int v_begin = blockIdx.x * chunk_vec, v_end = v_begin + chunk_vec < nvec ? v_begin + chunk_vec : nvec;
    for (int v0 = v_begin + wid * 64; v0 < v_end; v0 += NT) {
        const int v = v0 + lane;
        uint4 c = make_uint4(~0u, ~0u, ~0u, ~0u), q = c;
        if (v < v_end) {
            const size_t o = (size_t)head + ((size_t)v << 4);
            c = *reinterpret_cast<const uint4 *>(cur + o);
            if (tr_nonneg(c)) __builtin_memcpy(&q, prev + o, 16);               // not aligned: the planes' bases differ by P bytes
        }
        const unsigned int cw[4] = {c.x, c.y, c.z, c.w}, qw[4] = {q.x, q.y, q.z, q.w};
        const bool has = ((~cw[0] & ~qw[0]) | (~cw[1] & ~qw[1]) | (~cw[2] & ~qw[2]) | (~cw[3] & ~qw[3])) & 0x80808080u;
        if (!__ballot(has)) continue;
        if (!has) continue;
        int key = -1;
        unsigned int run = 0;
#pragma unroll
        for (int d = 0; d < 4; d++) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int i = (int)(int8_t)(qw[d] >> (8 * k)), j = (int)(int8_t)(cw[d] >> (8 * k));
                const int e = ((unsigned int)i < (unsigned int)K && (unsigned int)j < (unsigned int)K) ? i * K + j : -1;
                if (e != key) {
                    if (key >= 0) atomicAdd(&hist[key], run);
                    key = e;
                    run = 0;
                }
                run++;
            }
        }
        if (key >= 0) atomicAdd(&hist[key], run);
    }
    __syncthreads();
    unsigned int *o = ovl + t * (size_t)KK;
    if (gridDim.x == 1) {
        for (int i = threadIdx.x; i < KK; i += NT) o[i] = hist[i];
    } else {
        for (int i = threadIdx.x; i < KK; i += NT)
            if (hist[i]) atomicAdd(&o[i], hist[i]);                            // `ovl` was zeroed by the launcher
    }
}

__global__ __launch_bounds__(64) void k_tr_link(const unsigned int *__restrict__ ovl, const double *__restrict__ contacts, const int32_t *__restrict__ count,
                                                const TrackState *__restrict__ state, int K, int gate_on, double gate2, double *__restrict__ tracks,
                                                int32_t *__restrict__ fate, int32_t *__restrict__ linkrow)
{
    __shared__ unsigned int O[TR_MAXK * TR_LDS_ROW];
    __shared__ double pcx[TR_MAXK], pcy[TR_MAXK];
    __shared__ int merged[TR_MAXK];
    const size_t t = blockIdx.x;
    const int lane = threadIdx.x;
    const double *crow = contacts + t * (size_t)K * VISTAF_NCONTACT;
    const double *prow = t ? crow - (size_t)K * VISTAF_NCONTACT : state->rows;
    int m = t ? count[t - 1] : state->m, n = count[t];
    m = m < 0 ? 0 : (m > K ? K : m);
    n = n < 0 ? 0 : (n > K ? K : n);
    for (int e = lane; e < K * K; e += 64) O[(e / K) * TR_LDS_ROW + e % K] = ovl[t * (size_t)K * K + e];
    merged[lane] = 0;
    const double px = lane < m ? prow[lane * VISTAF_NCONTACT + VISTAF_CONTACT_CENTROID_X] : nan64();
    const double py = lane < m ? prow[lane * VISTAF_NCONTACT + VISTAF_CONTACT_CENTROID_Y] : nan64();
    const double cx = lane < n ? crow[lane * VISTAF_NCONTACT + VISTAF_CONTACT_CENTROID_X] : nan64();
    const double cy = lane < n ? crow[lane * VISTAF_NCONTACT + VISTAF_CONTACT_CENTROID_Y] : nan64();
    pcx[lane] = px;
    pcy[lane] = py;
    __syncthreads();
    // step 2: strict '>' in ascending order keeps the lowest index among equal overlaps
    int bn = -1, bp = -1;
    unsigned int on = 0, op = 0;
    if (lane < m)
        for (int j = 0; j < n; j++) { const unsigned int o = O[lane * TR_LDS_ROW + j]; if (o > on) { on = o; bn = j; } }
    if (lane < n)
        for (int i = 0; i < m; i++) { const unsigned int o = O[i * TR_LDS_ROW + lane]; if (o > op) { op = o; bp = i; } }
    // step 3
    const int bn_of_bp = __shfl(bn, bp < 0 ? 0 : bp, 64), bp_of_bn = __shfl(bp, bn < 0 ? 0 : bn, 64);      // by every lane: the sources must be active
    const bool linked_j = bp >= 0 && bn_of_bp == lane;
    const bool linked_i = bn >= 0 && bp_of_bn == lane;
    int parent = linked_j ? bp : TR_PARENT_BORN;
    const unsigned int overlap = linked_j ? op : 0u;
    int fate_i = lane < m ? (linked_i ? bn : (bn >= 0 ? VISTAF_FATE_ABSORBED(bn) : VISTAF_FATE_ENDED)) : VISTAF_FATE_NO_ROW;
    if (bn >= 0 && !linked_i) merged[bn] = 1;
    // step 4
    bool gated = false;
    if (gate_on) {
        bool cand_j = lane < n && bp < 0 && finitef(cx) && finitef(cy);
        unsigned long long imask = __ballot(lane < m && bn < 0 && finitef(px) && finitef(py));
        unsigned long long best_d = ~0ull;
        int best_i = -1;
        bool stale = true;
        for (;;) {
            if (cand_j && stale) {              // nearest remaining candidate of this row; ascending i and '<' keep the lowest i
                best_d = ~0ull;
                best_i = -1;
                for (unsigned long long r = imask; r; r &= r - 1) {
                    const int i = __ffsll((long long)r) - 1;
                    const double dx = cx - pcx[i], dy = cy - pcy[i];
                    const double d2 = dx * dx + dy * dy;
                    const unsigned long long bits = (unsigned long long)__double_as_longlong(d2);       // d2 >= 0: the bits order as the values
                    if (d2 <= gate2 && bits < best_d) { best_d = bits; best_i = i; }
                }
            }
            stale = false;
            const bool have = cand_j && best_i >= 0;
            const unsigned long long dmin = wave_min_u64(have ? best_d : ~0ull);
            if (dmin == ~0ull) break;
            const unsigned int ij = (unsigned int)wave_min_u64((have && best_d == dmin) ? (unsigned long long)(best_i * 64 + lane) : ~0ull);
            const int wi = (int)(ij >> 6), wj = (int)(ij & 63u);
            if (lane == wj) { parent = wi; gated = true; cand_j = false; }
            if (lane == wi) fate_i = wj;
            imask &= ~(1ull << wi);
            if (cand_j && best_i == wi) stale = true;
        }
    }
    __syncthreads();
    const bool split = parent < 0 && bp >= 0;
    // all 64 lanes: k_tr_ids reads a whole row of `linkrow` whatever K is, and a row it took for a birth would use up an id
    linkrow[t * TR_MAXK + lane] = lane < n ? ((parent & 0xff) | (((split ? bp : -1) & 0xff) << 8)) : (TR_PARENT_UNUSED & 0xff);
    if (lane >= K) return;
    fate[t * (size_t)K + lane] = fate_i;
    double *o = tracks + (t * (size_t)K + lane) * VISTAF_NTRACK;
    if (lane >= n) {
        for (int f = 0; f < VISTAF_NTRACK; f++) o[f] = nan64();
        return;
    }
    // VISTAF_TRACK_ID, _AGE_FRAMES and _ORIGIN_TRACK_ID of a used row are k_tr_ids'
    const int ev = (parent < 0 ? VISTAF_TRACKEV_BORN : 0) | (split ? VISTAF_TRACKEV_SPLIT : 0) | (merged[lane] ? VISTAF_TRACKEV_MERGED : 0) |
                   (gated ? VISTAF_TRACKEV_GATED : 0);
    o[VISTAF_TRACK_PARENT_ROW] = (double)parent;
    o[VISTAF_TRACK_EVENTS] = (double)ev;
    o[VISTAF_TRACK_OVERLAP_PX] = (double)overlap;
    const double *me = crow + lane * VISTAF_NCONTACT, *pa = prow + (parent < 0 ? 0 : parent) * VISTAF_NCONTACT;
    o[VISTAF_TRACK_DX] = parent < 0 ? nan64() : tr_sub(cx, pcx[parent]);
    o[VISTAF_TRACK_DY] = parent < 0 ? nan64() : tr_sub(cy, pcy[parent]);
    o[VISTAF_TRACK_DFORCE_N] = parent < 0 ? nan64() : tr_sub(me[VISTAF_CONTACT_FORCE_N], pa[VISTAF_CONTACT_FORCE_N]);
    o[VISTAF_TRACK_DVOLUME_CM3] = parent < 0 ? nan64() : tr_sub(me[VISTAF_CONTACT_VOLUME_CM3], pa[VISTAF_CONTACT_VOLUME_CM3]);
    for (int f = VISTAF_TRACK_ORIGIN_TRACK_ID + 1; f < VISTAF_NTRACK; f++) o[f] = nan64();
}

__global__ __launch_bounds__(64) void k_tr_ids(const int32_t *__restrict__ linkrow, const double *__restrict__ contacts, int B, int K,
                                               TrackState *__restrict__ state, double *__restrict__ tracks)
{
    __shared__ int32_t tile[TR_TILE * TR_MAXK];
    const int lane = threadIdx.x;
    long long id = state->ids[lane], age = state->ages[lane], next = state->next_id;
    int m = state->m;
    for (int t0 = 0; t0 < B; t0 += TR_TILE) {
        const int nt = B - t0 < TR_TILE ? B - t0 : TR_TILE;
        __syncthreads();
        for (int e = lane; e < nt * TR_MAXK; e += 64) tile[e] = linkrow[(size_t)t0 * TR_MAXK + e];
        __syncthreads();
        for (int f = 0; f < nt; f++) {
            const int w = tile[f * TR_MAXK + lane];
            const int parent = (int)(int8_t)(w & 0xff), origin = (int)(int8_t)((w >> 8) & 0xff);
            const bool used = parent != TR_PARENT_UNUSED, born = parent == TR_PARENT_BORN;
            const long long pid = __shfl(id, parent < 0 ? 0 : parent, 64), page = __shfl(age, parent < 0 ? 0 : parent, 64);
            const long long oid = __shfl(id, origin < 0 ? 0 : origin, 64);
            const unsigned long long births = __ballot(born);
            const long long nid = born ? next + __popcll(births & ((1ull << lane) - 1ull)) : pid;      // births in ascending row order
            const long long nage = born ? 0 : page + 1;
            next += __popcll(births);
            if (used && lane < K) {
                double *o = tracks + ((size_t)(t0 + f) * K + lane) * VISTAF_NTRACK;
                o[VISTAF_TRACK_ID] = (double)nid;
                o[VISTAF_TRACK_AGE_FRAMES] = (double)nage;
                o[VISTAF_TRACK_ORIGIN_TRACK_ID] = origin < 0 ? -1.0 : (double)oid;
            }
            id = used ? nid : 0;
            age = used ? nage : 0;
            m = __popcll(__ballot(used));
        }
    }
    state->ids[lane] = id;
    state->ages[lane] = age;
    if (lane == 0) { state->next_id = next; state->m = m; }
    const double *last = contacts + (size_t)(B - 1) * K * VISTAF_NCONTACT;
    for (int e = lane; e < K * VISTAF_NCONTACT; e += 64) state->rows[e] = last[e];
}

}  // namespace

struct vistaf_track_handle {
    int h = 0, w = 0, P = 0, maxB = 0, K = 0;
    double gate_px = 0.0;
    bool reset_pending = true;             // the state is cleared at the head of the next update, on that update's stream
    unsigned int *ovl = nullptr;           // [maxB, K*K] overlap histograms
    int32_t *linkrow = nullptr;            // [maxB, 64] parent | origin << 8 of every row, for k_tr_ids
    int8_t *carry_plane = nullptr;         // [P] index plane of the last frame
    TrackState *state = nullptr;
    DeviceAllocs mem;
};

extern "C" {

void vistaf_track_destroy(vistaf_track_handle *tr)
{
    if (!tr) return;
    tr->mem.free_all();
    delete tr;
}

int vistaf_track_create(int h, int w, int max_batch, int max_contacts, double gate_px, vistaf_track_handle **out)
{
    if (!out) return set_error(VISTAF_E_INVALID, "null argument");
    *out = nullptr;
    if (h < 1 || w < 1 || (long long)h * w > 0x7fffffffll) return set_error(VISTAF_E_INVALID, "frame size must be >= 1 x 1 and below 2^31 pixels");
    if (max_batch < 1) return set_error(VISTAF_E_INVALID, "max_batch must be >= 1");
    if (max_contacts < 1 || max_contacts > VISTAF_MAX_CONTACTS) return set_error(VISTAF_E_INVALID, "max_contacts must be 1..64");
    if (!(gate_px >= 0.0) || !(gate_px <= 1.7976931348623157e308)) return set_error(VISTAF_E_INVALID, "gate_px must be finite and >= 0");
    Created<vistaf_track_handle> tr(new vistaf_track_handle(), vistaf_track_destroy);
    tr->h = h; tr->w = w; tr->P = h * w; tr->maxB = max_batch; tr->K = max_contacts; tr->gate_px = gate_px;
    TRY(tr->mem.alloc(&tr->ovl, (size_t)max_batch * max_contacts * max_contacts));
    TRY(tr->mem.alloc(&tr->linkrow, (size_t)max_batch * TR_MAXK));
    TRY(tr->mem.alloc(&tr->carry_plane, (size_t)tr->P + 16));
    TRY(tr->mem.alloc(&tr->state, 1));
    *out = tr.release();
    return 0;
}

int vistaf_track_reset(vistaf_track_handle *tr)
{
    if (!tr) return set_error(VISTAF_E_INVALID, "null argument");
    tr->reset_pending = true;
    return 0;
}

int vistaf_track_update(vistaf_track_handle *tr, const int8_t *d_contact_index, const double *d_contacts, const int32_t *d_count, int B,
                        double *d_tracks, int32_t *d_fate, void *stream)
{
    if (!tr || !d_contact_index || !d_contacts || !d_count || !d_tracks || !d_fate) return set_error(VISTAF_E_INVALID, "null argument");
    if (B < 1 || B > tr->maxB) return set_error(VISTAF_E_INVALID, "batch must be 1..max_batch");
    hipStream_t st = (hipStream_t)stream;
    const int K = tr->K, P = tr->P;
    if (tr->reset_pending) {
        HIPCHK(hipMemsetAsync(tr->state, 0, sizeof(TrackState), st));           // m = 0, next_id = 0
        HIPCHK(hipMemsetAsync(tr->carry_plane, 0xff, (size_t)P, st));
        tr->reset_pending = false;
    }
    if (ct_chunked(B, P)) {
        const int nblk = (P + TR_CHUNK - 1) / TR_CHUNK;
        HIPCHK(hipMemsetAsync(tr->ovl, 0, sizeof(unsigned int) * (size_t)B * K * K, st));
        hipLaunchKernelGGL(k_tr_overlap<256>, dim3(nblk, B), dim3(256), 0, st, d_contact_index, tr->carry_plane, K, P, TR_CHUNK / 16, tr->ovl);
    } else {
        hipLaunchKernelGGL(k_tr_overlap<1024>, dim3(1, B), dim3(1024), 0, st, d_contact_index, tr->carry_plane, K, P, (P >> 4) + 1, tr->ovl);
    }
    if (int rc = launch_ok("k_tr_overlap")) return rc;
    HIPCHK(hipMemcpyAsync(tr->carry_plane, d_contact_index + (size_t)(B - 1) * P, (size_t)P, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(k_tr_link, dim3(B), dim3(64), 0, st, tr->ovl, d_contacts, d_count, tr->state, K, tr->gate_px > 0.0 ? 1 : 0,
                       tr->gate_px * tr->gate_px, d_tracks, d_fate, tr->linkrow);
    if (int rc = launch_ok("k_tr_link")) return rc;
    hipLaunchKernelGGL(k_tr_ids, dim3(1), dim3(64), 0, st, tr->linkrow, d_contacts, B, K, tr->state, d_tracks);
    return launch_ok("k_tr_ids");
}

}  // extern "C"
