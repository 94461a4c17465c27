// Per-contact read-out of the planes a predict leaves behind (include/vistaf_ftp.h, vistaf_ftp_contacts): one record per 8-connected
// component of the blob filter's `kept` mask -- pixel count, bounding box, contact pixels / area, volume, peak and its first pixel,
// depth-weighted centroid, force of the contact's own volume.  An extension: the reference reports one set of scalars per frame only.
//
// Nothing is labelled again.  The session's label plane (root = smallest pixel index of the component, -1 off the candidates) and
// `peak_bits` (the component's peak at its root, left by launch_blob_filter) identify and rank the contacts:
//   k_ct_roots   every kept root goes into the frame's root list (an atomic counter hands out the slots; the order of the list does not
//                matter, see k_ct_rank) and every kept pixel that attains its component's peak takes part in an integer atomicMin on
//                arg[root]: the first pixel of the maximum, np.argmax's choice
//   k_ct_rank    one workgroup per frame: K rounds of "largest key below the previous one" over the root list, key = peak bits << 32 |
//                ~argmax -- a total order (the arg-max pixels of two components differ), so the result does not depend on the order of
//                the list.  arg[root] is then overwritten with the contact's row, -1 for the contacts beyond K
//   k_ct_accum   ONE pass over the pixels: a wave takes 64 consecutive pixels, and for every row present among them the wave reduces
//                the counts (ballots), the box (integer max) and the three float64 sums (DPP tree, a fixed order) and lane 0 adds them
//                to the wave's own accumulators in LDS; the block then adds its waves up in wave order into a partial record
//   k_ct_final   adds the blocks' partial records up in block order, one thread per (row, field), and writes the table
// Every float64 sum is formed in an order fixed by the launch geometry alone, and every atomic is an integer min / add whose result
// does not depend on the order of arrival: two calls on the same state give the same bits.
// Two tiers, as launch_tail: one 1024-thread workgroup per frame for small frames (the planes sit in L2), 256-thread workgroups over
// chunks of CT_CHUNK pixels for frames where one workgroup per frame would leave the chip idle.  Same kernels, another grid.
#include "kernels.hpp"

namespace vf {

namespace {

// partial record of one contact: pixels, contact pixels (sums), x0, y0 (min), x1, y1 (max), then the float64 sums of depth, x * depth, y * depth
constexpr int CT_NF = 9, CT_F_MIN = 2, CT_F_MAX = 4, CT_F_DBL = 6;
constexpr int CT_CHUNK = 8192, CT_MAXK = 64;

__device__ inline unsigned long long ct_identity(int f) { return (f >= CT_F_MIN && f < CT_F_MAX) ? ~0ull : 0ull; }
__device__ inline unsigned long long ct_combine(int f, unsigned long long a, unsigned long long b)
{
    if (f < CT_F_MIN) return a + b;
    if (f < CT_F_MAX) return b < a ? b : a;
    if (f < CT_F_DBL) return b > a ? b : a;
    return (unsigned long long)__double_as_longlong(__longlong_as_double((long long)a) + __longlong_as_double((long long)b));
}

__global__ __launch_bounds__(256) void k_ct_roots(const float *__restrict__ depth, const uint8_t *__restrict__ kept, const int32_t *__restrict__ labels,
                                                  const unsigned int *__restrict__ peak_bits, const int32_t *__restrict__ status,
                                                  int32_t *__restrict__ arg, int32_t *__restrict__ list, int cap, int *__restrict__ nroots, int P)
{
    const size_t b = blockIdx.y;
    if (status[b] != 0) return;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < P; p += gridDim.x * blockDim.x) {
        const size_t i = b * (size_t)P + p;
        if (!kept[i]) continue;
        const int r = labels[i];
        if ((unsigned int)r >= (unsigned int)P) continue;
        if (r == p) { const int s = atomicAdd(&nroots[b], 1); if (s < cap) list[b * (size_t)cap + s] = p; }
        if (__float_as_uint(depth[i]) == peak_bits[b * (size_t)P + r]) atomicMin(&arg[b * (size_t)P + r], p);
    }
}

__global__ __launch_bounds__(256) void k_ct_rank(const int32_t *__restrict__ list, int cap, const int *__restrict__ nroots,
                                                 const unsigned int *__restrict__ peak_bits, const int32_t *__restrict__ status, int32_t *__restrict__ arg,
                                                 int K, unsigned long long *__restrict__ selkey, int *__restrict__ nsel, int P)
{
    __shared__ unsigned long long s64[16];
    __shared__ unsigned long long sk[CT_MAXK];
    const size_t b = blockIdx.x;
    const int total = status[b] == 0 ? nroots[b] : 0;
    const int n = total < cap ? total : cap;
    const int kk = n < K ? n : K;
    const int32_t *L = list + b * (size_t)cap;
    const unsigned int *PB = peak_bits + b * (size_t)P;
    int32_t *A = arg + b * (size_t)P;
    unsigned long long prev = ~0ull;
    for (int k = 0; k < kk; k++) {
        unsigned long long m = 0;
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            const int r = L[i];
            const unsigned long long key = ((unsigned long long)PB[r] << 32) | (unsigned int)(0xffffffffu - (unsigned int)A[r]);
            if (key < prev && key > m) m = key;
        }
        m = block_max_u64(m, s64);
        if (threadIdx.x == 0) sk[k] = m;
        prev = m;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int r = L[i];
        const unsigned long long key = ((unsigned long long)PB[r] << 32) | (unsigned int)(0xffffffffu - (unsigned int)A[r]);
        int slot = -1;
        if (kk > 0 && key >= sk[kk - 1])
            for (int k = 0; k < kk; k++) if (sk[k] == key) slot = k;
        A[r] = slot;
    }
    for (int k = threadIdx.x; k < kk; k += blockDim.x) selkey[b * CT_MAXK + k] = sk[k];
    if (threadIdx.x == 0) nsel[b] = total;
}

template <int NT>
__global__ __launch_bounds__(NT) void k_ct_accum(const float *__restrict__ depth, const uint8_t *__restrict__ kept, const int32_t *__restrict__ labels,
                                                 const int32_t *__restrict__ slotmap, const int *__restrict__ nsel, const int32_t *__restrict__ status,
                                                 float eps, int K, int chunk, unsigned long long *__restrict__ part, int8_t *__restrict__ index, int P, int w)
{
    extern __shared__ unsigned long long ct_acc[];        // [NT / 64 waves][K rows][CT_NF]
    const size_t b = blockIdx.y;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    constexpr int NW = NT / 64;
    const int total = status[b] == 0 ? nsel[b] : 0;
    const int kk = total < K ? total : K;
    unsigned long long *A = ct_acc + (size_t)wid * K * CT_NF;
    for (int i = lane; i < kk * CT_NF; i += 64) A[i] = ct_identity(i % CT_NF);
    __syncthreads();
    const int p_begin = blockIdx.x * chunk, p_end = p_begin + chunk < P ? p_begin + chunk : P;
    for (int p0 = p_begin + wid * 64; p0 < p_end; p0 += NT) {
        const int p = p0 + lane;
        const bool in = p < p_end;
        const size_t i = b * (size_t)P + (in ? p : 0);
        int slot = -1;
        float d = 0.f;
        if (in && kk > 0 && kept[i]) {
            const int r = labels[i];
            if ((unsigned int)r < (unsigned int)P) slot = slotmap[b * (size_t)P + r];
            if (slot >= kk) slot = -1;
            d = depth[i];
        }
        if (index && in) index[i] = (int8_t)slot;
        unsigned long long active = __ballot(slot >= 0);
        if (!active) continue;
        const int y = p / w, x = p - y * w;
        while (active) {
            const int leader = __ffsll((long long)active) - 1;
            const int s0 = __shfl(slot, leader, 64);
            const bool same = slot == s0;
            const bool c = same && d > eps;
            const unsigned long long m_same = __ballot(same), m_c = __ballot(c);
            const unsigned int nx0 = wave_max_u32(same ? ~(unsigned int)x : 0u), ny0 = wave_max_u32(same ? ~(unsigned int)y : 0u);
            const unsigned int x1 = wave_max_u32(same ? (unsigned int)x : 0u), y1 = wave_max_u32(same ? (unsigned int)y : 0u);
            const double dv = c ? (double)d : 0.0;
            const double sv = wave_sum(dv), sx = wave_sum(dv * (double)x), sy = wave_sum(dv * (double)y);
            if (lane == 0) {
                unsigned long long *R = A + s0 * CT_NF;
                R[0] += (unsigned long long)__popcll(m_same);
                R[1] += (unsigned long long)__popcll(m_c);
                R[2] = ct_combine(2, R[2], (unsigned long long)~nx0); R[3] = ct_combine(3, R[3], (unsigned long long)~ny0);
                R[4] = ct_combine(4, R[4], (unsigned long long)x1); R[5] = ct_combine(5, R[5], (unsigned long long)y1);
                R[6] = ct_combine(6, R[6], (unsigned long long)__double_as_longlong(sv));
                R[7] = ct_combine(7, R[7], (unsigned long long)__double_as_longlong(sx));
                R[8] = ct_combine(8, R[8], (unsigned long long)__double_as_longlong(sy));
            }
            active &= ~m_same;
        }
    }
    __syncthreads();
    unsigned long long *o = part + (b * gridDim.x + blockIdx.x) * (size_t)K * CT_NF;
    for (int i = threadIdx.x; i < kk * CT_NF; i += NT) {
        const int f = i % CT_NF;
        unsigned long long v = ct_acc[i];
        for (int wv = 1; wv < NW; wv++) v = ct_combine(f, v, ct_acc[(size_t)wv * K * CT_NF + i]);
        o[i] = v;
    }
}

__global__ __launch_bounds__(256) void k_ct_final(const unsigned long long *__restrict__ part, int nblk, int K, const unsigned long long *__restrict__ selkey,
                                                  const int *__restrict__ nsel, const int32_t *__restrict__ status, PostParams pp,
                                                  double *__restrict__ contacts, int nfield, int32_t *__restrict__ count)
{
    __shared__ unsigned long long red[CT_MAXK * CT_NF];
    const size_t b = blockIdx.x;
    const int total = status[b] == 0 ? nsel[b] : 0;
    const int kk = total < K ? total : K;
    for (int i = threadIdx.x; i < kk * CT_NF; i += blockDim.x) {
        const int f = i % CT_NF;
        unsigned long long v = ct_identity(f);
        for (int j = 0; j < nblk; j++) v = ct_combine(f, v, part[(b * nblk + j) * (size_t)K * CT_NF + i]);
        red[i] = v;
    }
    __syncthreads();
    double mm_per_px = pp.mm_per_px;
    if (pp.pair_geom) { const double period_px = pp.pair_geom[b].period; mm_per_px = period_px > 1e-12 ? pp.grating_pitch_mm / period_px : 0.0; }
    const double area_px = mm_per_px * mm_per_px;
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        double *row = contacts + (b * K + k) * (size_t)nfield;
        for (int f = 0; f < nfield; f++) row[f] = nan64();
        if (k >= kk) continue;
        const unsigned long long *R = red + k * CT_NF;
        const unsigned long long key = selkey[b * CT_MAXK + k];
        const double cnt = (double)R[1];
        const double vol = __longlong_as_double((long long)R[6]);
        const double volume_cm3 = cnt > 0 ? (double)(float)vol * area_px / 1000.0 : 0.0;
        row[0] = (double)R[0];
        row[1] = cnt;
        row[2] = cnt * area_px;
        row[3] = volume_cm3;
        row[4] = (double)__uint_as_float((unsigned int)(key >> 32));
        row[5] = (double)(0xffffffffu - (unsigned int)(key & 0xffffffffu));
        if (cnt > 0) { row[6] = __longlong_as_double((long long)R[7]) / vol; row[7] = __longlong_as_double((long long)R[8]) / vol; }
        row[8] = curve_eval(pp.force_curve, volume_cm3);
        row[9] = (double)R[2]; row[10] = (double)R[3]; row[11] = (double)R[4]; row[12] = (double)R[5];
    }
    if (threadIdx.x == 0) count[b] = total;
}

}  // namespace

bool ct_chunked(int B, int P) { return big_frames(B, P); }      // the frames launch_tail splits as well

int contact_root_capacity(int h, int w) { return ((h + 1) / 2) * ((w + 1) / 2); }      // 8-connected components of an h x w mask: no more than this
size_t contact_part_words(int max_batch, int P)
{
    const size_t nblk = ((size_t)P + CT_CHUNK - 1) / CT_CHUNK;       // at least the one block per frame of the small tier
    return (size_t)max_batch * nblk * CT_MAXK * CT_NF;
}

void launch_contacts(const float *depth, const uint8_t *kept, const int32_t *labels, const unsigned int *peak_bits, const int32_t *status,
                     PostParams pp, const ContactScratch &cs, int K, double *contacts, int nfield, int32_t *count, int8_t *index, int B, int h, int w,
                     hipStream_t st)
{
    const int P = h * w;
    hipMemsetAsync(cs.arg, 0x7f, sizeof(int32_t) * (size_t)B * P, st);       // above every pixel index
    hipMemsetAsync(cs.nroots, 0, sizeof(int) * B, st);
    const int gx = (P + 256 * 8 - 1) / (256 * 8);
    hipLaunchKernelGGL(k_ct_roots, dim3(gx, B), dim3(256), 0, st, depth, kept, labels, peak_bits, status, cs.arg, cs.list, cs.cap, cs.nroots, P);
    hipLaunchKernelGGL(k_ct_rank, dim3(B), dim3(256), 0, st, cs.list, cs.cap, cs.nroots, peak_bits, status, cs.arg, K, cs.selkey, cs.nsel, P);
    int nblk = 1;
    if (ct_chunked(B, P)) {
        nblk = (P + CT_CHUNK - 1) / CT_CHUNK;
        hipLaunchKernelGGL(k_ct_accum<256>, dim3(nblk, B), dim3(256), sizeof(unsigned long long) * 4 * K * CT_NF, st, depth, kept, labels, cs.arg, cs.nsel,
                           status, (float)pp.depth_eps_mm, K, CT_CHUNK, cs.part, index, P, w);
    } else {
        static DynLdsOnce lds_once;
        ensure_dyn_lds(lds_once, (const void *)k_ct_accum<1024>, (int)sizeof(unsigned long long) * 16 * CT_MAXK * CT_NF);
        hipLaunchKernelGGL(k_ct_accum<1024>, dim3(1, B), dim3(1024), sizeof(unsigned long long) * 16 * K * CT_NF, st, depth, kept, labels, cs.arg, cs.nsel,
                           status, (float)pp.depth_eps_mm, K, P, cs.part, index, P, w);
    }
    hipLaunchKernelGGL(k_ct_final, dim3(B), dim3(256), 0, st, cs.part, nblk, K, cs.selkey, cs.nsel, status, pp, contacts, nfield, count);
}

}  // namespace vf
