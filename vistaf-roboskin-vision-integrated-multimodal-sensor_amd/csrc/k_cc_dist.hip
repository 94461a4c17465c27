// Mask topology kernels: thresholding, 8-connected components (union-find), largest component,
// exact 3x3 chamfer distance transform.
//   threshold_mask   roi & (q >= thr) & isfinite(q)                       (shape_ftp.py:753)
//   cc_label         cv2.connectedComponentsWithStats(connectivity=8)     (shape_ftp.py:712, :1244)
//   cc_largest       labels == 1 + argmax(areas)                           (shape_ftp.py:716-718)
//   chamfer          cv2.distanceTransform(DIST_L2, 3)                     (shape_ftp.py:725, :1309, :1312)
//
// The rules the kernels share (contact rule, run-length counts, largest-root key, chamfer metric and closed form, LDS limits) are in
// mask_rules.hpp; the LDS label forest is in backend_device.hpp.
//
// k_cc_label_lds, k_cc_largest, k_chamfer_lds and k_chamfer2 give a frame to one workgroup, so what they write for one another stays on
// one CU: a __threadfence_block() orders it, and k_cc_largest's areas need no agent-scope write-back.  k_cc_init / k_cc_merge /
// k_cc_flatten are grids over all pixels of the batch: workgroups on different CUs unite and flatten the same forest at the same time, so
// there a label word is read with an agent-scope relaxed atomic load (served by L2, never a stale L1 line) and changed with an agent-scope
// atomicMin.  k_ccl_area / k_ccl_best / k_ccl_out are such grids too; they meet only in integer atomics (areas, the best key), which the
// next launch reads.
#include <cstdlib>
#include "kernels.hpp"
#include "backend_device.hpp"

namespace vf {

__global__ void k_threshold_mask(const float *__restrict__ q, const uint8_t *__restrict__ roi, const float *__restrict__ thr,
                                 uint8_t *__restrict__ out, int P)
{
    int p = blockIdx.x * blockDim.x + threadIdx.x;
    size_t b = blockIdx.y;
    if (p >= P) return;
    out[b * (size_t)P + p] = (uint8_t)quality_mask_px(roi[p], q[b * (size_t)P + p], thr[b]);
}
void launch_threshold_mask(const float *q, const uint8_t *roi, const float *thr, uint8_t *out, int B, int P, hipStream_t st)
{
    hipLaunchKernelGGL(k_threshold_mask, dim3((P + 255) / 256, B), dim3(256), 0, st, q, roi, thr, out, P);
}

// ---- union-find ---------------------------------------------------------------------------------
__device__ inline int cc_find(const int32_t *L, int i)
{
    int p = ld_relaxed<__HIP_MEMORY_SCOPE_AGENT>(&L[i]);
    while (p != i) { i = p; p = ld_relaxed<__HIP_MEMORY_SCOPE_AGENT>(&L[i]); }
    return i;
}
__device__ inline void cc_unite(int32_t *L, int a, int b)
{
    for (;;) {
        a = cc_find(L, a);
        b = cc_find(L, b);
        if (a == b) return;
        if (a > b) { int t = a; a = b; b = t; }
        // a < b: hang root b under a if b is still a root
        int old = atomicMin(&L[b], a);
        if (old == b) return;
        b = old;
    }
}

// Connected components (8-neighbourhood) by atomic union-find in global memory for frames too large for the LDS forest below: init, merge and
// flatten as separate launches over all pixels of the batch (one 1024-thread workgroup per frame took 45 ms per call on native 1182 x 1182 crops).  The union is an atomic "hang the larger root under the smaller" at agent scope,
// so the result -- every pixel labelled with the smallest pixel index of its component -- does not depend on which workgroup unites what when.
// init: every mask pixel points at the start of its horizontal run INSIDE its wave's 64-pixel segment (one ballot: a chain of "unite with the left
// neighbour" along a 1000-pixel run is a 1000-hop walk for every later find); merge then links a run to its left neighbour only where it
// crosses a segment boundary, and to the row above
__global__ void k_cc_init(const uint8_t *__restrict__ mask, int32_t *__restrict__ labels, int P, int w)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t b = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const bool in = p < P && mask[b * (size_t)P + (p < P ? p : 0)] != 0;
    const int x = p % w;
    const unsigned long long bits = __ballot(in);
    const unsigned long long rowstart = __ballot(x == 0);
    // lane j starts a run: masked, and lane j - 1 is not masked, or j is the first pixel of a row, or j == 0
    const unsigned long long starts = bits & (~(bits << 1) | rowstart | 1ull);
    if (p >= P) return;
    int lab = -1;
    if (in) {
        const unsigned long long upto = starts & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));
        lab = p - lane + (63 - __clzll((long long)upto));
    }
    labels[b * (size_t)P + p] = lab;
}
__global__ void k_cc_merge(const uint8_t *__restrict__ mask, int32_t *__restrict__ labels, int h, int w)
{
    int p = blockIdx.x * blockDim.x + threadIdx.x;
    size_t b = blockIdx.y;
    int P = h * w;
    if (p >= P) return;
    const uint8_t *m = mask + b * (size_t)P;
    int32_t *L = labels + b * (size_t)P;
    if (!m[p]) return;
    int y = p / w, x = p - y * w;
    const bool left = x > 0 && m[p - 1];
    if ((threadIdx.x & 63) == 0 && left) cc_unite(L, p, p - 1);       // the run continues in the previous segment
    cc_row_contacts(m, p, x, y, w, left, [L](int a, int b) { cc_unite(L, a, b); });
}
__global__ void k_cc_flatten(const uint8_t *__restrict__ mask, int32_t *__restrict__ labels, int P)
{
    int p = blockIdx.x * blockDim.x + threadIdx.x;
    size_t b = blockIdx.y;
    if (p >= P) return;
    int32_t *L = labels + b * (size_t)P;
    if (mask[b * (size_t)P + p]) { int r = cc_find(L, p); if (r != p) atomicMin(&L[p], r); }
}

// ---- LDS-resident variant for frames of at most 65535 pixels: the whole label forest lives in LDS as one uint16 per pixel (cc16_* and
// cc_lds_build in backend_device.hpp, shared with k_backend.hip).  MLDS: the mask plane is staged in LDS too (P bytes behind the forest)
template <bool MLDS>
__global__ __launch_bounds__(1024) void k_cc_label_lds(const uint8_t *__restrict__ mask, int32_t *__restrict__ labels, int h, int w)
{
    extern __shared__ __attribute__((aligned(16))) uint16_t L16[];
    size_t b = blockIdx.x;
    int P = h * w;
    const uint8_t *m = cc_lds_build<MLDS>(mask + b * (size_t)P, h, w, L16);
    int32_t *out = labels + b * (size_t)P;
    for (int p = threadIdx.x; p < P; p += blockDim.x) out[p] = m[p] ? cc16_find(L16, p) : -1;
}

int cc_label_tier(int h, int w, bool force_global)
{
    const int P = h * w;
    if (force_global || P > 65535) return CCT_GLOBAL;
    if (cc_lds_bytes(P) <= (size_t)LDS_DYN_MAX) return CCT_LDS_MASK;
    return cc_lds_forest_bytes(P) <= (size_t)LDS_DYN_HEADROOM ? CCT_LDS : CCT_GLOBAL;
}

template <bool MLDS>
static void launch_cc_label_lds(const uint8_t *mask, int32_t *labels, int B, int h, int w, hipStream_t st)
{
    static DynLdsOnce lds_once;
    ensure_dyn_lds(lds_once, (const void *)k_cc_label_lds<MLDS>, LDS_DYN_MAX);
    hipLaunchKernelGGL(k_cc_label_lds<MLDS>, dim3(B), dim3(1024), MLDS ? cc_lds_bytes(h * w) : cc_lds_forest_bytes(h * w), st, mask, labels, h, w);
}
void launch_cc_label(const uint8_t *mask, int32_t *labels, int B, int h, int w, hipStream_t st, bool force_global)
{
    int P = h * w;
    const int tier = cc_label_tier(h, w, force_global);
    if (tier == CCT_LDS_MASK) return launch_cc_label_lds<true>(mask, labels, B, h, w, st);
    if (tier == CCT_LDS) return launch_cc_label_lds<false>(mask, labels, B, h, w, st);
    const dim3 g((P + 255) / 256, B);
    hipLaunchKernelGGL(k_cc_init, g, dim3(256), 0, st, mask, labels, P, w);
    hipLaunchKernelGGL(k_cc_merge, g, dim3(256), 0, st, mask, labels, h, w);
    hipLaunchKernelGGL(k_cc_flatten, g, dim3(256), 0, st, mask, labels, P);
}

// areas per root (wave-aggregated atomics), then the largest root (ties: smallest root index = first
// in raster order = smallest OpenCV label), then out = (label == best) & and_static
__global__ __launch_bounds__(1024) void k_cc_largest(const int32_t *__restrict__ labels, int32_t *__restrict__ area,
                                                     const uint8_t *__restrict__ and_static, uint8_t *__restrict__ out, int P)
{
    __shared__ unsigned long long scratch[16];
    size_t b = blockIdx.x;
    const int32_t *L = labels + b * (size_t)P;
    int32_t *A = area + b * (size_t)P;
    int lane = threadIdx.x & 63;
    constexpr int U = 4;                    // independent loads in flight per thread (the loops are bound by memory round trips)
    const int T = blockDim.x;
    for (int p = threadIdx.x; p < P; p += T) A[p] = 0;
    __threadfence_block();      // one workgroup per frame: no agent-scope write-back of the L2
    __syncthreads();
    int Pr = ((P + U * 1024 - 1) / (U * 1024)) * (U * 1024);
    int run_root = -1, run_cnt = 0;
    for (int p0 = threadIdx.x; p0 < Pr; p0 += U * T) {
        int root[U];
#pragma unroll
        for (int u = 0; u < U; u++) { int p = p0 + u * T; root[u] = p < P ? L[p] : -1; }
#pragma unroll
        for (int u = 0; u < U; u++) ccl_run_count(root[u], run_root, run_cnt, A, lane);
    }
    ccl_run_flush(run_root, run_cnt, A, lane);
    __threadfence_block();      // one workgroup per frame: no agent-scope write-back of the L2
    __syncthreads();
    unsigned long long best = 0;
    for (int p0 = threadIdx.x; p0 < P; p0 += U * T) {
        int lab[U], ar[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            int p = p0 + u * T;
            lab[u] = p < P ? L[p] : -1;
            ar[u] = p < P ? ld_relaxed<__HIP_MEMORY_SCOPE_AGENT>(&A[p]) : 0;
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            int p = p0 + u * T;
            if (lab[u] != p) continue;
            const unsigned long long key = ccl_key(ar[u], p);
            if (key > best) best = key;
        }
    }
    best = block_max_u64(best, scratch);
    const int broot = ccl_root(best);
    for (int p0 = threadIdx.x; p0 < P; p0 += U * T) {
        int lab[U];
        uint8_t as[U];
#pragma unroll
        for (int u = 0; u < U; u++) { int p = p0 + u * T; lab[u] = p < P ? L[p] : -1; as[u] = (p < P && and_static) ? and_static[p] : (uint8_t)1; }
#pragma unroll
        for (int u = 0; u < U; u++) { int p = p0 + u * T; if (p < P) out[b * (size_t)P + p] = (uint8_t)(lab[u] == broot && as[u]); }
    }
}

// The same three steps as kernels over all pixels of the batch, for frames where one workgroup per frame leaves the chip idle (eight native
// crops: 1.46 ms in k_cc_largest): areas (run-length per wave, integer atomics), key of the largest root per frame (atomic max), output.
__global__ __launch_bounds__(256) void k_ccl_area(const int32_t *__restrict__ labels, int32_t *__restrict__ area, int P)
{
    constexpr int U = 4;
    const size_t b = blockIdx.y;
    const int32_t *L = labels + b * (size_t)P;
    int32_t *A = area + b * (size_t)P;
    const int lane = threadIdx.x & 63;
    // a wave takes U consecutive 64-pixel tiles: consecutive tiles mostly belong to the same (large) component
    const int p0 = (blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * (64 * U) + lane;
    int root[U];
#pragma unroll
    for (int u = 0; u < U; u++) { const int p = p0 + u * 64; root[u] = p < P ? L[p] : -1; }
    int run_root = -1, run_cnt = 0;
#pragma unroll
    for (int u = 0; u < U; u++) ccl_run_count(root[u], run_root, run_cnt, A, lane);
    ccl_run_flush(run_root, run_cnt, A, lane);
}
__global__ __launch_bounds__(256) void k_ccl_best(const int32_t *__restrict__ labels, const int32_t *__restrict__ area, unsigned long long *__restrict__ best, int P)
{
    const size_t b = blockIdx.y;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long key = 0;
    if (p < P && labels[b * (size_t)P + p] == p) key = ccl_key(area[b * (size_t)P + p], p);
    if (!__ballot(key != 0)) return;
    for (int o = 32; o; o >>= 1) { const unsigned long long v = __shfl_xor(key, o, 64); key = v > key ? v : key; }
    if ((threadIdx.x & 63) == 0) atomicMax(&best[b], key);
}
__global__ __launch_bounds__(256) void k_ccl_out(const int32_t *__restrict__ labels, const unsigned long long *__restrict__ best,
                                                 const uint8_t *__restrict__ and_static, uint8_t *__restrict__ out, int P)
{
    const size_t b = blockIdx.y;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const int broot = ccl_root(best[b]);
    out[b * (size_t)P + p] = (uint8_t)(labels[b * (size_t)P + p] == broot && (and_static ? and_static[p] : (uint8_t)1));
}

int cc_largest_tier(int B, int P, bool have_best, int force)
{
    if (force) return force == CCL_BATCH && have_best ? CCL_BATCH : CCL_FRAME;
    return have_best && big_frames(B, P) ? CCL_BATCH : CCL_FRAME;
}

// best: [B] scratch words (large frames only)
void launch_cc_largest(const int32_t *labels, int32_t *area_scratch, unsigned long long *best, const uint8_t *and_static,
                       uint8_t *out, int B, int P, hipStream_t st, int force)
{
    if (cc_largest_tier(B, P, best != nullptr, force) == CCL_BATCH) {
        (void)hipMemsetAsync(area_scratch, 0, (size_t)B * P * sizeof(int32_t), st);
        (void)hipMemsetAsync(best, 0, (size_t)B * sizeof(unsigned long long), st);
        hipLaunchKernelGGL(k_ccl_area, dim3((P + 1023) / 1024, B), dim3(256), 0, st, labels, area_scratch, P);
        const dim3 g((P + 255) / 256, B);
        hipLaunchKernelGGL(k_ccl_best, g, dim3(256), 0, st, labels, area_scratch, best, P);
        hipLaunchKernelGGL(k_ccl_out, g, dim3(256), 0, st, labels, best, and_static, out, P);
        return;
    }
    hipLaunchKernelGGL(k_cc_largest, dim3(B), dim3(1024), 0, st, labels, area_scratch, and_static, out, P);
}

// ---- chamfer distance ---------------------------------------------------------------------------
constexpr int CH_INF = 1 << 20;     // row distance of a row without a zero pixel (k_rowdist's plane)

// horizontal distance to the nearest "zero" pixel of each row, CH_INF when the row has none: one wave per row, 64 columns at a time.
// Left to right the position of the last zero pixel at or before x is a prefix maximum (DPP scan + carry across chunks), right to left the next
// one a suffix minimum; the distances are the same integers the two sequential sweeps count up (a thread per row was 0.6 ms per call on
// eight native crops: 1182 dependent, uncoalesced steps).
__global__ __launch_bounds__(256) void k_rowdist(const uint8_t *__restrict__ src, int invert, int32_t *__restrict__ g, int h, int w, int B)
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= B * h) return;
    const uint8_t *s = src + (size_t)row * w;
    int32_t *o = g + (size_t)row * w;
    int carry = ROW_NO_ZERO;
    for (int x0 = 0; x0 < w; x0 += 64) {
        const int x = x0 + lane;
        const bool zero = x < w && (invert ? (s[x] != 0) : (s[x] == 0));
        const int lz = row_last_zero(zero, x, carry);
        if (x < w) o[x] = lz == ROW_NO_ZERO ? CH_INF : x - lz;
    }
    const int far = 0x7fffffff;
    carry = far;
    for (int x0 = ((w - 1) / 64) * 64; x0 >= 0; x0 -= 64) {
        const int x = x0 + lane;
        const bool zero = x < w && (invert ? (s[x] != 0) : (s[x] == 0));
        int nz = wave_suffix_min_i32(zero ? x : far, far, lane);
        nz = nz < carry ? nz : carry;
        carry = __builtin_amdgcn_readlane(nz, 0);
        if (x < w && nz != far) { const int d = nz - x; if (d < o[x]) o[x] = d; }
    }
}

// the closed form (chamfer_col_min) over k_rowdist's plane, a thread per pixel
__global__ void k_chamfer_cols(const int32_t *__restrict__ g, float *__restrict__ dist, int h, int w, int cap)
{
    int x = blockIdx.x * blockDim.x + threadIdx.x;
    int y = blockIdx.y;
    size_t b = blockIdx.z;
    if (x >= w) return;
    const int32_t *G = g + b * (size_t)h * w;
    const int best = chamfer_col_min([G, w, x](int yy, int &gx) { gx = G[(size_t)yy * w + x]; return gx < CH_INF; }, y, h, cap);
    dist[b * (size_t)h * w + (size_t)y * w + x] = chamfer_to_float(best);
}

// ---- the two-pass 3x3 chamfer itself (cv::distanceTransform DIST_L2, 3x3 mask: distanceTransform_3x3), one wave per frame.
// Row y of the forward pass is  d(x) = min(t(x), d(x-1) + HV)  with  t(x) = 0 on a zero pixel, else
// min(up-left + DG, up + HV, up-right + DG): t is data-parallel and the recurrence along the row is a min-plus
// prefix scan, so a wave that holds PPL consecutive columns per lane does a row in a few dozen instructions
// (lane-local scan, one DPP wave scan for the carries, one DPP shift for the neighbours across lanes).  The
// backward pass is the mirror image.  Integer arithmetic throughout: results equal the sequential loops bit for
// bit.
// A single wave has nothing else to hide memory latency with, and a row step is short next to a round trip to memory, so the rows are
// prefetched ch2_ring(PPL) rows ahead into registers (the wave is alone on its SIMD: launch_bounds(64) leaves it 512 VGPRs).  The
// depth is what the 6-bit vmcnt counter can tell apart: with aligned rows (w a multiple of 4, planes aligned as hipMalloc leaves them) a
// row is PPL / 4 dword loads of the mask or dwordx4 loads of the temporary plane and as many dwordx4 stores, 2 * PPL / 4 operations, and
// at most 63 may be outstanding behind the load a row waits for.  Other widths load and store element by element (and wait earlier).
__host__ __device__ constexpr int ch2_ring(int ppl) { return ppl == 4 ? 31 : ppl == 8 ? 15 : 6; }

// mask bytes of columns x0 .. x0 + PPL of row y, four to a word (0 beyond the frame)
template <int PPL>
__device__ inline void ch2_load_mask(const uint8_t *__restrict__ src, int y, int h, int w, int x0, bool vec, uint32_t (&m)[PPL / 4])
{
#pragma unroll
    for (int q = 0; q < PPL / 4; q++) {
        const int x = x0 + 4 * q;
        uint32_t v = 0;
        if (y < h && x < w) {
            const uint8_t *s = src + (size_t)y * w + x;
            if (vec) v = *(const uint32_t *)s;
            else {
                v = s[0];
                if (x + 1 < w) v |= (uint32_t)s[1] << 8;
                if (x + 2 < w) v |= (uint32_t)s[2] << 16;
                if (x + 3 < w) v |= (uint32_t)s[3] << 24;
            }
        }
        m[q] = v;
    }
}
// columns x0 .. x0 + PPL of row y of the temporary plane (CH_DIST_MAX beyond the frame; y < 0: no row)
template <int PPL>
__device__ inline void ch2_load_tmp(const int32_t *__restrict__ tmp, int y, int w, int x0, bool vec, int (&v)[PPL])
{
#pragma unroll
    for (int q = 0; q < PPL / 4; q++) {
        const int x = x0 + 4 * q;
        int4 t = make_int4(CH_DIST_MAX, CH_DIST_MAX, CH_DIST_MAX, CH_DIST_MAX);
        if (y >= 0 && x < w) {
            const int32_t *s = tmp + (size_t)y * w + x;
            if (vec) t = *(const int4 *)s;
            else {
                t.x = s[0];
                if (x + 1 < w) t.y = s[1];
                if (x + 2 < w) t.z = s[2];
                if (x + 3 < w) t.w = s[3];
            }
        }
        v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
    }
}
template <int PPL, typename T, typename T4>
__device__ inline void ch2_store_row(T *__restrict__ dst, int y, int w, int x0, bool vec, const T (&v)[PPL])
{
#pragma unroll
    for (int q = 0; q < PPL / 4; q++) {
        const int x = x0 + 4 * q;
        if (x >= w) continue;
        T *d = dst + (size_t)y * w + x;
        if (vec) { T4 t; t.x = v[4 * q]; t.y = v[4 * q + 1]; t.z = v[4 * q + 2]; t.w = v[4 * q + 3]; *(T4 *)d = t; }
        else {
            d[0] = v[4 * q];
            if (x + 1 < w) d[1] = v[4 * q + 1];
            if (x + 2 < w) d[2] = v[4 * q + 2];
            if (x + 3 < w) d[3] = v[4 * q + 3];
        }
    }
}

template <int PPL>
__global__ __launch_bounds__(64) void k_chamfer2(const uint8_t *__restrict__ src_all, int invert, int32_t *__restrict__ tmp_all,
                                                 float *__restrict__ dist_all, int32_t *__restrict__ tmp2_all, float *__restrict__ dist2_all, int B,
                                                 int h, int w)
{
    static_assert(PPL % 4 == 0, "columns per lane come in groups of four");
    constexpr int RING = ch2_ring(PPL);
    // workgroups [B, 2B) (launch_chamfer_pair): the distance to the complementary set of the same frames, into the second pair of planes
    const int lane = threadIdx.x;
    size_t b = blockIdx.x;
    if (b >= (size_t)B) { b -= B; invert = !invert; tmp_all = tmp2_all; dist_all = dist2_all; }
    const size_t P = (size_t)h * w;
    const uint8_t *src = src_all + b * P;
    int32_t *tmp = tmp_all + b * P;
    float *dist = dist_all + b * P;
    const int x0 = lane * PPL;
    const int step = CH_HV * PPL;
    // every group of four columns is one aligned word of the mask and one aligned 16 bytes of the two 4-byte planes (wave-uniform)
    const bool vec = (w & 3) == 0 && ((uintptr_t)src_all & 3) == 0 && ((uintptr_t)tmp_all & 15) == 0 && ((uintptr_t)dist_all & 15) == 0;

    // ---- forward pass (top-left to bottom-right); the result plane goes to tmp
    {
        int up[PPL];
#pragma unroll
        for (int j = 0; j < PPL; j++) up[j] = CH_DIST_MAX;
        uint32_t ring[RING][PPL / 4];
#pragma unroll
        for (int r = 0; r < RING; r++) ch2_load_mask<PPL>(src, r, h, w, x0, vec, ring[r]);
        for (int y0 = 0; y0 < h; y0 += RING) {
#pragma unroll
            for (int r = 0; r < RING; r++) {
                const int y = y0 + r;
                if (y >= h) break;
                const int upl = wave_shr1(up[PPL - 1], CH_DIST_MAX), upr = wave_shl1(up[0], CH_DIST_MAX);
                int t[PPL];
#pragma unroll
                for (int j = 0; j < PPL; j++) {
                    const bool in = x0 + j < w;
                    const uint32_t px = (ring[r][j >> 2] >> (8 * (j & 3))) & 0xffu;
                    const bool zero = in && (invert ? px != 0 : px == 0);
                    const int a = (j > 0 ? up[j - 1] : upl) + CH_DG, c = (j < PPL - 1 ? up[j + 1] : upr) + CH_DG, u = up[j] + CH_HV;
                    int m = a < u ? a : u;
                    m = c < m ? c : m;
                    t[j] = zero ? 0 : m;
                }
                // next row of the ring
                ch2_load_mask<PPL>(src, y + RING, h, w, x0, vec, ring[r]);
                // d(x) = min(t(x), d(x-1) + HV): lane-local scan, carries across lanes by a wave scan of (last - step * lane)
#pragma unroll
                for (int j = 1; j < PPL; j++) { int v = t[j - 1] + CH_HV; t[j] = v < t[j] ? v : t[j]; }
                const int sc = wave_scan_min_i32(t[PPL - 1] - step * lane, 0x7fffffff) + step * lane;      // final value of this lane's last column
                const int carry = wave_shr1(sc, CH_DIST_MAX);                                     // d(x0 - 1)
#pragma unroll
                for (int j = 0; j < PPL; j++) {
                    int v = carry + CH_HV * (j + 1);
                    up[j] = v < t[j] ? v : t[j];
                }
                ch2_store_row<PPL, int32_t, int4>(tmp, y, w, x0, vec, up);
            }
        }
    }
    __threadfence_block();
    // ---- backward pass (bottom-right to top-left)
    {
        int dn[PPL];
#pragma unroll
        for (int j = 0; j < PPL; j++) dn[j] = CH_DIST_MAX;
        int ring[RING][PPL];
#pragma unroll
        for (int r = 0; r < RING; r++) ch2_load_tmp<PPL>(tmp, h - 1 - r, w, x0, vec, ring[r]);
        for (int y0 = 0; y0 < h; y0 += RING) {
#pragma unroll
            for (int r = 0; r < RING; r++) {
                const int y = h - 1 - (y0 + r);
                if (y < 0) break;
                const int dnl = wave_shr1(dn[PPL - 1], CH_DIST_MAX), dnr = wave_shl1(dn[0], CH_DIST_MAX);
                int t[PPL];
#pragma unroll
                for (int j = 0; j < PPL; j++) {
                    const int a = (j < PPL - 1 ? dn[j + 1] : dnr) + CH_DG, c = (j > 0 ? dn[j - 1] : dnl) + CH_DG, u = dn[j] + CH_HV;
                    int m = a < u ? a : u;
                    m = c < m ? c : m;
                    const int cur = x0 + j < w ? ring[r][j] : CH_DIST_MAX;
                    t[j] = m < cur ? m : cur;
                }
                ch2_load_tmp<PPL>(tmp, y - RING, w, x0, vec, ring[r]);
                // d(x) = min(t(x), d(x+1) + HV): the same scan on mirrored lanes
#pragma unroll
                for (int j = PPL - 2; j >= 0; j--) { int v = t[j + 1] + CH_HV; t[j] = v < t[j] ? v : t[j]; }
                // "lanes to the right": a suffix minimum, taken of (first - step * mirrored lane)
                const int ml = 63 - lane;
                const int first = wave_suffix_min_i32(t[0] - step * ml, 0x7fffffff, lane) + step * ml;     // final value of this lane's first column
                const int carry = wave_shl1(first, CH_DIST_MAX);                                  // d(x0 + PPL)
                float o[PPL];
#pragma unroll
                for (int j = 0; j < PPL; j++) {
                    int v = carry + CH_HV * (PPL - j);
                    dn[j] = v < t[j] ? v : t[j];
                    o[j] = chamfer_to_float(dn[j] > CH_DIST_MAX ? CH_DIST_MAX : dn[j]);
                }
                ch2_store_row<PPL, float, float4>(dist, y, w, x0, vec, o);
            }
        }
    }
}

// ---- the same distances from the closed form, one 1024-thread workgroup per frame, exact up to `cap` rows (all the callers look at).
// The chamfer metric between two pixels is HV * (max - min) + DG * min of (|dx|, |dy|), and it grows with |dx| for a fixed |dy|, so
//   d(x, y) = min over rows y' of metric(g(y', x), |y - y'|),   g = horizontal distance to the nearest zero pixel of row y'.
// Phase 1 (rows are independent: 16 waves, a DPP max / min scan per 64-pixel chunk) leaves g in LDS as uint16; phase 2 is a short
// loop per pixel with the early exit of k_chamfer_cols.  The two-pass kernel above is one wave per frame and 2 * h dependent row steps.
constexpr uint16_t CHL_NONE = 0xffffu;
__global__ __launch_bounds__(1024) void k_chamfer_lds(const uint8_t *__restrict__ src_all, int invert, float *__restrict__ dist_all, int h, int w,
                                                      int cap)
{
    extern __shared__ uint16_t chl_g[];                  // [h * w]
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const size_t b = blockIdx.x;
    const int P = h * w;
    const uint8_t *src = src_all + b * (size_t)P;
    // phase 1: the zero pixels of a row as ballot words (the byte loads of the row are issued together: one memory round trip per
    // row); the distances to the nearest zero at or left / right of a pixel are then bit scans of those words
    constexpr int CHL_W = 8;                              // 64-pixel words per row handled in registers (w <= 512)
    const int nwords = (w + 63) >> 6;
    for (int y = wid; y < h; y += 16) {
        const uint8_t *row = src + (size_t)y * w;
        uint8_t px[CHL_W];
#pragma unroll
        for (int c = 0; c < CHL_W; c++) { const int x = c * 64 + lane; px[c] = (c < nwords && x < w) ? row[x] : (uint8_t)(invert ? 0 : 1); }
        unsigned long long Z[CHL_W];
#pragma unroll
        for (int c = 0; c < CHL_W; c++) {
            const int x = c * 64 + lane;
            Z[c] = __ballot(c < nwords && x < w && (invert ? px[c] != 0 : px[c] == 0));
        }
#pragma unroll
        for (int c = 0; c < CHL_W; c++) {
            if (c >= nwords) break;
            const int x = c * 64 + lane;
            // nearest zero at or left of x
            int dl = 0x7fff0000;
            {
                const unsigned long long zl = Z[c] & ((2ull << lane) - 1ull);
                if (zl) dl = lane - (63 - __clzll((long long)zl));
                else {
#pragma unroll
                    for (int k = 1; k < CHL_W; k++) {
                        if (c - k < 0) break;
                        if (Z[c - k]) { dl = lane + 64 * k - (63 - __clzll((long long)Z[c - k])); break; }
                    }
                }
            }
            int dr = 0x7fff0000;
            {
                const unsigned long long zr = Z[c] >> lane;
                if (zr) dr = __ffsll((long long)zr) - 1;
                else {
#pragma unroll
                    for (int k = 1; k < CHL_W; k++) {
                        if (c + k >= nwords) break;
                        if (Z[c + k]) { dr = 64 * k - lane + (__ffsll((long long)Z[c + k]) - 1); break; }
                    }
                }
            }
            const int d = dl < dr ? dl : dr;
            if (x < w) chl_g[y * w + x] = d > 0xfffe ? CHL_NONE : (uint16_t)d;
        }
    }
    __syncthreads();
    // phase 2
    float *dist = dist_all + b * (size_t)P;
    for (int p = tid; p < P; p += 1024) {
        const int y = p / w, x = p - y * w;
        const int best = chamfer_col_min([w, x](int yy, int &gx) { gx = (int)chl_g[yy * w + x]; return gx != (int)CHL_NONE; }, y, h, cap);
        dist[p] = chamfer_to_float(best);
    }
}

// the two-pass kernel on nwg workgroups of one wave each, with the columns per lane that cover the width (no tier admits more than 1280)
static void launch_chamfer2(const uint8_t *src, int invert, int32_t *tmp_a, float *dist_a, int32_t *tmp_b, float *dist_b, int nwg, int B, int h, int w,
                            hipStream_t st)
{
    auto *k = w <= 256 ? k_chamfer2<4> : w <= 512 ? k_chamfer2<8> : k_chamfer2<20>;
    hipLaunchKernelGGL(k, dim3(nwg), dim3(64), 0, st, src, invert, tmp_a, dist_a, tmp_b, dist_b, B, h, w);
}
int chamfer_tier(int h, int w, int cap_px, bool force_twopass)
{
    // small caps (the erosion margins): a handful of rows per pixel on 16 waves; for wide bands the per-pixel loop costs more than
    // the one-wave two-pass kernel (measured at cap 46: 345 us against 200 us)
    if (!force_twopass && chamfer_cap_rows(h, cap_px) <= 16 && chamfer_lds_fits(h, w) && w <= 512) return CHT_LDS;
    // beyond the two-pass kernel's 512 columns: closed form of the same two passes, exact up to cap_px (all that the callers look at)
    return w <= 512 ? CHT_TWOPASS : CHT_ROWCOL;
}
int chamfer_pair_tier(int B, int h, int w, int cap_px, bool force_twopass)
{
    // wide bands on wide frames (native crops, band 200 px): the closed form walks up to 2 * cap rows per pixel (0.3 ms per frame, all CUs),
    // the two-pass kernel a frame's rows once each way on one wave per frame and set (4 ms, all frames side by side): the latter from 16 frames on
    const int cap = chamfer_cap_rows(h, cap_px);
    const bool two_pass = (force_twopass || cap > 16 || !chamfer_lds_fits(h, w)) && (w <= 512 || (w <= 1280 && cap > 64 && (B >= 16 || force_twopass)));
    return two_pass ? CHT_TWOPASS : chamfer_tier(h, w, cap_px, false);
}

void launch_chamfer(const uint8_t *src, bool invert, int32_t *rowdist, float *dist, int B, int h, int w, int cap_px, hipStream_t st, bool force_twopass)
{
    const int cap = chamfer_cap_rows(h, cap_px);
    const int tier = chamfer_tier(h, w, cap_px, force_twopass);
    if (tier == CHT_LDS) {
        static DynLdsOnce lds_once;
        ensure_dyn_lds(lds_once, (const void *)k_chamfer_lds, LDS_DYN_MAX);
        hipLaunchKernelGGL(k_chamfer_lds, dim3(B), dim3(1024), (size_t)h * w * 2, st, src, invert ? 1 : 0, dist, h, w, cap);
        return;
    }
    if (tier == CHT_TWOPASS) {
        launch_chamfer2(src, invert ? 1 : 0, rowdist, dist, nullptr, nullptr, B, B, h, w, st);
        return;
    }
    int rows = B * h;
    hipLaunchKernelGGL(k_rowdist, dim3((rows + 3) / 4), dim3(256), 0, st, src, invert ? 1 : 0, rowdist, h, w, B);
    hipLaunchKernelGGL(k_chamfer_cols, dim3((w + 255) / 256, h, B), dim3(256), 0, st, rowdist, dist, h, w, cap);
}

// distance to the zero pixels (-> dist_a) and to the non-zero pixels (-> dist_b) of the same masks.  The two-pass kernel is one wave per
// frame, so both transforms of a batch run side by side in ONE launch of 2B workgroups.  All of them are resident at once: the prefetch rings
// cost 144 to 175 VGPRs, so each of the chip's 1024 SIMDs holds at least two such waves, 2048 or more against the 512 of a batch of 256.
void launch_chamfer_pair(const uint8_t *src, int32_t *tmp_a, float *dist_a, int32_t *tmp_b, float *dist_b, int B, int h, int w, int cap_px,
                         hipStream_t st, bool force_twopass)
{
    if (chamfer_pair_tier(B, h, w, cap_px, force_twopass) != CHT_TWOPASS) {
        launch_chamfer(src, false, tmp_a, dist_a, B, h, w, cap_px, st, false);
        launch_chamfer(src, true, tmp_b, dist_b, B, h, w, cap_px, st, false);
        return;
    }
    launch_chamfer2(src, 0, tmp_a, dist_a, tmp_b, dist_b, 2 * B, B, h, w, st);
}

__global__ void k_erode_by_dist(const float *__restrict__ dist, const uint8_t *__restrict__ src, float margin, uint8_t *__restrict__ out, size_t n)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = (uint8_t)(src[i] && dist[i] > margin);
}
void launch_erode_by_dist(const float *dist, const uint8_t *src, float margin, uint8_t *out, int B, int P, hipStream_t st)
{
    size_t n = (size_t)B * P;
    hipLaunchKernelGGL(k_erode_by_dist, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dist, src, margin, out, n);
}

}  // namespace vf
