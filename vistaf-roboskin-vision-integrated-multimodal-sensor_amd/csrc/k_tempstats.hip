// Statistics of a float32 map over a valid mask, equal to NumPy's to the last bit (vistaf_tsensor_map_statistics, include/vistaf_tempsensor.h):
// writers.temperature_statistics = np.mean / np.median / np.std / np.min / np.max of t[valid] and its length (multimodal_sensor.py:558-567).
//
// What NumPy 2.x computes for a contiguous float32 vector v of n values (numpy/_core/_methods.py, loops_utils.h.src):
//   sum   np.add.reduce: the accumulator starts at 0.0f and takes the pairwise sum of each 8192-element buffer of v in turn;
//         pairwise(a, m): m < 8 -> 0.0f + a0 + a1 ...; m <= 128 -> 8 strided accumulators, ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the
//         remainder in sequence; else split at m/2 rounded down to a multiple of 8.  The tree depends on n only.
//   mean  f32(f64(sum) / n)                                  (float32 scalar / intp divides in float64, cast back)
//   std   sqrt(f32(f64(sum_pairwise(f32(f32(v - mean)^2))) / n)) in float32 (np.var's two-pass form)
//   median  the middle order statistic (odd n) or f32(f32(0 + a + b) / 2) (even n): the mean of the one or two middle elements
//   min / max  NaN if any value is NaN.  With no value: NaN statistics, count 0.
// Order of the work, all on one stream, no float atomics (deterministic for a given n):
//   count (valid pixels, NaNs, min, max per 4096-pixel tile) -> one-block scan of the tile counts -> row-major scatter of the valid values ->
//   exact median through launch_select (select.hpp / k_big.hip, the finite valid values) -> per-8192 buffer pairwise sums (one workgroup per
//   buffer: leaves in parallel, inner nodes on one lane) -> one workgroup adds the buffer sums in order -> the same two steps on the squares.
// Known difference: the median is selected among the FINITE valid values; NumPy's counts +-inf too (only an explicit mask can hold them; the
// chain's isfinite mask never does).  The sign of a zero min / max when +0 and -0 tie follows no fixed element order here (nor in NumPy's
// SIMD reduction).
#include "host_util.hpp"

namespace vf {
namespace {

constexpr int ST_T = 256;                  // threads of the tile kernels
constexpr int ST_PT = 16;                  // consecutive pixels per thread
constexpr int ST_TILE = ST_T * ST_PT;      // 4096 pixels per tile
constexpr int ST_BUF = 8192;               // NumPy's reduction buffer
constexpr int ST_LEAF = 128;               // NumPy's pairwise block (PW_BLOCKSIZE)
constexpr int ST_MAXLEAF = ST_BUF / 64;    // leaves of a buffer are >= 64 values long once it exceeds 128

struct StState {
    uint32_t n, nnan;
    float mn, mx, mean, sum, sum2, med;
    int32_t cnt;
    float req;                              // launch_select's request: negative = the median
};

struct StWork {
    StState *s;
    uint8_t *sel;                           // valid & finite: the selection's mask
    float *vals;                            // the valid values, row-major
    uint32_t *tcnt, *tnan, *toff;
    float *tmin, *tmax, *bsum;
};

__device__ inline bool st_valid(const float *m, const uint8_t *valid, size_t i)
{
    return valid ? valid[i] != 0 : finitef(m[i]);
}

__global__ void k_st_init(StState *s)
{
    s->n = 0; s->nnan = 0; s->req = -1.0f; s->cnt = 0;
}

// per tile: valid count, NaNs among them, min / max of the non-NaN ones; the selection mask
__global__ __launch_bounds__(ST_T) void k_st_count(const float *__restrict__ m, const uint8_t *__restrict__ valid, StWork w, size_t P)
{
    __shared__ float smn[ST_T], smx[ST_T];
    __shared__ uint32_t sc[ST_T], sn[ST_T];
    const size_t i0 = (size_t)blockIdx.x * ST_TILE + (size_t)threadIdx.x * ST_PT;
    uint32_t c = 0, nn = 0;
    float mn = INFINITY, mx = -INFINITY;
    for (int k = 0; k < ST_PT; k++) {
        const size_t i = i0 + k;
        if (i >= P) break;
        const float x = m[i];
        const bool v = st_valid(m, valid, i);
        w.sel[i] = (uint8_t)(v && finitef(x));
        if (!v) continue;
        c++;
        if (x != x) { nn++; continue; }
        mn = fminf(mn, x); mx = fmaxf(mx, x);
    }
    sc[threadIdx.x] = c; sn[threadIdx.x] = nn; smn[threadIdx.x] = mn; smx[threadIdx.x] = mx;
    __syncthreads();
    for (int o = ST_T / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            sc[threadIdx.x] += sc[threadIdx.x + o]; sn[threadIdx.x] += sn[threadIdx.x + o];
            smn[threadIdx.x] = fminf(smn[threadIdx.x], smn[threadIdx.x + o]); smx[threadIdx.x] = fmaxf(smx[threadIdx.x], smx[threadIdx.x + o]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { w.tcnt[blockIdx.x] = sc[0]; w.tnan[blockIdx.x] = sn[0]; w.tmin[blockIdx.x] = smn[0]; w.tmax[blockIdx.x] = smx[0]; }
}

// exclusive scan of the tile counts (tile order), totals, min / max; one workgroup
__global__ __launch_bounds__(1024) void k_st_scan(StWork w, int ntiles)
{
    __shared__ uint32_t sc[1024];
    __shared__ float smn[1024], smx[1024];
    __shared__ uint32_t carry, nnan;
    __shared__ float mn, mx;
    const int t = threadIdx.x;
    if (t == 0) { carry = 0; nnan = 0; mn = INFINITY; mx = -INFINITY; }
    __syncthreads();
    for (int base = 0; base < ntiles; base += 1024) {
        const int i = base + t;
        const uint32_t c = i < ntiles ? w.tcnt[i] : 0u;
        sc[t] = c;
        smn[t] = i < ntiles ? w.tmin[i] : INFINITY;
        smx[t] = i < ntiles ? w.tmax[i] : -INFINITY;
        uint32_t nn = i < ntiles ? w.tnan[i] : 0u;
        if (nn) atomicAdd(&nnan, nn);                                  // integer count: order does not matter
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {                           // inclusive Hillis-Steele scan
            const uint32_t v = t >= o ? sc[t - o] : 0u;
            __syncthreads();
            sc[t] += v;
            __syncthreads();
        }
        if (i < ntiles) w.toff[i] = carry + sc[t] - c;
        for (int o = 512; o > 0; o >>= 1) {
            if (t < o) { smn[t] = fminf(smn[t], smn[t + o]); smx[t] = fmaxf(smx[t], smx[t + o]); }
            __syncthreads();
        }
        if (t == 0) { carry += sc[1023]; mn = fminf(mn, smn[0]); mx = fmaxf(mx, smx[0]); }
        __syncthreads();
    }
    if (t == 0) { w.s->n = carry; w.s->nnan = nnan; w.s->mn = mn; w.s->mx = mx; }
}

// the valid values of each tile at their row-major rank
__global__ __launch_bounds__(ST_T) void k_st_scatter(const float *__restrict__ m, const uint8_t *__restrict__ valid, StWork w, size_t P)
{
    __shared__ uint32_t sc[ST_T];
    const size_t i0 = (size_t)blockIdx.x * ST_TILE + (size_t)threadIdx.x * ST_PT;
    uint32_t c = 0;
    for (int k = 0; k < ST_PT; k++) {
        const size_t i = i0 + k;
        if (i >= P) break;
        c += st_valid(m, valid, i) ? 1u : 0u;
    }
    sc[threadIdx.x] = c;
    __syncthreads();
    for (int o = 1; o < ST_T; o <<= 1) {
        const uint32_t v = (int)threadIdx.x >= o ? sc[threadIdx.x - o] : 0u;
        __syncthreads();
        sc[threadIdx.x] += v;
        __syncthreads();
    }
    uint32_t pos = w.toff[blockIdx.x] + sc[threadIdx.x] - c;
    for (int k = 0; k < ST_PT; k++) {
        const size_t i = i0 + k;
        if (i >= P) break;
        if (st_valid(m, valid, i)) w.vals[pos++] = m[i];
    }
}

// the pairwise tree of one buffer of m values: the leaf holding offset p
__device__ inline void st_leaf_at(int m, int p, int &s, int &len)
{
    s = 0; len = m;
    while (len > ST_LEAF) {
        int n2 = len / 2;
        n2 -= n2 % 8;
        if (p < s + n2) len = n2;
        else { s += n2; len -= n2; }
    }
}

__device__ inline float st_term(const float *v, int i, int sq, float mean)
{
    const float x = v[i];
    if (!sq) return x;
    const float d = __fsub_rn(x, mean);
    return __fmul_rn(d, d);
}

// pairwise sum of buffer blockIdx.x (values or, sq = 1, squared deviations from the mean); one leaf per thread
__global__ __launch_bounds__(ST_MAXLEAF) void k_st_pairwise(StWork w, int sq)
{
    __shared__ int ls[ST_MAXLEAF], ll[ST_MAXLEAF];
    __shared__ float lv[ST_MAXLEAF];
    __shared__ int nleaf;
    const uint32_t n = w.s->n;
    const size_t b0 = (size_t)blockIdx.x * ST_BUF;
    if (b0 >= n) return;
    const int m = (int)min((size_t)ST_BUF, (size_t)n - b0);
    const float mean = w.s->mean;
    const float *v = w.vals + b0;
    if (threadIdx.x == 0) {
        int k = 0;
        for (int p = 0; p < m; k++) { int s, len; st_leaf_at(m, p, s, len); ls[k] = s; ll[k] = len; p = s + len; }
        nleaf = k;
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < nleaf) {
        const int s = ls[t], len = ll[t];
        float res;
        if (len < 8) {
            res = 0.0f;
            for (int i = 0; i < len; i++) res = __fadd_rn(res, st_term(v, s + i, sq, mean));
        } else {
            float r[8];
#pragma unroll
            for (int j = 0; j < 8; j++) r[j] = st_term(v, s + j, sq, mean);
            int i = 8;
            for (; i < len - (len % 8); i += 8)
#pragma unroll
                for (int j = 0; j < 8; j++) r[j] = __fadd_rn(r[j], st_term(v, s + i + j, sq, mean));
            res = __fadd_rn(__fadd_rn(__fadd_rn(r[0], r[1]), __fadd_rn(r[2], r[3])), __fadd_rn(__fadd_rn(r[4], r[5]), __fadd_rn(r[6], r[7])));
            for (; i < len; i++) res = __fadd_rn(res, st_term(v, s + i, sq, mean));
        }
        lv[t] = res;
    }
    __syncthreads();
    if (t != 0) return;
    // inner nodes, post-order with explicit stacks: node (start, length, stage), values of finished subtrees
    int ns[16], nl[16], stg[16];
    float vs[16];
    int sp = 0, vp = 0, leaf = 0;
    ns[0] = 0; nl[0] = m; stg[0] = 0; sp = 1;
    while (sp > 0) {
        const int top = sp - 1;
        if (nl[top] <= ST_LEAF) { vs[vp++] = lv[leaf++]; sp--; continue; }
        int n2 = nl[top] / 2;
        n2 -= n2 % 8;
        if (stg[top] == 0) { stg[top] = 1; ns[sp] = ns[top]; nl[sp] = n2; stg[sp] = 0; sp++; }
        else if (stg[top] == 1) { stg[top] = 2; ns[sp] = ns[top] + n2; nl[sp] = nl[top] - n2; stg[sp] = 0; sp++; }
        else { const float r = vs[--vp], l = vs[--vp]; vs[vp++] = __fadd_rn(l, r); sp--; }
    }
    w.bsum[blockIdx.x] = vs[0];
}

// 0.0f + the buffer sums in order; sq = 0: the mean, sq = 1: the variance, then the six results
__global__ __launch_bounds__(256) void k_st_final(StWork w, int sq, double *__restrict__ out)
{
    __shared__ float sb[2048];
    __shared__ float acc;
    const uint32_t n = w.s->n;
    const int nb = (int)((n + ST_BUF - 1) / ST_BUF);
    if (threadIdx.x == 0) acc = 0.0f;
    __syncthreads();
    for (int base = 0; base < nb; base += 2048) {
        const int cnt = min(2048, nb - base);
        for (int i = threadIdx.x; i < cnt; i += blockDim.x) sb[i] = w.bsum[base + i];
        __syncthreads();
        if (threadIdx.x == 0) {
            float a = acc;
            for (int i = 0; i < cnt; i++) a = __fadd_rn(a, sb[i]);
            acc = a;
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    StState *s = w.s;
    if (!sq) {
        s->sum = acc;
        s->mean = (float)((double)acc / (double)n);
        return;
    }
    s->sum2 = acc;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    if (n == 0) {
        for (int k = 0; k < 5; k++) out[k] = qnan;
        out[5] = 0.0;
        return;
    }
    const float var = (float)((double)acc / (double)n);
    const float sd = (float)sqrt((double)var);                      // correctly rounded float32 sqrt (53 >= 2 * 24 + 2)
    const bool has_nan = s->nnan != 0;
    // np.median: the mean of the middle element(s) starts from 0.0f (turns -0 into +0); a NaN anywhere makes it NaN
    const float med = has_nan ? __int_as_float(0x7fc00000) : __fadd_rn(0.0f, s->med);
    out[0] = (double)s->mean;
    out[1] = (double)med;
    out[2] = (double)sd;
    out[3] = has_nan ? qnan : (double)s->mn;
    out[4] = has_nan ? qnan : (double)s->mx;
    out[5] = (double)n;
}

StWork tstats_scratch(ScratchLayout &L, int h, int w)
{
    const size_t P = (size_t)h * w, nt = (P + ST_TILE - 1) / ST_TILE, nb = (P + ST_BUF - 1) / ST_BUF;
    StWork wk;
    wk.s = L.take<StState>(1, 256, "s");
    wk.vals = L.take<float>(P, 256, "vals");
    wk.sel = L.take<uint8_t>(P, 256, "sel");
    wk.tcnt = L.take<uint32_t>(nt, 256, "tcnt");
    wk.tnan = L.take<uint32_t>(nt, 256, "tnan");
    wk.toff = L.take<uint32_t>(nt, 256, "toff");
    wk.tmin = L.take<float>(nt, 256, "tmin");
    wk.tmax = L.take<float>(nt, 256, "tmax");
    wk.bsum = L.take<float>(nb, 256, "bsum");
    return wk;
}

}  // namespace

size_t tstats_scratch_bytes(int h, int w, ScratchRec *rec) { ScratchLayout L(nullptr, rec); tstats_scratch(L, h, w); return L.bytes(); }

bool tstats_needs_big_scratch(int h, int w) { return big_frames(1, h * w); }

void launch_tstats(const float *map, const uint8_t *valid, int h, int w, void *scratch, void *big_scratch, double *out, hipStream_t st)
{
    const size_t P = (size_t)h * w;
    ScratchLayout L(scratch);
    const StWork wk = tstats_scratch(L, h, w);
    const unsigned nt = (unsigned)((P + ST_TILE - 1) / ST_TILE), nb = (unsigned)((P + ST_BUF - 1) / ST_BUF);
    hipLaunchKernelGGL(k_st_init, dim3(1), dim3(1), 0, st, wk.s);
    hipLaunchKernelGGL(k_st_count, dim3(nt), dim3(ST_T), 0, st, map, valid, wk, P);
    hipLaunchKernelGGL(k_st_scan, dim3(1), dim3(1024), 0, st, wk, (int)nt);
    hipLaunchKernelGGL(k_st_scatter, dim3(nt), dim3(ST_T), 0, st, map, valid, wk, P);
    launch_select(map, wk.sel, P, nullptr, false, &wk.s->req, 1, &wk.s->med, &wk.s->cnt, 1, (int)P, st, big_scratch);
    hipLaunchKernelGGL(k_st_pairwise, dim3(nb), dim3(ST_MAXLEAF), 0, st, wk, 0);
    hipLaunchKernelGGL(k_st_final, dim3(1), dim3(256), 0, st, wk, 0, out);
    hipLaunchKernelGGL(k_st_pairwise, dim3(nb), dim3(ST_MAXLEAF), 0, st, wk, 1);
    hipLaunchKernelGGL(k_st_final, dim3(1), dim3(256), 0, st, wk, 1, out);
}

}  // namespace vf
