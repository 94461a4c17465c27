// Temperature regressors (include/vistaf_tempmodel.h): Code/temperature_sensor.py:230-243 TempModel.predict and :295 predict_map_for_mask
// evaluated per pixel from exported StandardScaler -> PolynomialFeatures -> HuberRegressor (+ IsotonicRegression) parameters.
//
// Every model is evaluated in one canonical basis: the 70 monomials of 4 feature slots up to degree 4, in PolynomialFeatures order
// (degree-major, then combinations with replacement).  A model of F < 4 features leaves slots F..3 at 0; the order of its own monomials
// is the same as in its F-feature basis, so the model's powers map onto canonical slots with a zero-free coefficient per used slot and
// a `used` bit.  Each monomial of degree >= 2 is parent * x_f with f its lowest feature, which is how PolynomialFeatures.transform builds
// its columns; the degree-d blocks above the model's degree are skipped by uniform branches.  Parameters sit in one device block written
// at create time; the map kernel reads them through a kernel-argument pointer (scalar loads).
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/vistaf_tempmodel.h"
#include "host_util.hpp"

using namespace vf;

namespace {

constexpr int NSLOT = 4, NCANON = 70, MAXDEG = 4;
constexpr int DEG_START[MAXDEG + 2] = {0, 1, 5, 15, 35, 70};
constexpr int ISO_LDS_MAX = 2048;            // isotonic entries staged in LDS per launch (16 B each: 32 KB)

struct Canon {
    int8_t f[NCANON];        // feature multiplied in last (the lowest one with a nonzero power)
    int8_t parent[NCANON];   // canonical index of the monomial with one power of f removed
    int8_t pw[NCANON][NSLOT];
};
// PolynomialFeatures.transform's column construction over 4 slots: the degree-d block is, for f = 0..3, x_f times the degree-(d-1)
// monomials whose lowest feature is >= f.
constexpr Canon make_canon()
{
    Canon c{};
    c.f[0] = -1; c.parent[0] = -1;
    int n = 1, idx[NSLOT] = {}, end = 0;
    for (int f = 0; f < NSLOT; f++) { c.f[n] = (int8_t)f; c.parent[n] = 0; c.pw[n][f] = 1; idx[f] = n; n++; }
    end = n;
    for (int d = 2; d <= MAXDEG; d++) {
        int nidx[NSLOT] = {};
        for (int f = 0; f < NSLOT; f++) {
            nidx[f] = n;
            for (int p = idx[f]; p < end; p++) {
                c.f[n] = (int8_t)f; c.parent[n] = (int8_t)p;
                for (int s = 0; s < NSLOT; s++) c.pw[n][s] = c.pw[p][s];
                c.pw[n][f]++;
                n++;
            }
        }
        for (int f = 0; f < NSLOT; f++) idx[f] = nidx[f];
        end = n;
    }
    return c;
}
constexpr Canon CANON = make_canon();
static_assert(CANON.f[NCANON - 1] == 3 && CANON.pw[NCANON - 1][3] == 4 && CANON.pw[5][0] == 2 && CANON.pw[6][0] == 1 && CANON.pw[6][1] == 1,
              "canonical order");

struct TmDev {                       // one device block per model; the isotonic tables follow it
    double mean[NSLOT], scale[NSLOT];
    double coef[NCANON];
    double intercept, iso_xmin, iso_xmax;
    uint64_t used_lo, used_hi;       // canonical slots the model has a term in (bit c of lo for c < 64, bit c - 64 of hi)
    int32_t nf, degree, with_mean, with_std;
    int32_t plane[NSLOT];            // plane of each slot (0..3), -1 beyond nf
    int32_t iso_k, iso_nan;
    const double *iso_x, *iso_y;     // device copies (iso_k entries each)
};

__device__ __forceinline__ float tm_scale1(float x, double m, double s, int wm, int ws)
{
    if (wm) x = (float)__dsub_rn((double)x, m);
    if (ws) x = (float)__ddiv_rn((double)x, s);
    return x;
}
__device__ __forceinline__ double tm_scale1(double x, double m, double s, int wm, int ws)
{
    if (wm) x = __dsub_rn(x, m);
    if (ws) x = __ddiv_rn(x, s);
    return x;
}
__device__ __forceinline__ float tm_mul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ double tm_mul(double a, double b) { return __dmul_rn(a, b); }

// scaler + monomials in R (the input dtype) + float64 dot, term order
template <typename R>
__device__ __forceinline__ double tm_eval(const TmDev *__restrict__ p, R x0, R x1, R x2, R x3)
{
    R x[NSLOT] = {x0, x1, x2, x3};
    const int nf = p->nf, wm = p->with_mean, ws = p->with_std, D = p->degree;
#pragma unroll
    for (int s = 0; s < NSLOT; s++)
        if (s < nf) x[s] = tm_scale1(x[s], p->mean[s], p->scale[s], wm, ws);
        else x[s] = (R)0;
    R v[NCANON];
    v[0] = (R)1;
#pragma unroll
    for (int c = 1; c < DEG_START[2]; c++) v[c] = x[CANON.f[c]];
#pragma unroll
    for (int d = 2; d <= MAXDEG; d++) {
        if (D >= d) {
#pragma unroll
            for (int c = DEG_START[d]; c < DEG_START[d + 1]; c++) v[c] = tm_mul(x[CANON.f[c]], v[CANON.parent[c]]);
        }
    }
    const uint64_t lo = p->used_lo, hi = p->used_hi;
    double acc = 0.0;
#pragma unroll
    for (int d = 0; d <= MAXDEG; d++) {
        if (D >= d) {
#pragma unroll
            for (int c = DEG_START[d]; c < DEG_START[d + 1]; c++) {
                const bool used = c < 64 ? ((lo >> c) & 1) : ((hi >> (c - 64)) & 1);
                if (used) acc = __fma_rn(p->coef[c], (double)v[c], acc);
            }
        }
    }
    return __dadd_rn(acc, p->intercept);
}

// IsotonicRegression._transform -> interp1d -> np.interp for float64 tables (see the header); xt / yt in LDS or global memory
__device__ __forceinline__ double tm_iso(const TmDev *__restrict__ p, const double *xt, const double *yt, double y)
{
    const int K = p->iso_k;
    if (K == 0) return y;
    if (K == 1) return yt[0];
    if (!p->iso_nan) y = fmin(fmax(y, p->iso_xmin), p->iso_xmax);       // np.clip (a NaN stays NaN)
    if (!(y >= xt[0] && y <= xt[K - 1])) return __longlong_as_double(0x7ff8000000000000ll);
    if (y == xt[K - 1]) return yt[K - 1];
    int lo = 0, hi = K - 1;                                              // xt[lo] <= y < xt[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (xt[mid] <= y) lo = mid; else hi = mid;
    }
    const double xl = xt[lo], yl = yt[lo];
    if (xl == y) return yl;
    const double slope = __ddiv_rn(__dsub_rn(yt[lo + 1], yl), __dsub_rn(xt[lo + 1], xl));
    double r = __dadd_rn(__dmul_rn(slope, __dsub_rn(y, xl)), yl);
    if (isnan(r)) {                                                      // np.interp's retry from the right end, then the flat segment
        r = __dadd_rn(__dmul_rn(slope, __dsub_rn(y, xt[lo + 1])), yt[lo + 1]);
        if (isnan(r) && yl == yt[lo + 1]) r = yl;
    }
    return r;
}

__device__ __forceinline__ float tm_pick(const float pv[4], int s) { return s == 0 ? pv[0] : s == 1 ? pv[1] : s == 2 ? pv[2] : pv[3]; }

struct TmMapArgs {
    const TmDev *m[2];
    const uint8_t *mask[2];
    float *out[2];
    const float *plane[4];
    size_t P;
    int iso_off[2];                  // LDS offset (entries) of each model's table, -1 = global
    uint32_t plane_used;
};

template <int NM>
__global__ __launch_bounds__(256) void k_tmodel_map(const TmMapArgs a)
{
    extern __shared__ double tm_lds[];
    const double *xt[NM], *yt[NM];
    int lds_n = 0;
#pragma unroll
    for (int k = 0; k < NM; k++) {
        xt[k] = a.m[k]->iso_x; yt[k] = a.m[k]->iso_y;
        if (a.iso_off[k] >= 0) {
            const int K = a.m[k]->iso_k;
            double *lx = tm_lds + 2 * a.iso_off[k], *ly = lx + K;
            for (int j = threadIdx.x; j < K; j += blockDim.x) { lx[j] = xt[k][j]; ly[j] = yt[k][j]; }
            xt[k] = lx; yt[k] = ly;
            lds_n = 1;
        }
    }
    if (lds_n) __syncthreads();
    const float qnan = nanf32();
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.P; i += (size_t)gridDim.x * blockDim.x) {
        bool in[NM], any = false;
#pragma unroll
        for (int k = 0; k < NM; k++) { in[k] = a.mask[k][i] != 0; any |= in[k]; }
        float pv[4] = {0.f, 0.f, 0.f, 0.f};
        if (any) {
#pragma unroll
            for (int q = 0; q < 4; q++)
                if ((a.plane_used >> q) & 1) pv[q] = a.plane[q][i];
        }
#pragma unroll
        for (int k = 0; k < NM; k++) {
            float o = qnan;
            if (in[k]) {
                const TmDev *__restrict__ p = a.m[k];
                const int nf = p->nf;
                const float x0 = tm_pick(pv, p->plane[0]);
                const float x1 = nf > 1 ? tm_pick(pv, p->plane[1]) : 0.f;
                const float x2 = nf > 2 ? tm_pick(pv, p->plane[2]) : 0.f;
                const float x3 = nf > 3 ? tm_pick(pv, p->plane[3]) : 0.f;
                o = (float)tm_iso(p, xt[k], yt[k], tm_eval<float>(p, x0, x1, x2, x3));
            }
            a.out[k][i] = o;
        }
    }
}

template <typename R>
__global__ __launch_bounds__(256) void k_tmodel_rows(const TmDev *__restrict__ p, const R *__restrict__ rows, int64_t n, double *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int nf = p->nf;
    const R *r = rows + i * nf;
    const R x0 = r[0], x1 = nf > 1 ? r[1] : (R)0, x2 = nf > 2 ? r[2] : (R)0, x3 = nf > 3 ? r[3] : (R)0;
    out[i] = tm_iso(p, p->iso_x, p->iso_y, tm_eval<R>(p, x0, x1, x2, x3));
}

bool finite_all(const double *v, int n)
{
    for (int i = 0; i < n; i++)
        if (!std::isfinite(v[i])) return false;
    return true;
}

}  // namespace

struct vistaf_tmodel {
    TmDev host;          // host copy (iso_x / iso_y point into dev)
    char *dev = nullptr; // TmDev followed by the isotonic tables
    DeviceAllocs mem;
    int device = 0;
};

extern "C" {

int vistaf_tmodel_create(int n_features, const int32_t *feature_planes, const double *mean, const double *scale, int with_mean, int with_std,
                         int n_terms, const int32_t *powers, const double *coef, double intercept, int n_iso, const double *iso_x,
                         const double *iso_y, double iso_x_min, double iso_x_max, int iso_out_of_bounds, vistaf_tmodel **out)
{
    if (!out) return set_error(VISTAF_E_INVALID, "tmodel_create: null output handle");
    *out = nullptr;
    if (n_features < 1 || n_features > NSLOT) return set_error(VISTAF_E_INVALID, "tmodel_create: n_features must be 1..4");
    if (!feature_planes || !powers || !coef) return set_error(VISTAF_E_INVALID, "tmodel_create: null feature_planes, powers or coef");
    if ((with_mean && !mean) || (with_std && !scale)) return set_error(VISTAF_E_INVALID, "tmodel_create: null mean or scale");
    TmDev t;
    std::memset(&t, 0, sizeof(t));
    t.nf = n_features; t.with_mean = with_mean ? 1 : 0; t.with_std = with_std ? 1 : 0;
    for (int s = 0; s < NSLOT; s++) { t.plane[s] = -1; t.scale[s] = 1.0; }
    for (int s = 0; s < n_features; s++) {
        const int q = feature_planes[s];
        if (q < 0 || q > 3) return set_error(VISTAF_E_INVALID, "tmodel_create: feature plane must be 0..3 (L, a, b, gray)");
        for (int r = 0; r < s; r++)
            if (feature_planes[r] == q) return set_error(VISTAF_E_INVALID, "tmodel_create: a plane feeds two features");
        t.plane[s] = q;
        if (with_mean) {
            if (!std::isfinite(mean[s])) return set_error(VISTAF_E_INVALID, "tmodel_create: mean must be finite");
            t.mean[s] = mean[s];
        }
        if (with_std) {
            if (!std::isfinite(scale[s]) || !(scale[s] > 0.0)) return set_error(VISTAF_E_INVALID, "tmodel_create: scale must be finite and > 0");
            t.scale[s] = scale[s];
        }
    }
    if (n_terms < 1 || n_terms > NCANON) return set_error(VISTAF_E_INVALID, "tmodel_create: n_terms must be 1..70");
    if (!finite_all(coef, n_terms) || !std::isfinite(intercept)) return set_error(VISTAF_E_INVALID, "tmodel_create: coef and intercept must be finite");
    for (int r = 0; r < n_terms; r++) {
        int pw[NSLOT] = {0, 0, 0, 0}, deg = 0;
        for (int s = 0; s < n_features; s++) {
            const int e = powers[r * n_features + s];
            if (e < 0 || e > MAXDEG) return set_error(VISTAF_E_INVALID, "tmodel_create: powers must be 0..4");
            pw[s] = e; deg += e;
        }
        if (deg > MAXDEG) return set_error(VISTAF_E_INVALID, "tmodel_create: term degree above 4");
        int c = -1;
        for (int k = DEG_START[deg]; k < DEG_START[deg + 1] && c < 0; k++)
            if (CANON.pw[k][0] == pw[0] && CANON.pw[k][1] == pw[1] && CANON.pw[k][2] == pw[2] && CANON.pw[k][3] == pw[3]) c = k;
        uint64_t &word = c < 64 ? t.used_lo : t.used_hi;
        const uint64_t bit = 1ull << (c < 64 ? c : c - 64);
        if (word & bit) return set_error(VISTAF_E_INVALID, "tmodel_create: repeated powers row");
        word |= bit;
        t.coef[c] = coef[r];
        if (deg > t.degree) t.degree = deg;
    }
    t.intercept = intercept;
    if (n_iso < 0) return set_error(VISTAF_E_INVALID, "tmodel_create: n_iso must be >= 0");
    if (n_iso > 0) {
        if (!iso_x || !iso_y) return set_error(VISTAF_E_INVALID, "tmodel_create: null isotonic table");
        if (!finite_all(iso_x, n_iso) || !finite_all(iso_y, n_iso) || !std::isfinite(iso_x_min) || !std::isfinite(iso_x_max))
            return set_error(VISTAF_E_INVALID, "tmodel_create: isotonic table must be finite");
        for (int j = 1; j < n_iso; j++)
            if (!(iso_x[j] > iso_x[j - 1])) return set_error(VISTAF_E_INVALID, "tmodel_create: isotonic thresholds must be strictly increasing");
        if (iso_x_min > iso_x_max) return set_error(VISTAF_E_INVALID, "tmodel_create: isotonic x_min > x_max");
        if (iso_out_of_bounds != VISTAF_TMODEL_OOB_CLIP && iso_out_of_bounds != VISTAF_TMODEL_OOB_NAN)
            return set_error(VISTAF_E_INVALID, "tmodel_create: out_of_bounds must be 0 (clip) or 1 (nan)");
        t.iso_k = n_iso; t.iso_nan = iso_out_of_bounds; t.iso_xmin = iso_x_min; t.iso_xmax = iso_x_max;
    }
    Created<vistaf_tmodel> m(new vistaf_tmodel(), vistaf_tmodel_destroy);
    HIPCHK(hipGetDevice(&m->device));
    const size_t bytes = sizeof(TmDev) + 2 * sizeof(double) * (size_t)n_iso;
    TRY(m->mem.alloc(&m->dev, bytes));
    double *tab = (double *)(m->dev + sizeof(TmDev));
    t.iso_x = n_iso ? tab : nullptr;
    t.iso_y = n_iso ? tab + n_iso : nullptr;
    std::vector<char> blob(bytes);
    std::memcpy(blob.data(), &t, sizeof(TmDev));
    if (n_iso) {
        std::memcpy(blob.data() + sizeof(TmDev), iso_x, sizeof(double) * n_iso);
        std::memcpy(blob.data() + sizeof(TmDev) + sizeof(double) * n_iso, iso_y, sizeof(double) * n_iso);
    }
    HIPCHK(hipMemcpy(m->dev, blob.data(), bytes, hipMemcpyHostToDevice));
    m->host = t;
    *out = m.release();
    return 0;
}

void vistaf_tmodel_destroy(vistaf_tmodel *m)
{
    if (!m) return;
    m->mem.free_all();
    delete m;
}

int vistaf_tmodel_predict_maps(int n_models, const vistaf_tmodel *const *models, const uint8_t *const *d_masks, float *const *d_outs,
                               const float *const *d_planes, int64_t H, int64_t W, void *stream)
{
    if (n_models < 1 || n_models > 2) return set_error(VISTAF_E_INVALID, "tmodel_predict_maps: n_models must be 1 or 2");
    if (!models || !d_masks || !d_outs || !d_planes) return set_error(VISTAF_E_INVALID, "tmodel_predict_maps: null argument");
    if (H < 1 || W < 1) return set_error(VISTAF_E_INVALID, "tmodel_predict_maps: H and W must be >= 1");
    TmMapArgs a;
    std::memset(&a, 0, sizeof(a));
    a.P = (size_t)H * (size_t)W;
    int lds = 0;
    for (int k = 0; k < n_models; k++) {
        const vistaf_tmodel *m = models[k];
        if (!m || !d_masks[k] || !d_outs[k]) return set_error(VISTAF_E_INVALID, "tmodel_predict_maps: null model, mask or output");
        for (int s = 0; s < m->host.nf; s++) {
            const int q = m->host.plane[s];
            if (!d_planes[q]) return set_error(VISTAF_E_INVALID, "tmodel_predict_maps: a plane the model uses is NULL");
            a.plane_used |= 1u << q;
        }
        a.m[k] = (const TmDev *)m->dev; a.mask[k] = d_masks[k]; a.out[k] = d_outs[k];
        const int K = m->host.iso_k;
        a.iso_off[k] = -1;
        if (K > 1 && lds + K <= ISO_LDS_MAX) { a.iso_off[k] = lds; lds += K; }
    }
    for (int q = 0; q < 4; q++) a.plane[q] = d_planes[q];
    const int threads = 256;
    const size_t want = (a.P + threads - 1) / threads;
    const int blocks = (int)(want < 8192 ? want : 8192);              // grid-stride: LDS tables staged once per block
    const size_t shmem = sizeof(double) * 2 * (size_t)lds;
    hipStream_t st = (hipStream_t)stream;
    if (n_models == 1) hipLaunchKernelGGL(k_tmodel_map<1>, dim3(blocks), dim3(threads), shmem, st, a);
    else hipLaunchKernelGGL(k_tmodel_map<2>, dim3(blocks), dim3(threads), shmem, st, a);
    return launch_ok("tmodel_predict_maps");
}

int vistaf_tmodel_predict_rows(const vistaf_tmodel *m, const void *d_rows, int rows_dtype, int64_t n_rows, double *d_out, void *stream)
{
    if (!m) return set_error(VISTAF_E_INVALID, "tmodel_predict_rows: null model");
    if (rows_dtype != 0 && rows_dtype != 1) return set_error(VISTAF_E_INVALID, "tmodel_predict_rows: rows_dtype must be 0 (float32) or 1 (float64)");
    if (n_rows < 0) return set_error(VISTAF_E_INVALID, "tmodel_predict_rows: n_rows must be >= 0");
    if (n_rows == 0) return 0;
    if (!d_rows || !d_out) return set_error(VISTAF_E_INVALID, "tmodel_predict_rows: null rows or output");
    const int threads = 256;
    const int64_t blocks = (n_rows + threads - 1) / threads;
    if (blocks > 0x7fffffff) return set_error(VISTAF_E_INVALID, "tmodel_predict_rows: too many rows");
    hipStream_t st = (hipStream_t)stream;
    const TmDev *p = (const TmDev *)m->dev;
    if (rows_dtype == 0) hipLaunchKernelGGL(k_tmodel_rows<float>, dim3((unsigned)blocks), dim3(threads), 0, st, p, (const float *)d_rows, n_rows, d_out);
    else hipLaunchKernelGGL(k_tmodel_rows<double>, dim3((unsigned)blocks), dim3(threads), 0, st, p, (const double *)d_rows, n_rows, d_out);
    return launch_ok("tmodel_predict_rows");
}

}  // extern "C"
