// Pressure read-out (include/vistaf_pressure.h): the contact pressure map linear elasticity assigns to a depth plane, p^ = G(|k|) u^ for an
// elastic layer on a rigid base (or a half-space), and its per-contact and per-frame tables.  An extension, as the other read-outs: the
// reference has no counterpart.  The definition is in the header; tests/pressure_helpers.py restates it in NumPy.
//
// The transform sizes Ph x Pw are whatever h + pad, w + pad are, so both transforms are dense DFTs: four float64 contractions on the
// matrix cores (v_mfma_f64_16x16x4_f64) between twiddle tables built once on the host (long double angles, reduced exactly modulo the size).
//   k_pressure_clean   U: the depth plane with non-finite values, values <= eps and the frames of a bad status zeroed (float32, parked in
//                      the spectrum plane's memory until stage 2 overwrites it), so that stage 1 is the demodulation's own kernel.
//   stage 1            k_dft_fwd1_mfma (k_dft.hip, launch_dft_rows): real rows times the half table,  T [B h, Wh] = U [B h, w] . Ex [w, Wh].
//   k_pressure_fwd2    the column transform  Z [Ph, Wh] = Ey [Ph, h] . T [h, Wh]  per frame, the complex product as the real GEMM of
//                      cgemm_mfma.hpp (K = 2h), with G, the Hermitian weight and 1000 / (Ph Pw) in the epilogue: G is computed there from
//                      mm_per_px[b], which is per frame.
//   k_pressure_inv1    the conjugate column transform pruned to the h kept rows,  V [h, Wh] = Fy [h, Ph] . Z [Ph, Wh]  (K = 2 Ph).
//   k_pressure_inv2    the real inverse row transform  p [h, w] = V [h, 2 Wh] . Rx [2 Wh, w]  (V's rows as interleaved re / im, Rx = cos and
//                      -sin), with the float32 store.  A wave owns 16 rows x 64 columns, as in the complex stages.
//   k_pressure_rows    one workgroup per (frame, row) walks the contact's box (pixel i to thread i mod PR_NT); sums go lane -> wave over the
//                      DPP tree and wave -> workgroup in wave order.  The raw sums the frame row needs are parked in the reserved fields.
//   k_pressure_frame   one workgroup per frame: the whole-plane sums and peak, then thread 0 goes through the rows in ascending order, writes
//                      every row's force share and restores the reserved fields to NaN.
// Operands come straight from global memory / L2 as in k_dft.hip; staging them in LDS was not built or measured.  The workspace
// is three complex128 planes, T, Z and V, of which V lives in T's memory (stage 3 reads Z only).  No memset, no atomics: every element of
// every plane is written by exactly one lane before it is read, and every sum has an order fixed by the sizes and the launch geometry, so a
// frame gives the same bits alone, anywhere in a batch and on a second call.
#include <cmath>
#include <string>
#include <vector>

#include "../../include/vistaf_pressure.h"
#include "cgemm_mfma.hpp"
#include "contact_rows.hpp"
#include "host_util.hpp"

using namespace vf;

namespace vf {

struct PrBufs { double2 *rows, *spec; };      // T (and V) [maxB, h, Wh]; Z [maxB, Ph, Wh] (and U, float32 [maxB, h, w], before stage 2)

// base == nullptr sizes the buffer the first measure allocates, the same call with the pointer carves it
static PrBufs pressure_scratch(ScratchLayout &L, int maxB, int h, int w, int pad)
{
    const size_t Ph = (size_t)h + pad, Wh = ((size_t)w + pad) / 2 + 1;
    PrBufs bf;
    bf.rows = L.take<double2>((size_t)maxB * h * Wh, 256, "rows");
    bf.spec = L.take<double2>((size_t)maxB * Ph * Wh, 256, "spectrum");       // 16 Wh >= 4 w bytes per row: U fits
    return bf;
}

size_t pressure_scratch_bytes(int B, int h, int w, int pad, ScratchRec *rec)
{
    ScratchLayout L(nullptr, rec);
    pressure_scratch(L, B, h, w, pad);
    return L.bytes();
}

}  // namespace vf

namespace {

constexpr int PR_NT = 256;                               // threads of k_pressure_rows
constexpr int PR_FT = 1024;                              // threads of k_pressure_frame
constexpr int PR_PP = 13, PR_XP = 14, PR_YP = 15;        // where k_pressure_rows parks Pp, Xp, Yp for k_pressure_frame
constexpr double PR_TWO_PI = 6.283185307179586476925286766559;

struct PrModel { double E, Es, k, c0, t, g0; int halfspace; };     // c0 = 10 - 24 nu + 16 nu^2, g0 = G(0)

// header, step 2
__device__ inline double pr_gain(const PrModel &m, double q)
{
    if (q == 0.0) return m.g0;
    if (m.halfspace) return m.Es * q / 2.0;
    const double x = q * m.t, e = exp(-2.0 * x);
    const double S = (m.k * (1.0 - e * e) - 4.0 * x * e) / (m.k * (1.0 + e * e) + (4.0 * x * x + m.c0) * e);
    return m.Es * q / (2.0 * S);
}

__global__ __launch_bounds__(256) void k_pressure_clean(const float *__restrict__ depth, const int32_t *__restrict__ status, float eps, unsigned P,
                                                        float *__restrict__ U)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= P) return;
    const size_t b = blockIdx.y;
    const float d = depth[b * P + i];
    const bool ok = !status || status[b] == 0;
    U[b * P + i] = (ok && finitef(d) && d > eps) ? d : 0.0f;
}

__global__ __launch_bounds__(256) void k_pressure_fwd2(const double2 *__restrict__ T, const double2 *__restrict__ Ey, const double *__restrict__ mm_per_px,
                                                       const int32_t *__restrict__ status, PrModel m, double2 *__restrict__ Z, int h, int Ph, int Pw,
                                                       int Wh)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int x0 = blockIdx.x * 64, y0 = (blockIdx.y * 4 + wid) * 16;
    const size_t b = blockIdx.z;
    if (y0 >= Ph) return;
    const int r = lane & 15, kk = lane >> 4;
    v4f64 cre[4], cim[4];
    cgemm16x64_mfma((const double *)Ey, h, h, T + b * (size_t)h * Wh, Wh, Wh, min(y0 + r, Ph - 1), x0, lane, cre, cim);
    const bool ok = !status || status[b] == 0;
    const double s = ok ? mm_per_px[b] : 1.0, norm = 1000.0 / ((double)Ph * (double)Pw);
    double2 *Zb = Z + b * (size_t)Ph * Wh;
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int c = x0 + 16 * t + r;
        if (c >= Wh) continue;
        const double fx = (double)c / (double)Pw, wgt = (c == 0 || 2 * c == Pw) ? 1.0 : 2.0;
#pragma unroll
        for (int qd = 0; qd < 4; qd++) {
            const int a = y0 + kk + 4 * qd;
            if (a >= Ph) continue;
            const double fy = (double)(a <= Ph / 2 ? a : a - Ph) / (double)Ph;
            const double q = PR_TWO_PI * sqrt(fx * fx + fy * fy) / s;
            const double g = pr_gain(m, q) * (wgt * norm);
            Zb[(size_t)a * Wh + c] = ok ? make_double2(cre[t][qd] * g, cim[t][qd] * g) : make_double2(0.0, 0.0);
        }
    }
}

__global__ __launch_bounds__(256) void k_pressure_inv1(const double2 *__restrict__ Z, const double2 *__restrict__ Fy, double2 *__restrict__ V, int h, int Ph,
                                                       int Wh)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int x0 = blockIdx.x * 64, y0 = (blockIdx.y * 4 + wid) * 16;
    const size_t b = blockIdx.z;
    if (y0 >= h) return;
    const int r = lane & 15, kk = lane >> 4;
    v4f64 cre[4], cim[4];
    cgemm16x64_mfma((const double *)Fy, Ph, Ph, Z + b * (size_t)Ph * Wh, Wh, Wh, min(y0 + r, h - 1), x0, lane, cre, cim);
    double2 *Vb = V + b * (size_t)h * Wh;
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int c = x0 + 16 * t + r;
        if (c >= Wh) continue;
#pragma unroll
        for (int qd = 0; qd < 4; qd++) {
            const int y = y0 + kk + 4 * qd;
            if (y < h) Vb[(size_t)y * Wh + c] = make_double2(cre[t][qd], cim[t][qd]);
        }
    }
}

// p[y][x] = sum_k V[y][k] * Rx[k][x], k = 0..K2-1 (K2 = 2 Wh: re, im of column 0, re, im of column 1, ...); A[i = lane & 15][k = lane >> 4],
// B[k = lane >> 4][j = lane & 15], D[row = (lane >> 4) + 4 reg][col = lane & 15]
__global__ __launch_bounds__(256) void k_pressure_inv2(const double *__restrict__ V, const double *__restrict__ Rx, float *__restrict__ p, int h, int w, int K2)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int x0 = blockIdx.x * 64, y0 = (blockIdx.y * 4 + wid) * 16;
    const size_t b = blockIdx.z;
    if (y0 >= h) return;
    const int r = lane & 15, kk = lane >> 4;
    const double *Va = V + (b * (size_t)h + (size_t)min(y0 + r, h - 1)) * K2;
    v4f64 acc[4];
    int xc[4];
#pragma unroll
    for (int t = 0; t < 4; t++) { acc[t] = (v4f64){0.0, 0.0, 0.0, 0.0}; xc[t] = min(x0 + 16 * t + r, w - 1); }
    for (int k0 = 0; k0 < K2; k0 += 4) {
        const int k = k0 + kk;
        const bool in = k < K2;
        const int kq = in ? k : 0;
        const double a = in ? Va[kq] : 0.0;
        double bv[4];
#pragma unroll
        for (int t = 0; t < 4; t++) bv[t] = Rx[(size_t)kq * w + xc[t]];
#pragma unroll
        for (int t = 0; t < 4; t++) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, in ? bv[t] : 0.0, acc[t], 0, 0, 0);
    }
    float *pb = p + b * (size_t)h * w;
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int x = x0 + 16 * t + r;
        if (x >= w) continue;
#pragma unroll
        for (int qd = 0; qd < 4; qd++) {
            const int y = y0 + kk + 4 * qd;
            if (y < h) pb[(size_t)y * w + x] = (float)acc[t][qd];
        }
    }
}

__global__ __launch_bounds__(PR_NT) void k_pressure_rows(const float *__restrict__ p, const int8_t *__restrict__ index, const double *__restrict__ contacts,
                                                         const int32_t *__restrict__ count, const double *__restrict__ mm_per_px,
                                                         const int32_t *__restrict__ status, int h, int w, int K, double *__restrict__ rows)
{
    __shared__ double sd[16];
    __shared__ unsigned long long s64[16];
    const int k = blockIdx.x, tid = threadIdx.x;
    const size_t b = blockIdx.y;
    double *row = rows + (b * (size_t)K + k) * VISTAF_NPRESSURE;
    const bool ok = !status || status[b] == 0;
    if (nan_row(k >= clamp_count(ok ? count[b] : 0, K), row, VISTAF_NPRESSURE)) return;
    const ContactBox box(contacts + (b * (size_t)K + k) * VISTAF_NCONTACT, h, w);
    const float *pf = p + b * (size_t)h * w;
    const int8_t *ix = index + b * (size_t)h * w;
    double Pp = 0.0, Pn = 0.0, Xp = 0.0, Yp = 0.0, Pe = 0.0;
    unsigned long long n = 0, Sx = 0, Sy = 0, key = 0;
    BoxWalk<PR_NT>(box, tid).each([&](int x, int y) {
        const size_t o = (size_t)y * w + x;
        if (ix[o] != k) return;
        const float v32 = pf[o];
        const double v = (double)v32, vp = v > 0.0 ? v : 0.0;
        n++; Sx += (unsigned)x; Sy += (unsigned)y;
        Pp += vp;
        Pn += -v > 0.0 ? -v : 0.0;
        Xp += (double)x * vp;
        Yp += (double)y * vp;
        const bool edge = x == 0 || y == 0 || x == w - 1 || y == h - 1 || ix[o - 1] != k || ix[o + 1] != k || ix[o - w] != k || ix[o + w] != k;
        if (edge) Pe += vp;
        const unsigned long long ky = argmax_key(v32, (unsigned)o);
        key = ky > key ? ky : key;
    });
    Pp = block_sum<double>(Pp, sd); Pn = block_sum<double>(Pn, sd); Xp = block_sum<double>(Xp, sd); Yp = block_sum<double>(Yp, sd);
    Pe = block_sum<double>(Pe, sd);
    n = block_sum<unsigned long long>(n, s64); Sx = block_sum<unsigned long long>(Sx, s64); Sy = block_sum<unsigned long long>(Sy, s64);
    key = block_max_u64(key, s64);
    if (tid != 0) return;
    const double s = mm_per_px[b], px = s * s, nn = (double)n;
    const double mean = n ? (Pp - Pn) / nn : nan64(), peak = n ? (double)key2f((uint32_t)(key >> 32)) : nan64();
    const double cx = Pp != 0.0 ? Xp / Pp : nan64(), cy = Pp != 0.0 ? Yp / Pp : nan64();
    row[VISTAF_PRESSURE_PIXELS] = nn;
    row[VISTAF_PRESSURE_FORCE_MODEL_N] = 1e-3 * px * Pp;
    row[VISTAF_PRESSURE_TENSILE_MODEL_N] = 1e-3 * px * Pn;
    row[VISTAF_PRESSURE_FORCE_N] = nan64();
    row[VISTAF_PRESSURE_MEAN_KPA] = mean;
    row[VISTAF_PRESSURE_PEAK_KPA] = peak;
    row[VISTAF_PRESSURE_PEAK_INDEX] = n ? (double)(0xffffffffu - (uint32_t)key) : nan64();
    row[VISTAF_PRESSURE_COP_X] = cx;
    row[VISTAF_PRESSURE_COP_Y] = cy;
    row[VISTAF_PRESSURE_OFFSET_X_MM] = n ? (cx - (double)Sx / nn) * s : nan64();
    row[VISTAF_PRESSURE_OFFSET_Y_MM] = n ? (cy - (double)Sy / nn) * s : nan64();
    row[VISTAF_PRESSURE_PEAK_OVER_MEAN] = (n && mean > 0.0) ? peak / mean : nan64();
    row[VISTAF_PRESSURE_EDGE_SHARE] = Pp != 0.0 ? Pe / Pp : nan64();
    row[PR_PP] = Pp;
    row[PR_XP] = Xp;
    row[PR_YP] = Yp;
}

// index / count / rows null together: the plane and the frame row only
__global__ __launch_bounds__(PR_FT) void k_pressure_frame(const float *__restrict__ p, const int8_t *__restrict__ index, const int32_t *__restrict__ count,
                                                          const double *__restrict__ mm_per_px, const double *__restrict__ force,
                                                          const int32_t *__restrict__ status, double E, unsigned P, int K, double *__restrict__ rows,
                                                          double *__restrict__ frame)
{
    __shared__ double sd[16];
    __shared__ unsigned long long s64[16];
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    double *fr = frame + b * VISTAF_NPRESSUREFRAME;
    const int st = status ? status[b] : 0;
    if (st != 0) {                                      // the contact rows are NaN already
        if (tid < VISTAF_NPRESSUREFRAME) fr[tid] = tid == VISTAF_PRESSUREFRAME_STATUS ? (double)st : nan64();
        return;
    }
    const int kk = clamp_count(index ? count[b] : 0, K);
    const float *pf = p + b * (size_t)P;
    const int8_t *ix = index ? index + b * (size_t)P : nullptr;
    double Tn = 0.0, Out = 0.0;
    unsigned long long key = 0;
    for (unsigned i = tid; i < P; i += PR_FT) {
        const float v32 = pf[i];
        const double v = (double)v32;
        Tn += -v > 0.0 ? -v : 0.0;
        const int id = ix ? (int)ix[i] : -1;
        if (id < 0 || id >= kk) Out += fabs(v);
        const unsigned long long ky = argmax_key(v32, i);
        key = ky > key ? ky : key;
    }
    Tn = block_sum<double>(Tn, sd);
    Out = block_sum<double>(Out, sd);
    key = block_max_u64(key, s64);
    if (tid != 0) return;
    const double s = mm_per_px[b], px = s * s, F = force ? force[b] : nan64();
    double fm = 0.0, sp = 0.0, sx = 0.0, sy = 0.0;
    double *rw = rows ? rows + b * (size_t)K * VISTAF_NPRESSURE : nullptr;
    for (int k = 0; k < kk; k++) {
        const double *row = rw + (size_t)k * VISTAF_NPRESSURE;
        fm += row[VISTAF_PRESSURE_FORCE_MODEL_N]; sp += row[PR_PP]; sx += row[PR_XP]; sy += row[PR_YP];
    }
    for (int k = 0; k < kk; k++) {
        double *row = rw + (size_t)k * VISTAF_NPRESSURE;
        row[VISTAF_PRESSURE_FORCE_N] = !force ? nan64() : (fm == 0.0 ? 0.0 : F * (row[VISTAF_PRESSURE_FORCE_MODEL_N] / fm));
        row[PR_PP] = nan64(); row[PR_XP] = nan64(); row[PR_YP] = nan64();
    }
    const unsigned pi = 0xffffffffu - (uint32_t)key;    // P >= 1: a pixel was seen
    const int pid = ix ? (int)ix[pi] : -1;
    const double scale = (force && fm > 0.0) ? F / fm : nan64();
    fr[VISTAF_PRESSUREFRAME_CONTACTS] = (double)kk;
    fr[VISTAF_PRESSUREFRAME_FORCE_MODEL_N] = fm;
    fr[VISTAF_PRESSUREFRAME_TENSILE_MODEL_N] = 1e-3 * px * Tn;
    fr[VISTAF_PRESSUREFRAME_OUTSIDE_MODEL_N] = 1e-3 * px * Out;
    fr[VISTAF_PRESSUREFRAME_SCALE] = scale;
    fr[VISTAF_PRESSUREFRAME_E_EFFECTIVE_MPA] = scale * E;
    fr[VISTAF_PRESSUREFRAME_PEAK_KPA] = (double)key2f((uint32_t)(key >> 32));
    fr[VISTAF_PRESSUREFRAME_PEAK_INDEX] = (double)pi;
    fr[VISTAF_PRESSUREFRAME_PEAK_ROW] = (pid >= 0 && pid < kk) ? (double)pid : -1.0;
    fr[VISTAF_PRESSUREFRAME_COP_X] = sp != 0.0 ? sx / sp : nan64();
    fr[VISTAF_PRESSUREFRAME_COP_Y] = sp != 0.0 ? sy / sp : nan64();
    fr[VISTAF_PRESSUREFRAME_STATUS] = 0.0;
}

// exp(sign * 2 pi i * num / den), the angle reduced exactly and evaluated in long double
inline double2 pr_twiddle(long long num, int den, int sign)
{
    const long double ang = 2.0L * 3.14159265358979323846264338327950288L * (long double)(num % den) / (long double)den;
    return make_double2((double)cosl(ang), (double)(sign * sinl(ang)));
}

}  // namespace

struct vistaf_pressure_handle {
    int h = 0, w = 0, maxB = 0, K = 0, pad = 0, Ph = 0, Pw = 0, Wh = 0;
    PrModel m = {};
    std::vector<double2> Ex, Ey, Fy;                    // [w][Wh] forward, [Ph][h] forward, [h][Ph] inverse
    std::vector<double> Rx;                             // [2 Wh][w]: cos, -sin
    bool uploaded = false;
    double2 *d_Ex = nullptr, *d_Ey = nullptr, *d_Fy = nullptr;
    double *d_Rx = nullptr;
    void *buf = nullptr;
    PrBufs bf = {};
    DeviceAllocs mem;
};

static int pressure_upload(vistaf_pressure_handle *pr)
{
    if (pr->uploaded) return 0;
    int rc = pr->mem.upload(&pr->d_Ex, pr->Ex);
    if (!rc) rc = pr->mem.upload(&pr->d_Ey, pr->Ey);
    if (!rc) rc = pr->mem.upload(&pr->d_Fy, pr->Fy);
    if (!rc) rc = pr->mem.upload(&pr->d_Rx, pr->Rx);
    if (!rc) rc = ensure_carved(pr->mem, pr->buf, &pr->bf, [&](ScratchLayout &L) { return pressure_scratch(L, pr->maxB, pr->h, pr->w, pr->pad); });
    if (rc) pr->mem.free_all();                         // the next measure starts over
    pr->uploaded = !rc;
    return rc;
}

extern "C" {

void vistaf_pressure_destroy(vistaf_pressure_handle *pr)
{
    if (!pr) return;
    pr->mem.free_all();
    delete pr;
}

int vistaf_pressure_create(int h, int w, int max_batch, int max_contacts, int pad_px, double E_mpa, double nu, double thickness_mm,
                           vistaf_pressure_handle **out)
{
    if (!out) return set_error(VISTAF_E_INVALID, "null argument: out");
    *out = nullptr;
    if (h < 1 || w < 1 || h > 4096 || w > 4096) return set_error(VISTAF_E_INVALID, "frame size must be 1..4096 each way");
    if (max_batch < 1 || max_batch > 65535) return set_error(VISTAF_E_INVALID, "max_batch must be 1..65535");
    if (max_contacts < 0 || max_contacts > VISTAF_MAX_CONTACTS) return set_error(VISTAF_E_INVALID, "max_contacts must be 0..64");
    if (pad_px < 0 || pad_px > 4096) return set_error(VISTAF_E_INVALID, "pad_px must be 0..4096");
    if (!(E_mpa > 0.0) || !std::isfinite(E_mpa)) return set_error(VISTAF_E_INVALID, "E_mpa must be finite and > 0");
    if (!(nu >= 0.0 && nu <= 0.49)) return set_error(VISTAF_E_INVALID, "nu must be 0..0.49");
    if (!(thickness_mm > 0.0)) return set_error(VISTAF_E_INVALID, "thickness_mm must be > 0 or +inf");
    Created<vistaf_pressure_handle> pr(new vistaf_pressure_handle(), vistaf_pressure_destroy);
    pr->h = h; pr->w = w; pr->maxB = max_batch; pr->K = max_contacts; pr->pad = pad_px;
    const int Ph = pr->Ph = h + pad_px, Pw = pr->Pw = w + pad_px, Wh = pr->Wh = Pw / 2 + 1;
    PrModel &m = pr->m;
    m.E = E_mpa;
    m.Es = E_mpa / (1.0 - nu * nu);
    m.k = 3.0 - 4.0 * nu;
    m.c0 = 10.0 - 24.0 * nu + 16.0 * nu * nu;
    m.halfspace = std::isinf(thickness_mm) ? 1 : 0;
    m.t = thickness_mm;
    m.g0 = m.halfspace ? 0.0 : E_mpa * (1.0 - nu) / ((1.0 + nu) * (1.0 - 2.0 * nu) * thickness_mm);
    pr->Ex.resize((size_t)w * Wh);
    for (int x = 0; x < w; x++)
        for (int c = 0; c < Wh; c++) pr->Ex[(size_t)x * Wh + c] = pr_twiddle((long long)c * x, Pw, -1);
    pr->Ey.resize((size_t)Ph * h);
    pr->Fy.resize((size_t)h * Ph);
    for (int a = 0; a < Ph; a++)
        for (int y = 0; y < h; y++) {
            const double2 e = pr_twiddle((long long)a * y, Ph, -1);
            pr->Ey[(size_t)a * h + y] = e;
            pr->Fy[(size_t)y * Ph + a] = make_double2(e.x, -e.y);
        }
    pr->Rx.resize((size_t)2 * Wh * w);
    for (int c = 0; c < Wh; c++)
        for (int x = 0; x < w; x++) {
            const double2 e = pr_twiddle((long long)c * x, Pw, -1);        // cos, -sin
            pr->Rx[(size_t)(2 * c) * w + x] = e.x;
            pr->Rx[(size_t)(2 * c + 1) * w + x] = e.y;
        }
    *out = pr.release();
    return 0;
}

int vistaf_pressure_measure(vistaf_pressure_handle *pr, const float *d_depth_mm, const int8_t *d_contact_index, const double *d_contacts,
                            const int32_t *d_count, const double *d_mm_per_px, const double *d_frame_force_N, const int32_t *d_status,
                            float depth_eps_mm, int B, float *d_pressure_kpa, double *d_rows, double *d_frame, void *stream)
{
    if (!pr) return set_error(VISTAF_E_INVALID, "null argument: handle");
    if (!d_depth_mm) return set_error(VISTAF_E_INVALID, "null argument: depth_mm");
    if (!d_mm_per_px) return set_error(VISTAF_E_INVALID, "null argument: mm_per_px");
    if (!d_pressure_kpa) return set_error(VISTAF_E_INVALID, "null argument: pressure_kpa");
    if (!d_frame) return set_error(VISTAF_E_INVALID, "null argument: frame");
    const int given = (d_contact_index ? 1 : 0) + (d_contacts ? 1 : 0) + (d_count ? 1 : 0) + (d_rows ? 1 : 0);
    if (given != 0 && given != 4) return set_error(VISTAF_E_INVALID, "contact_index, contacts, count and rows must be given or NULL together");
    if (given && pr->K == 0) return set_error(VISTAF_E_INVALID, "a read-out of max_contacts 0 takes no contact arguments");
    if (!given && pr->K != 0) return set_error(VISTAF_E_INVALID, "a read-out of max_contacts > 0 needs the contact arguments");
    if (B < 1 || B > pr->maxB) return set_error(VISTAF_E_INVALID, "batch must be 1..max_batch");
    if (!std::isfinite(depth_eps_mm)) return set_error(VISTAF_E_INVALID, "depth_eps_mm must be finite");
    if (((uintptr_t)d_depth_mm & 3u) || ((uintptr_t)d_count & 3u) || ((uintptr_t)d_status & 3u) || ((uintptr_t)d_pressure_kpa & 3u))
        return set_error(VISTAF_E_INVALID, "depth_mm, count, status and pressure_kpa must be 4-byte aligned");
    if (((uintptr_t)d_contacts & 7u) || ((uintptr_t)d_mm_per_px & 7u) || ((uintptr_t)d_frame_force_N & 7u) || ((uintptr_t)d_rows & 7u) ||
        ((uintptr_t)d_frame & 7u))
        return set_error(VISTAF_E_INVALID, "contacts, mm_per_px, frame_force_N, rows and frame must be 8-byte aligned");
    if (const int rc = pressure_upload(pr)) return rc;
    const hipStream_t st = (hipStream_t)stream;
    const int h = pr->h, w = pr->w, Ph = pr->Ph, Pw = pr->Pw, Wh = pr->Wh;
    const unsigned P = (unsigned)h * (unsigned)w;
    float *U = (float *)pr->bf.spec;
    double2 *T = pr->bf.rows, *Z = pr->bf.spec, *V = pr->bf.rows;
    hipLaunchKernelGGL(k_pressure_clean, dim3((P + 255u) / 256u, (unsigned)B), dim3(256), 0, st, d_depth_mm, d_status, depth_eps_mm, P, U);
    launch_dft_rows(U, nullptr, pr->d_Ex, T, B, h, w, Wh, st);
    hipLaunchKernelGGL(k_pressure_fwd2, dim3((Wh + 63) / 64, (Ph + 63) / 64, (unsigned)B), dim3(256), 0, st, (const double2 *)T, (const double2 *)pr->d_Ey,
                       d_mm_per_px, d_status, pr->m, Z, h, Ph, Pw, Wh);
    hipLaunchKernelGGL(k_pressure_inv1, dim3((Wh + 63) / 64, (h + 63) / 64, (unsigned)B), dim3(256), 0, st, (const double2 *)Z, (const double2 *)pr->d_Fy, V, h,
                       Ph, Wh);
    hipLaunchKernelGGL(k_pressure_inv2, dim3((w + 63) / 64, (h + 63) / 64, (unsigned)B), dim3(256), 0, st, (const double *)V, (const double *)pr->d_Rx,
                       d_pressure_kpa, h, w, 2 * Wh);
    if (given)
        hipLaunchKernelGGL(k_pressure_rows, dim3((unsigned)pr->K, (unsigned)B), dim3(PR_NT), 0, st, (const float *)d_pressure_kpa, d_contact_index, d_contacts,
                           d_count, d_mm_per_px, d_status, h, w, pr->K, d_rows);
    hipLaunchKernelGGL(k_pressure_frame, dim3((unsigned)B), dim3(PR_FT), 0, st, (const float *)d_pressure_kpa, d_contact_index, d_count, d_mm_per_px,
                       d_frame_force_N, d_status, pr->m.E, P, pr->K, d_rows, d_frame);
    return launch_ok("k_pressure_*");
}

}  // extern "C"
