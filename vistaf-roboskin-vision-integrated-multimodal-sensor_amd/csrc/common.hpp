// Shared device helpers for the gfx950 FTP kernels (wave = 64 lanes).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

namespace vf {

constexpr int WAVE = 64;

// cv::borderInterpolate BORDER_REFLECT_101
__host__ __device__ inline int reflect101(int p, int len)
{
    if (len == 1) return 0;
    while (p < 0 || p >= len) p = p < 0 ? -p : 2 * (len - 1) - p;
    return p;
}
// cv::borderInterpolate BORDER_REFLECT
__host__ __device__ inline int reflect_edge(int p, int len)
{
    if (len == 1) return 0;
    while (p < 0 || p >= len) p = p < 0 ? -p - 1 : 2 * len - 1 - p;
    return p;
}

// order-preserving float <-> uint32 (ascending): bit operations, the same on the host
__host__ __device__ inline uint32_t f2key(float f)
{
    uint32_t u = __builtin_bit_cast(uint32_t, f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline float key2f(uint32_t k)
{
    uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    return __builtin_bit_cast(float, u);
}
// the same with -0.0 on +0.0's key: the order of ==, under which the two zeros are one value (key2f gives +0.0 back for either).  For keys
// that carry an index behind the value: a tie between the two zeros is then decided by the index, as NumPy's argmax / argmin decide it
__host__ __device__ inline uint32_t f2key_eq(float f)
{
    const uint32_t u = __builtin_bit_cast(uint32_t, f);
    return (u << 1) == 0 ? 0x80000000u : f2key(f);
}
// arg-max key: the larger value wins, among equal values (-0.0 == +0.0 among them) the smaller index
__device__ inline unsigned long long argmax_key(float v, unsigned i) { return ((unsigned long long)f2key_eq(v) << 32) | (0xffffffffu - i); }
// arg-min key: the smaller value wins, among equal values the smaller index; ~0 is above every key
__device__ inline unsigned long long argmin_key(float v, unsigned i) { return ((unsigned long long)f2key_eq(v) << 32) | i; }

__device__ inline bool finitef(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ inline bool finitef(double v) { return ((unsigned long long)__double_as_longlong(v) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }
// the quiet NaN every kernel writes (NumPy's np.nan bits)
__host__ __device__ inline float nanf32() { return __builtin_bit_cast(float, 0x7fc00000u); }
__device__ inline double nan64() { return __longlong_as_double(0x7ff8000000000000ll); }

// One correctly rounded float32 operation that is never contracted into an fma, for rules a host program calls too: the __f*_rn intrinsic on
// the device, the plain operator on the host (the same operation under the -ffp-contract=off the library and every host check are built with)
#ifdef __HIP_DEVICE_COMPILE__
#define VF_RN(dev, host) return dev
#else
#define VF_RN(dev, host) return host
#endif
__host__ __device__ inline float rn_add(float a, float b) { VF_RN(__fadd_rn(a, b), a + b); }
__host__ __device__ inline float rn_sub(float a, float b) { VF_RN(__fsub_rn(a, b), a - b); }
__host__ __device__ inline float rn_mul(float a, float b) { VF_RN(__fmul_rn(a, b), a * b); }
__host__ __device__ inline float rn_div(float a, float b) { VF_RN(__fdiv_rn(a, b), a / b); }
#undef VF_RN

// ---- wave-level reductions on the DPP network (no LDS round trips): quad xor 1, quad xor 2, row_half_mirror,
// row_mirror leave the row result in every lane of a 16-lane row; row_bcast15 / row_bcast31 then carry it
// across rows so that lane 63 holds the wave result, which is broadcast back through an SGPR.
template <int CTRL, int RM>
__device__ inline uint32_t dppmov(uint32_t old, uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, CTRL, RM, 0xf, false); }
template <int CTRL, int RM>
__device__ inline unsigned long long dppmov(unsigned long long old, unsigned long long v)
{
    uint32_t lo = dppmov<CTRL, RM>((uint32_t)old, (uint32_t)v), hi = dppmov<CTRL, RM>((uint32_t)(old >> 32), (uint32_t)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}
__device__ inline uint32_t bcast63(uint32_t v) { return (uint32_t)__builtin_amdgcn_readlane((int)v, 63); }
__device__ inline unsigned long long bcast63(unsigned long long v)
{
    return ((unsigned long long)bcast63((uint32_t)(v >> 32)) << 32) | bcast63((uint32_t)v);
}
// lane l's 64-bit value in every lane (l wave-uniform)
__device__ inline unsigned long long readlane64(unsigned long long v, int l)
{
    return ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(v >> 32), l) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)v, l);
}
// relaxed atomic load / store at memory scope SCOPE (__HIP_MEMORY_SCOPE_WORKGROUP, _AGENT): a value another wave may write, read past the
// caches that scope does not share.  The scope is spelled at every call site
template <int SCOPE, typename T>
__device__ inline T ld_relaxed(const T *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, SCOPE); }
template <int SCOPE, typename T>
__device__ inline void st_relaxed(T *p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, SCOPE); }
// RAW = bits of the value (uint32_t or unsigned long long); op combines two RAW words; id = bits of op's identity
template <typename RAW, typename F>
__device__ inline RAW wave_reduce_raw(RAW v, RAW id, F op)
{
    v = op(v, dppmov<0xB1, 0xf>(v, v));
    v = op(v, dppmov<0x4E, 0xf>(v, v));
    v = op(v, dppmov<0x141, 0xf>(v, v));
    v = op(v, dppmov<0x140, 0xf>(v, v));
    v = op(v, dppmov<0x142, 0xa>(id, v));
    v = op(v, dppmov<0x143, 0xc>(id, v));
    return bcast63(v);
}
__device__ inline uint32_t wave_sum(uint32_t v) { return wave_reduce_raw<uint32_t>(v, 0u, [](uint32_t a, uint32_t b) { return a + b; }); }
__device__ inline int wave_sum(int v) { return (int)wave_sum((uint32_t)v); }
__device__ inline unsigned long long wave_sum(unsigned long long v)
{
    return wave_reduce_raw<unsigned long long>(v, 0ull, [](unsigned long long a, unsigned long long b) { return a + b; });
}
__device__ inline float wave_sum(float v)
{
    return __uint_as_float(wave_reduce_raw<uint32_t>(__float_as_uint(v), 0u,
                                                     [](uint32_t a, uint32_t b) { return __float_as_uint(__uint_as_float(a) + __uint_as_float(b)); }));
}
__device__ inline double wave_sum(double v)
{
    return __longlong_as_double((long long)wave_reduce_raw<unsigned long long>(
        (unsigned long long)__double_as_longlong(v), 0ull, [](unsigned long long a, unsigned long long b) {
            return (unsigned long long)__double_as_longlong(__longlong_as_double((long long)a) + __longlong_as_double((long long)b));
        }));
}
__device__ inline uint32_t wave_max_u32(uint32_t v) { return wave_reduce_raw<uint32_t>(v, 0u, [](uint32_t a, uint32_t b) { return b > a ? b : a; }); }
__device__ inline unsigned long long wave_max_u64(unsigned long long v)
{
    return wave_reduce_raw<unsigned long long>(v, 0ull, [](unsigned long long a, unsigned long long b) { return b > a ? b : a; });
}
__device__ inline unsigned long long wave_min_u64(unsigned long long v)
{
    return wave_reduce_raw<unsigned long long>(v, ~0ull, [](unsigned long long a, unsigned long long b) { return b < a ? b : a; });
}

// ---- wave-level inclusive scans on the same network: row_shr 1/2/4/8 scan each 16-lane row (bound_ctrl: lanes without a source read 0),
// row_bcast15 / row_bcast31 then add the totals of the rows below.  0 must be op's identity (sums; maxima of values >= 0).
template <typename F>
__device__ inline uint32_t wave_scan_raw(uint32_t v, F op)
{
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true));
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true));
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true));
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true));
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false));
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false));
    return v;
}
__device__ inline uint32_t wave_scan_add(uint32_t v) { return wave_scan_raw(v, [](uint32_t a, uint32_t b) { return a + b; }); }
__device__ inline int wave_scan_add(int v) { return (int)wave_scan_add((uint32_t)v); }
__device__ inline uint32_t wave_scan_max(uint32_t v) { return wave_scan_raw(v, [](uint32_t a, uint32_t b) { return b > a ? b : a; }); }
// The same scan for a signed value whose identity is not 0 (a maximum of values that may be negative, a minimum): lanes without a source
// read `identity` (bound_ctrl off), in the row steps as in the broadcasts.
template <typename F>
__device__ inline int wave_scan_ident(int v, int identity, F op)
{
    v = op(v, __builtin_amdgcn_update_dpp(identity, v, 0x111, 0xf, 0xf, false));
    v = op(v, __builtin_amdgcn_update_dpp(identity, v, 0x112, 0xf, 0xf, false));
    v = op(v, __builtin_amdgcn_update_dpp(identity, v, 0x114, 0xf, 0xf, false));
    v = op(v, __builtin_amdgcn_update_dpp(identity, v, 0x118, 0xf, 0xf, false));
    v = op(v, __builtin_amdgcn_update_dpp(identity, v, 0x142, 0xa, 0xf, false));
    v = op(v, __builtin_amdgcn_update_dpp(identity, v, 0x143, 0xc, 0xf, false));
    return v;
}
// inclusive prefix maximum / minimum over lanes 0..l; id: a value no input exceeds / falls below
__device__ inline int wave_scan_max_i32(int v, int id) { return wave_scan_ident(v, id, [](int a, int b) { return b > a ? b : a; }); }
__device__ inline int wave_scan_min_i32(int v, int id) { return wave_scan_ident(v, id, [](int a, int b) { return b < a ? b : a; }); }
// inclusive suffix minimum over lanes l..63: mirror the lanes (ds_bpermute with 63 - lane), prefix minimum, mirror back
__device__ inline int wave_suffix_min_i32(int v, int id, int lane)
{
    v = __builtin_amdgcn_ds_bpermute((63 - lane) << 2, v);
    v = wave_scan_min_i32(v, id);
    return __builtin_amdgcn_ds_bpermute((63 - lane) << 2, v);
}
// exclusive prefix sum and the wave total
__device__ inline int wave_excl_scan(int v, int &total)
{
    const int incl = wave_scan_add(v);
    total = __builtin_amdgcn_readlane(incl, 63);
    return incl - v;
}
// exclusive prefix sum over the threads of a workgroup of NW waves and the workgroup's total; wtot: NW ints of LDS, free to reuse once the
// next barrier is passed (the one in front of the write orders the reads of an earlier call).  Every thread calls it
template <int NW>
__device__ inline int block_excl_scan(int v, int *wtot, int &total)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int wt;
    const int ex = wave_excl_scan(v, wt);
    __syncthreads();
    if (lane == 0) wtot[wid] = wt;
    __syncthreads();
    int pre = 0, tot = 0;
#pragma unroll
    for (int q = 0; q < NW; q++) {
        const int t = wtot[q];
        pre += q < wid ? t : 0;
        tot += t;
    }
    total = tot;
    return pre + ex;
}
// workgroup barrier, and workgroup OR, that also order the stores to tables that are in LDS for one workgroup and in global memory for
// another (the tiers of k_centreline_rows, k_lobes_rows) before the loads behind them
__device__ __forceinline__ void block_sync_fenced()
{
    __threadfence_block();
    __syncthreads();
    __threadfence_block();
}
__device__ __forceinline__ int block_any_fenced(bool p)
{
    __threadfence_block();
    const int r = __syncthreads_or(p ? 1 : 0);
    __threadfence_block();
    return r;
}
// the value of lane - 1 / lane + 1 (wave_shr:1 / wave_shl:1); the lane without a source takes `fill`
__device__ inline uint32_t wave_shr1(uint32_t v, uint32_t fill) { return (uint32_t)__builtin_amdgcn_update_dpp((int)fill, (int)v, 0x138, 0xf, 0xf, false); }
__device__ inline int wave_shr1(int v, int fill) { return __builtin_amdgcn_update_dpp(fill, v, 0x138, 0xf, 0xf, false); }
__device__ inline int wave_shl1(int v, int fill) { return __builtin_amdgcn_update_dpp(fill, v, 0x130, 0xf, 0xf, false); }

// ---- cv::warpAffine's fixed-point source coordinates (WarpAffineInvoker)
constexpr int AB_BITS = 10, AB_SCALE = 1 << AB_BITS, INTER_BITS = 5, INTER_TAB = 1 << INTER_BITS;
struct Aff { double m[6]; };      // source = M * (x, y, 1): the inverse map warpAffine iterates with
__device__ inline long long cvr(double v) { return __double2ll_rn(v); }          // cvRound / saturate_cast<int>(double): half to even
// source coordinate of destination pixel (x, y).  INTER_LINEAR: round_delta = AB_SCALE / INTER_TAB / 2, shift = AB_BITS - INTER_BITS (integer
// part and 1/32 fraction); INTER_NEAREST: round_delta = AB_SCALE / 2, shift = AB_BITS
__device__ inline void warp_src_coord(const Aff &a, int x, int y, int round_delta, int shift, int &X, int &Y)
{
    const long long ad = cvr(a.m[0] * x * AB_SCALE), bd = cvr(a.m[3] * x * AB_SCALE);
    const long long X0 = cvr((a.m[1] * y + a.m[2]) * AB_SCALE) + round_delta, Y0 = cvr((a.m[4] * y + a.m[5]) * AB_SCALE) + round_delta;
    X = (int)((X0 + ad) >> shift);
    Y = (int)((Y0 + bd) >> shift);
}

// block-wide sum for blockDim.x <= 1024; `scratch` must hold 16 elements of T; result valid in all threads
template <typename T>
__device__ inline T block_sum(T v, T *scratch)
{
    int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    v = wave_sum(v);
    __syncthreads();
    if (lane == 0) scratch[wid] = v;
    __syncthreads();
    T r = 0;
    for (int i = 0; i < nw; i++) r += scratch[i];
    return r;
}
__device__ inline unsigned long long block_max_u64(unsigned long long v, unsigned long long *scratch)
{
    int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    v = wave_max_u64(v);
    __syncthreads();
    if (lane == 0) scratch[wid] = v;
    __syncthreads();
    unsigned long long r = 0;
    for (int i = 0; i < nw; i++) r = scratch[i] > r ? scratch[i] : r;
    return r;
}
__device__ inline unsigned long long block_min_u64(unsigned long long v, unsigned long long *scratch)
{
    int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    v = wave_min_u64(v);
    __syncthreads();
    if (lane == 0) scratch[wid] = v;
    __syncthreads();
    unsigned long long r = ~0ull;
    for (int i = 0; i < nw; i++) r = scratch[i] < r ? scratch[i] : r;
    return r;
}

// Dynamic-LDS limit of a kernel above the 64 KB default: the attribute is per device, and one process may hold sessions on several
// GPUs, so "already set" is tracked per device ordinal.
struct DynLdsOnce { bool done[64] = {}; };
inline void ensure_dyn_lds(DynLdsOnce &o, const void *fn, int bytes)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = -1;
    if (dev >= 0 && dev < 64 && o.done[dev]) return;
    (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (dev >= 0 && dev < 64) o.done[dev] = true;
}

// calibration curve (shape_ftp.py:682-700 / force_sensor.py:129-167), double arithmetic
struct Curve { int type; double a, b, c; };
__host__ __device__ inline double curve_eval(const Curve &cv, double v)
{
    switch (cv.type) {
    case 0: return cv.a * v;
    case 1: return cv.a * v + cv.b;
    case 2: return cv.a * v * v + cv.b * v + cv.c;
    case 3: return cv.a * (1.0 - exp(-cv.b * fmax(v, 0.0)));
    case 4: return cv.a * (exp(cv.b * fmax(v, 0.0)) - 1.0);
    default: return cv.a * ((1.0 - exp(-cv.b * fmax(v - cv.c, 0.0))) - (1.0 - exp(-cv.b * fmax(0.0 - cv.c, 0.0))));
    }
}

}  // namespace vf
