// The complex128 product C = A . Q as the real float64 GEMM  [re | im] = [Ar | Ai] . [[Qr, Qi], [-Qi, Qr]]  on the matrix cores
// (v_mfma_f64_16x16x4_f64), the one copy behind k_dft_inv2_mfma, k_full2_mfma (k_dft.hip) and the column transforms of the pressure
// read-out (k_pressure.hip).  Operand layout of the instruction: A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15],
// D[row = (lane >> 4) + 4 * reg][col = lane & 15].
#pragma once
#include <hip/hip_runtime.h>

namespace vf {

typedef double v4f64 __attribute__((ext_vector_type(4)));

// One wave's 16 rows x 64 columns of C (four column tiles x {re, im} accumulators, zeroed here): row ya of A (the lane's own, clamped by
// the caller) against columns x0 + 16 t + (lane & 15) of Q, clamped to ncols - 1.  A is [rows][lda] double2 handed over as doubles, Q is
// [lda][ldq] double2; the sum runs over k = 0..kext-1 (kext <= lda), K = 2 * kext real k-steps of 4: first the real parts of A's row, then
// the imaginary parts, one double2 of Q per lane and k-step giving both B operands ((q.x, q.y) below kext, (-q.y, q.x) above).
// Operands come straight from global memory / L2.
__device__ __forceinline__ void cgemm16x64_mfma(const double *__restrict__ A, int lda, int kext, const double2 *__restrict__ Q, int ldq, int ncols,
                                                int ya, int x0, int lane, v4f64 (&cre)[4], v4f64 (&cim)[4])
{
    const int r = lane & 15, kk = lane >> 4;
#pragma unroll
    for (int t = 0; t < 4; t++) { cre[t] = (v4f64){0.0, 0.0, 0.0, 0.0}; cim[t] = (v4f64){0.0, 0.0, 0.0, 0.0}; }
    const int K = 2 * kext;
    for (int k0 = 0; k0 < K; k0 += 4) {
        const int k = k0 + kk;
        const bool in = k < K, hi = k >= kext;
        const int kq = in ? (hi ? k - kext : k) : 0;
        const double a = in ? A[((size_t)ya * lda + kq) * 2 + (hi ? 1 : 0)] : 0.0;
        double2 q[4];
#pragma unroll
        for (int t = 0; t < 4; t++) q[t] = Q[(size_t)kq * ldq + min(x0 + 16 * t + r, ncols - 1)];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const double bre = in ? (hi ? -q[t].y : q[t].x) : 0.0, bim = in ? (hi ? q[t].x : q[t].y) : 0.0;
            cre[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bre, cre[t], 0, 0, 0);
            cim[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bim, cim[t], 0, 0, 0);
        }
    }
}

// The staged sibling: the same k-steps in the same order with the same operand in every (lane, k) slot, read from LDS.  sA: this wave's 16 rows
// of A as they lie in memory ([16][lda] double2 handed over as doubles), ra the lane's own row among them (clamped by the caller); sQ: rows
// 0..kext-1 of the workgroup's 64 columns of Q ([kext][64] double2, columns past ncols clamped when they were staged).  NT column tiles from
// tile t0 on: the caller walks the four tiles in passes, so that only 2 NT accumulators are live across its epilogue.  A row of sQ is 1 KB, so
// a lane's bank depends on its column alone and the 16-byte reads are conflict-free; the 8-byte read of sA is two-way at worst.
template <int NT>
__device__ __forceinline__ void cgemm16_lds_mfma(const double *sA, int lda, int kext, const double2 *sQ, int ra, int t0, int lane, v4f64 (&cre)[NT],
                                                 v4f64 (&cim)[NT])
{
    const int r = lane & 15, kk = lane >> 4;
#pragma unroll
    for (int t = 0; t < NT; t++) { cre[t] = (v4f64){0.0, 0.0, 0.0, 0.0}; cim[t] = (v4f64){0.0, 0.0, 0.0, 0.0}; }
    const int K = 2 * kext;
    for (int k0 = 0; k0 < K; k0 += 4) {
        const int k = k0 + kk;
        const bool in = k < K, hi = k >= kext;
        const int kq = in ? (hi ? k - kext : k) : 0;
        const double av = sA[(ra * lda + kq) * 2 + (hi ? 1 : 0)];  // read whatever `in` says (kq is 0 beyond K): no branch in the loop
        const double a = in ? av : 0.0;
        double2 q[NT];
#pragma unroll
        for (int t = 0; t < NT; t++) q[t] = sQ[kq * 64 + 16 * (t0 + t) + r];
#pragma unroll
        for (int t = 0; t < NT; t++) {
            const double bre = in ? (hi ? -q[t].y : q[t].x) : 0.0, bim = in ? (hi ? q[t].x : q[t].y) : 0.0;
            cre[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bre, cre[t], 0, 0, 0);
            cim[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bim, cim[t], 0, 0, 0);
        }
    }
}

}  // namespace vf
