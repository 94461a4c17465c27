// The least-squares polynomial over a contact's pixels in box-centred coordinates, shared by the shape read-out (k_shapes.hip: the quadric cap)
// and the texture read-out (k_texture.hip: the form that is taken away): the accumulation of the monomial sums, the normal equations with the
// two-Cholesky verdict, and the evaluation.  Both headers (include/vistaf_shape.h step 5 and 7, include_ext/vistaf_texture.h step 2 and 3)
// promise these operations in this order; one copy keeps their bits the same.  Device inline code only.
#pragma once
#include "chol.hpp"
#include "common.hpp"

namespace vf {

constexpr int FIT_NF = 20;                                  // float64 sums: 14 monomials beside the pixel count, 6 right-hand sides
constexpr double FIT_PIVOT_FLOOR = 1.0 / 4294967296.0;      // 2^-32 of the diagonal

// box-centred coordinates of the table's own box bx0..by1: u = (x - xc) / hx, v = (y - yc) / hy
struct FitCoords {
    double xc, yc, hx, hy;
    __device__ inline FitCoords(int bx0, int by0, int bx1, int by1)
        : xc(((double)bx0 + (double)bx1) / 2.0), yc(((double)by0 + (double)by1) / 2.0), hx(fmax(((double)bx1 - (double)bx0) / 2.0, 1.0)),
          hy(fmax(((double)by1 - (double)by0) / 2.0, 1.0))
    {
    }
    __device__ inline double u(int px) const { return ((double)px - xc) / hx; }
    __device__ inline double v(int py) const { return ((double)py - yc) / hy; }
};

// one pixel of depth dd at (u, v) into the thread's sums f[FIT_NF]
__device__ inline void fit_accumulate(double (&f)[FIT_NF], double u, double v, double dd)
{
    const double u2 = u * u, uv = u * v, v2 = v * v, u3 = u2 * u, u2v = u2 * v, uv2 = u * v2, v3 = v2 * v;
    f[0] += u; f[1] += v; f[2] += u2; f[3] += uv; f[4] += v2; f[5] += u3; f[6] += u2v; f[7] += uv2; f[8] += v3;
    f[9] += u2 * u2; f[10] += u3 * v; f[11] += u2 * v2; f[12] += u * v3; f[13] += v2 * v2;
    f[14] += dd; f[15] += dd * u; f[16] += dd * v; f[17] += dd * u2; f[18] += dd * uv; f[19] += dd * v2;
}

// The first N of the basis 1, u, v, u*u, u*v, v*v fitted to the workgroup's sums tf[FIT_NF] over dm pixels: the normal equations A c = rhs, the
// verdict from chol_solve<N> of A - 2^-32 diag(A), the solution from chol_solve<N> of A.  false: no fit (c is then not to be read).
template <int N>
__device__ inline bool fit_solve(const double *tf, double dm, double (&c)[6])
{
    // S(a, b) = sum u^a v^b
    const double S[5][5] = {{dm, tf[1], tf[4], tf[8], tf[13]}, {tf[0], tf[3], tf[7], tf[12], 0}, {tf[2], tf[6], tf[11], 0, 0},
                            {tf[5], tf[10], 0, 0, 0}, {tf[9], 0, 0, 0, 0}};
    constexpr int ea[6] = {0, 1, 0, 2, 1, 0}, eb[6] = {0, 0, 1, 0, 1, 2};
    double A[6][6], A2[6][6], c2[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 6; j++) c[j] = tf[14 + j];
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j < 6; j++) {
            A[i][j] = S[ea[i] + ea[j]][eb[i] + eb[j]];
            A2[i][j] = i == j ? A[i][j] - FIT_PIVOT_FLOOR * A[i][j] : A[i][j];
        }
    return chol_solve<N>(A2, c2) && chol_solve<N>(A, c);
}

// the fitted polynomial, summed left to right
__device__ inline double fit_poly(const double *c, double u, double v)
{
    return c[0] + c[1] * u + c[2] * v + c[3] * (u * u) + c[4] * (u * v) + c[5] * (v * v);
}

}  // namespace vf
