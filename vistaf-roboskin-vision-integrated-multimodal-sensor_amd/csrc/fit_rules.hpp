// The rules of robust_polyfit2d (shape_ftp.py:1086-1136) that every dataflow of the fit spells the same way; private to k_fit.hip and
// k_big.hip.  What stays apart on purpose is listed in DESIGN.md, "The selection and fit family's one copy".
// tests/diag/fit_select_host_check.hip runs the __host__ __device__ rules on the host.
#pragma once
#include "common.hpp"

namespace vf {

#define VF_RULE __device__ __attribute__((always_inline)) inline
#define VF_HRULE __host__ __device__ __attribute__((always_inline)) inline

// ---- coordinates: pixel i of n -> [-1, 1] in float32; n = 1 gives 0 / 0 = NaN (such a plane never passes the gate's 200 pixels)
VF_HRULE float fit_centre(int n) { return (float)((n - 1) / 2.0); }
VF_HRULE float fit_coord(int i, float centre) { return rn_div(rn_sub((float)i, centre), centre); }

// ---- the fitted surface.  eval_poly2d's operation order (shape_ftp.py:1093-1097): what the residual plane subtracts
VF_HRULE float fit_eval(const float *c, int order, float xn, float yn)
{
    float fit = rn_add(rn_add(rn_mul(c[0], xn), rn_mul(c[1], yn)), c[2]);
    if (order >= 2) {
        fit = rn_add(fit, rn_mul(rn_mul(c[3], xn), xn));
        fit = rn_add(fit, rn_mul(rn_mul(c[4], xn), yn));
        fit = rn_add(fit, rn_mul(rn_mul(c[5], yn), yn));
    }
    return fit;
}
// Column form, for the sweeps of a thread that keeps one image column: fit = (yn Bt + At) + c5 yn^2 with the terms of x formed once
struct FitCol { float At, Bt; };
VF_RULE FitCol fit_col_terms(const float *c, float xn)
{
    return {fmaf(c[3], __fmul_rn(xn, xn), fmaf(c[0], xn, c[2])), fmaf(c[4], xn, c[1])};
}
VF_RULE float fit_col_eval(float At, float Bt, float c5, float yn) { return __fadd_rn(fmaf(yn, Bt, At), __fmul_rn(c5, __fmul_rn(yn, yn))); }

// ---- IRLS weight 1 / (1 + (r / csig)^2) from the residual and 1 / csig, and scale
VF_RULE float fit_cauchy(float r, float inv_csig)
{
    const float uu = __fmul_rn(r, inv_csig);
    return __fdiv_rn(1.0f, __fadd_rn(1.0f, __fmul_rn(uu, uu)));
}
// csig = c * sigma, sigma = 1.4826 * (median|r - median r| + 1e-6)
VF_HRULE float fit_csig(float c, float mad) { return rn_mul(c, rn_mul(1.4826f, rn_add(mad, 1e-6f))); }

// ---- key ranges of the two medians, without a pass over the data (the histogram refinement only needs a range that CONTAINS the keys)
struct FitKeys { uint32_t kmin, kmax; };
// r = z - fit: |xn|, |yn| <= 1, so |fit| <= sum |coef| (plus rounding slack)
VF_HRULE FitKeys fit_resid_range(const float *c, float zmin, float zmax)
{
    float fb = 0.f;
    for (int i = 0; i < 6; i++) fb += fabsf(c[i]);
    fb = fb * 1.0001f + 1e-30f;
    return {f2key(zmin - fb - 1e-6f * fabsf(zmin)), f2key(zmax + fb + 1e-6f * fabsf(zmax))};
}
// |r - med| lies in [0, max(rmax - med, med - rmin)] (float subtraction is monotone)
VF_HRULE FitKeys fit_mad_range(FitKeys r, float med)
{
    const float hi1 = fabsf(rn_sub(key2f(r.kmax), med)), hi2 = fabsf(rn_sub(key2f(r.kmin), med));
    return {f2key(0.f), f2key(hi1 > hi2 ? hi1 : hi2)};
}

// ---- the gate: 200 fitted pixels upstream (:1103); min_mask_count: 500 mask pixels for the ramp removal (:1364-1366), else 0
VF_HRULE bool fit_gate(int n, int nmask, int min_count, int min_mask_count) { return n >= min_count && (min_mask_count <= 0 || nmask >= min_mask_count); }

// ---- normal equations from monomial sums.  Index of the sum of w^2 x^a y^b among the (DEG + 1)(DEG + 2) / 2 monomials of degree <= DEG:
// b-major with DEG + 1, DEG, ... entries
VF_HRULE constexpr int fit_mono(int a, int b, int DEG) { return b * (DEG + 1) - b * (b - 1) / 2 + a; }
// A = A^T W^2 A and rhs of the NC coefficients [x, y, 1, x^2, xy, y^2] from S: the monomial sums of degree <= DEG (DEG >= 2 for NC = 3, 4 for
// NC = 6), followed by the right-hand sides in the order of the basis.  Rows and columns >= NC are zero.
template <int NC, int DEG>
VF_HRULE void fit_assemble(const double *S, double (&A)[6][6], double (&rhs)[6])
{
    static_assert((NC == 3 && DEG >= 2) || (NC == 6 && DEG >= 4), "the products of two basis functions are among the monomials");
    constexpr int NM = (DEG + 1) * (DEG + 2) / 2;
    const int ea[6] = {1, 0, 0, 2, 1, 0}, eb[6] = {0, 1, 0, 0, 1, 2};          // exponents of the basis
#pragma unroll
    for (int i = 0; i < 6; i++) {
#pragma unroll
        for (int j = 0; j < 6; j++) {
            const int k = fit_mono(ea[i] + ea[j], eb[i] + eb[j], DEG);
            A[i][j] = (i < NC && j < NC) ? S[k < NM ? k : 0] : 0.0;
        }
        rhs[i] = i < NC ? S[NM + i] : 0.0;
    }
}

#undef VF_RULE
#undef VF_HRULE

}  // namespace vf
