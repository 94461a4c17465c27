/* vistaf_tempmodel.h -- C ABI of the temperature regressors (last slice), part of libvistaf_ftp.so.
 *
 * Replaces, on the MI355X, the step that turns the feature planes into temperature maps:
 *
 *   Code/temperature_sensor.py:230-243  TempModel.predict(X)          a fitted StandardScaler -> PolynomialFeatures -> HuberRegressor
 *                                                                     pipeline, optionally followed by an IsotonicRegression calibrator
 *   Code/temperature_sensor.py:295      predict_map_for_mask(planes, mask)
 *
 * The library never loads a pickle.  A model is handed over as the arrays of the fitted objects (the Python side reads them from
 * already-loaded scikit-learn objects or from a JSON file, tempmodel.py):
 *   n_features F (1..4) and feature_planes[F]: which plane feeds feature f (0 = L, 1 = a, 2 = b, 3 = gray; distinct)
 *   StandardScaler   mean[F] (mean_), scale[F] (scale_, finite and > 0), with_mean, with_std (NULL allowed where the flag is off)
 *   PolynomialFeatures  powers[T][F] (powers_, row-major, including the bias row when include_bias); every row of degree <= 4, no two
 *                    rows equal, T <= 70 (all monomials of 4 features up to degree 4); interaction_only is not part of the family
 *   HuberRegressor   coef[T] (coef_), intercept (intercept_), finite doubles
 *   IsotonicRegression (optional, n_iso = 0: none)  iso_x[K] (X_thresholds_, finite, strictly increasing), iso_y[K] (y_thresholds_,
 *                    finite), x_min / x_max (X_min_ / X_max_), out_of_bounds 0 = "clip", 1 = "nan" ("raise" is not supported)
 * The calibrator is assumed to compose as iso(pipeline(X)), as the colour model's metrics file records use_isotonic_calibration; the
 * reference's TempModel source that applies it is not part of the mounted tree.
 *
 * ARITHMETIC (pinned against scikit-learn 1.7 / NumPy 2 / SciPy 1.15 on the CPU): what those libraries compute for the input dtype.
 *   float32 input (the feature planes, float32 rows):
 *     z = f32(f64(x) - mean) if with_mean, then z = f32(f64(z) / scale) if with_std               (StandardScaler.transform, in place)
 *     a monomial of degree >= 2 is f32(x_f * parent), f the lowest feature with a nonzero power, parent the monomial with one power of f
 *     removed: the order in which PolynomialFeatures.transform builds its columns (L^2 a = L (L a))
 *     y = sum_t coef[t] * f64(term_t) + intercept in float64
 *   float64 rows: the same steps in float64.
 *   isotonic on the float64 y, as IsotonicRegression._transform with SciPy's interp1d, which delegates float64 tables to np.interp:
 *     clip mode: y = min(max(y, x_min), x_max); then y outside [iso_x[0], iso_x[K-1]] is NaN (interp1d's fill value, so "nan" mode);
 *     y == iso_x[j] gives iso_y[j]; otherwise j with iso_x[j] < y < iso_x[j+1],
 *     slope = (iso_y[j+1] - iso_y[j]) / (iso_x[j+1] - iso_x[j]), result slope * (y - iso_x[j]) + iso_y[j]; K = 1: the constant iso_y[0].
 *     A NaN prediction stays NaN (features are finite in every path the reference runs).
 *   Maps are f32 of the result; rows stay float64.  The float64 sum runs in term order with fused multiply-adds where NumPy's matmul
 *   hands the dot to BLAS, so the float64 result can differ in the last bits (< 1e-12 relative) and a map value by at most one float32 ulp.
 * TERM CONVENTION (pinned against the reference's stored equations, tests/golden/ref_temp_{color,black}_metrics.json): the six fitted
 *   models list their terms in PolynomialFeatures.powers_ order with the bias column beside the intercept.
 * NOT PINNED: the reference's own fitted parameters (its scaler means and scales are only inside the .joblib files, absent from the tree);
 *   parity with the shipped models is the user's export of them.
 *
 * Every function returns 0 or a negative VISTAF_E_* code (vistaf_ftp.h); vistaf_ftp_last_error() holds the message.  Device pointers are
 * HIP device pointers, `stream` a hipStream_t passed as void*.
 */
#ifndef VISTAF_TEMPMODEL_H
#define VISTAF_TEMPMODEL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vistaf_tmodel vistaf_tmodel;

#define VISTAF_TMODEL_MAX_FEATURES 4
#define VISTAF_TMODEL_MAX_DEGREE 4
#define VISTAF_TMODEL_MAX_TERMS 70
#define VISTAF_TMODEL_PLANE_L 0
#define VISTAF_TMODEL_PLANE_A 1
#define VISTAF_TMODEL_PLANE_B 2
#define VISTAF_TMODEL_PLANE_GRAY 3
#define VISTAF_TMODEL_OOB_CLIP 0
#define VISTAF_TMODEL_OOB_NAN 1

/* Validates the arrays (host pointers), uploads them to the current device once (synchronous).  Invalid arguments -- null pointers, a
 * feature count or plane outside the ranges above, scale <= 0, non-finite values, powers of degree > 4 or repeated, a term count outside
 * 1..70, an unsorted or non-finite isotonic table, x_min > x_max, an unknown out_of_bounds -- return VISTAF_E_INVALID. */
int vistaf_tmodel_create(int n_features, const int32_t *feature_planes, const double *mean, const double *scale, int with_mean, int with_std,
                         int n_terms, const int32_t *powers, const double *coef, double intercept, int n_iso, const double *iso_x,
                         const double *iso_y, double iso_x_min, double iso_x_max, int iso_out_of_bounds, vistaf_tmodel **out);
void vistaf_tmodel_destroy(vistaf_tmodel *m);

/* predict_map_for_mask for n_models = 1 or 2 models in one pass over the planes: d_out[k][i] = f32(model_k(pixel i)) where d_masks[k][i]
 * is nonzero, NaN elsewhere.  d_planes[4] = L, a, b, gray float32 [H, W] (a plane no model uses may be NULL); masks uint8 [H, W]; any
 * H, W >= 1.  The outputs are the only writes.  Isotonic tables are staged in LDS when they fit (<= 2048 entries per launch), else searched
 * in global memory.  Asynchronous on `stream`. */
int vistaf_tmodel_predict_maps(int n_models, const vistaf_tmodel *const *models, const uint8_t *const *d_masks, float *const *d_outs,
                               const float *const *d_planes, int64_t H, int64_t W, void *stream);

/* TempModel.predict(X): d_rows [n_rows, F] row-major, float32 (rows_dtype 0) or float64 (rows_dtype 1), F = the model's n_features,
 * feature f in column f; d_out float64 [n_rows].  n_rows >= 0.  Asynchronous on `stream`. */
int vistaf_tmodel_predict_rows(const vistaf_tmodel *m, const void *d_rows, int rows_dtype, int64_t n_rows, double *d_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
