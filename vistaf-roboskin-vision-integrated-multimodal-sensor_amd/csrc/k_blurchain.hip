// Short Gaussian blurs (ksize <= GF_MAXK) with the element-wise passes around them run inside the blur's LDS tile (gauss_tile.hpp): the
// planes that the streaming kernels hand to the blur and take from it (inorm, z0, mplane, num, den, z0f, snum) never travel to memory.
// Every expression is the one its streaming kernel calls (pixel_ops.hpp), the taps are the plain blur's: same bits as the kernel sequence.
#include "kernels.hpp"
#include "gauss_tile.hpp"
#include "pixel_ops.hpp"

namespace vf {

// ---- illumination normalise -> pre-blur -> apodise: k_illum_norm, k_gauss_fused, k_mul_static ---------------------------------------
template <int RMAX>
__global__ __launch_bounds__(256) void k_illum_pre_apod(const float *__restrict__ img, const float *__restrict__ blur_illum,
                                                        const float *__restrict__ apo, float *__restrict__ iw,
                                                        const float *__restrict__ kern, int ksize, int h, int w)
{
    __shared__ __align__(16) GaussTile<RMAX, 1> tile;
    const size_t P = (size_t)h * w;
    gauss_tile(tile,
               [&](size_t b, int y, int x, float (&v)[1]) {
                   const size_t i = b * P + (size_t)y * w + x;
                   v[0] = illum_norm_px(img[i], blur_illum[i]);
               },
               [&](size_t b, int y, int x, const float (&blur)[1], const float (&)[1]) {
                   const size_t p = (size_t)y * w + x;
                   iw[b * P + p] = mul_static_px(blur[0], apo[p]);
               },
               kern, ksize, h, w);
}
void launch_illum_pre_apod(const float *img, const float *blur_illum, const float *apo, float *iw, const float *kern, int ksize, int B, int h,
                           int w, hipStream_t st)
{
    VF_LAUNCH_GAUSS_TILE(k_illum_pre_apod, ksize, B, h, w, st, img, blur_illum, apo, iw, kern, ksize, h, w);
}

// ---- reliable-only smoothing: k_sub_scalar_mask, k_gauss_fused on the masked values and on the mask, k_div_planes ----------------------
template <int RMAX>
__global__ __launch_bounds__(256) void k_smooth_reliable(const float *__restrict__ detr, const float *__restrict__ bg_med,
                                                         const uint8_t *__restrict__ reliable, float *__restrict__ hmap,
                                                         const float *__restrict__ kern, int ksize, int h, int w)
{
    __shared__ __align__(16) GaussTile<RMAX, 2> tile;
    const size_t P = (size_t)h * w;
    const float med = bg_med[blockIdx.z];
    gauss_tile(tile,
               [&](size_t b, int y, int x, float (&v)[2]) {
                   const size_t i = b * P + (size_t)y * w + x;
                   sub_scalar_mask_px(detr[i], med, reliable[i], v[0], v[1]);
               },
               [&](size_t b, int y, int x, const float (&blur)[2], const float (&)[2]) {
                   hmap[b * P + (size_t)y * w + x] = div_planes_px(blur[0], blur[1]);
               },
               kern, ksize, h, w);
}
void launch_smooth_reliable(const float *detr, const float *bg_med, const uint8_t *reliable, float *hmap, const float *kern, int ksize, int B,
                            int h, int w, hipStream_t st)
{
    VF_LAUNCH_GAUSS_TILE(k_smooth_reliable, ksize, B, h, w, st, detr, bg_med, reliable, hmap, kern, ksize, h, w);
}

// ---- frontier taper -> unreliable-region blur -> clamp -> mm curve: k_frontier_compose, k_gauss_fused, k_finalize_unitless, k_to_mm ------
// dist_out is never a plane the kernel writes (post_demod puts the second distance transform into a plane that is idle when this kernel
// runs, not into `depth`), so every pointer is __restrict__ and the store step's reads of a tile's eight output rows (GaussTile's `pre`)
// are all in flight before the float64 mm curve of the first row is evaluated.
struct ComposeRowIn { uint8_t roi, rel; float den, dist; };
template <int RMAX>
__global__ __launch_bounds__(256) void k_compose_finalize_mm(const float *__restrict__ hmap, const uint8_t *__restrict__ reliable,
                                                             const uint8_t *__restrict__ roi, const float *__restrict__ dist_in, float taper_band,
                                                             const float *__restrict__ roi_den, const float *__restrict__ dist_out, float band,
                                                             int use_band, Curve curve, int use_neg, float *__restrict__ unitless,
                                                             float *__restrict__ depth, uint8_t *__restrict__ cand,
                                                             unsigned int *__restrict__ gmax_bits, const float *__restrict__ kern, int ksize, int h,
                                                             int w)
{
    __shared__ __align__(16) GaussTile<RMAX, 1> tile;
    __shared__ unsigned long long scratch[16];
    const size_t P = (size_t)h * w;
    unsigned int mx = 0;
    gauss_tile(tile,
               [&](size_t b, int y, int x, float (&v)[1]) {
                   const size_t p = (size_t)y * w + x, i = b * P + p;
                   const uint8_t rel = reliable[i], in_roi = roi[p];      // all four requested before any is looked at
                   const float hgt = hmap[i], din = dist_in[i];
                   v[0] = frontier_compose_px(rel && in_roi, hgt, din, taper_band);
               },
               [&](size_t b, int y, int x) {
                   const size_t p = (size_t)y * w + x, i = b * P + p;
                   ComposeRowIn c;
                   c.roi = roi[p]; c.rel = reliable[i]; c.den = roi_den[p]; c.dist = dist_out[i];
                   return c;
               },
               [&](size_t b, int y, int x, const float (&blur)[1], const float (&z0)[1], const ComposeRowIn &in) {
                   const size_t i = b * P + (size_t)y * w + x;
                   const bool in_roi = in.roi != 0, rel = in_roi && in.rel != 0;
                   const float u = finalize_unitless_px(in_roi, rel, z0[0], true, blur[0], in.den, use_band != 0, in.dist, band);
                   unitless[i] = u;
                   float d;
                   const bool c = to_mm_px(u, in_roi, curve, use_neg, d);
                   depth[i] = d;
                   cand[i] = (uint8_t)c;
                   if (c) { unsigned int bits = __float_as_uint(d); if (bits > mx) mx = bits; }
               },
               kern, ksize, h, w);
    unsigned long long m = block_max_u64(mx, scratch);
    if (threadIdx.x == 0 && m) atomicMax(&gmax_bits[blockIdx.z], (unsigned int)m);
}
void launch_compose_finalize_mm(const float *hmap, const uint8_t *reliable, const uint8_t *roi, const float *dist_in, float taper_band,
                                const float *roi_den, const float *dist_out, float band, int use_band, Curve curve, int use_neg, float *unitless,
                                float *depth, uint8_t *cand, unsigned int *gmax_bits, const float *kern, int ksize, int B, int h, int w,
                                hipStream_t st)
{
    hipMemsetAsync(gmax_bits, 0, sizeof(unsigned int) * B, st);
    VF_LAUNCH_GAUSS_TILE(k_compose_finalize_mm, ksize, B, h, w, st, hmap, reliable, roi, dist_in, taper_band, roi_den, dist_out, band, use_band,
                         curve, use_neg, unitless, depth, cand, gmax_bits, kern, ksize, h, w);
}

}  // namespace vf
