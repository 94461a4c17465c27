// Launcher declarations for the gfx950 FTP kernels.  All pointers are device pointers; planes are
// [B, P] (P = h*w) unless noted; `st` is the HIP stream every launch goes to.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>
#include "common.hpp"

namespace vf {

// Which of the parity-equivalent kernels a stage runs.  Defaults are the production kernels; the alternatives are fallbacks for
// sizes or masks the defaults do not cover and stay selectable so the parity tests can pin them against the defaults (csrc/test_hooks.h).
// The fields marked "test only" force such a fallback on inputs that would not take it.
struct Tiers {
    int inpaint = 2;            // 2: frame-window march (k_telea_window) + whole-frame fallback; 1: whole-frame kernel only; 0: cluster front end first
    int big_flood_handback = 0; // test only: 1 = the bitmap flood of frames beyond the uint16 rank range (k_unwrap_big.hip) hands every frame to the generic kernel
    int chamfer_twopass = 0;    // 1: force the one-wave two-pass chamfer even where the LDS closed form applies
    int telea_two_tier = 1;     // 1: 111 KB first tier of the window march + full-size retry of the frames it hands back; 0: full size only
    int unwrap_fast = 1;        // 1: frames whose wrapped field is verified path-independent skip the priority flood (k_unwrap_fast.hip); 0: always flood
    int big_chain = 1;          // 1: frames of 512 x 512 and more take k_big.hip's chains of streaming kernels for the exact selections and the IRLS fits; 0: one workgroup per frame
    int big_queue_lds = 1;      // 1: a big cluster's march keeps its queue in LDS whenever its cell counts bound the queue (k_inpaint_big.hip); 0: always this wave's slice of global memory
    int big_gq_cap = 0;         // test only: capacity (entries, power of two) the big-cluster march checks its global queue slice against; 0: the slice's own size
    int big_fallback = 1;       // 1: frames whose big-cluster queue overflowed are re-marched by the whole-frame kernel; 0: they keep status 2 (test only)
    int telea_mw = 1;           // 1: the 16-wave window kernel (ordering pass + dataflow fills, k_inpaint_mw.hip) as first tier, single-wave tiers behind it; 0: single-wave tiers only
    int fused_backend = 1;      // 1: frames whose label forest fits LDS run blob filter, force tail and output copy in one launch per batch (k_backend.hip); 0: the separate kernels
    int select_resident = 1;    // 1: the exact selections of planes of up to 65536 pixels keep their keys in registers (k_select_resident) and the core threshold and core median share a launch; 0: the streaming k_select, one launch per selection
    int fused_masks = 7;        // bits 1 / 2 / 4: the bad-pixel, reliable and contact mask chain of frames mask_chain_fits takes run as one launch each, bit planes in LDS (k_maskchain.hip); 0: the separate kernels
    int dft_staged = 1;         // 1: the demodulation stages dft_staged_fits names take their operands from LDS (k_dft.hip: k_dft_fwd1_staged, k_dft_inv2_staged); 0: every stage reads global memory / L2 per k-step
    int fused_chains = 1;       // 1: the element-wise passes around a short Gaussian (<= 15 taps) run inside the blur's tile (k_blurchain.hip); 0: one streaming kernel each
    int gauss_strip = 1;        // 1: a session's long Gaussians (> 15 taps) on frames gauss_strip_fits takes run both passes in one launch, the intermediate in LDS (k_gauss_strip); 0: the row and the column kernel
    int fit_window = 1;         // 1: where a column variant has a window instance, the ramp removal and the first detrend fit share one launch of the window kernel one ladder step down (k_robust_polyfit_colwin), the chained plain-size body behind it for the frames it flags; 0: one plain kernel per fit
};

// Frames of 512 x 512 pixels and more: the ones whose per-frame stages are split over the chip (k_big.hip and the chunked tiers)
inline bool large_frame(size_t P) { return P >= 262144; }

// host_util.hpp: the bump carver every scratch layout is written with, beside its launcher.  The *_scratch_bytes() below run the same layout on a
// null base; `rec` (vistaf_ftp_test_scratch_regions only) receives the regions
struct ScratchLayout;
struct ScratchRegion;
using ScratchRec = std::vector<ScratchRegion>;

struct RowSpanSE {      // structuring element as per-row x spans (cv::getStructuringElement ELLIPSE)
    int k;              // k x k, anchor at centre (k <= 33)
    int8_t lo[33];      // relative x offset of first set element in row i (lo > hi: empty row)
    int8_t hi[33];
};

// ---- k_basic.hip ------------------------------------------------------------------------------
// w: the frame's width, which the camera formats (VISTAF_FMT_RGB_U8 and up, k_formats.hip) need; formats 0..3 are planes of P pixels
void launch_to_gray(const void *frames, int format, float *gray, int B, int P, hipStream_t st, int w = 0);
void launch_sobel_mag(const float *img, float *grad, int B, int h, int w, hipStream_t st);
void launch_bad_flags(const float *img, const float *grad, const uint8_t *valid, const float *thr_hi, const float *thr_g,
                      uint8_t *bad, int B, int P, hipStream_t st);
// force: 0 the dispatch (morph_tier of mask_bits.hpp), or a MorphTier the caller has checked the frame and element for (vistaf_ftp_test_morph)
enum MorphTier { MORPH_GENERIC = 1, MORPH_PREFIX = 2, MORPH_BITS = 3 };      // k_morph; k_row_prefix + k_morph_prefix; k_morph_bits
void launch_morph(const uint8_t *src, uint8_t *dst, int B, int h, int w, const RowSpanSE &se, bool dilate,
                  const uint8_t *and_static, const uint8_t *and_frame, hipStream_t st, uint16_t *prefix_scratch = nullptr, int force = 0);
void launch_morph_seq(const uint8_t *src, uint8_t *dst, uint8_t *tmp, int B, int h, int w, const RowSpanSE &se, const int *dilates, int n,
                      const uint8_t *and_static, const uint8_t *and_frame, hipStream_t st, uint16_t *prefix_scratch = nullptr);
void launch_gauss_rows(const float *src, float *dst, const float *kern, int ksize, int B, int h, int w, hipStream_t st);
// separable blur src -> dst (tmp: intermediate plane of the two-kernel path).  strip: Tiers::gauss_strip.  force: 0 the dispatch, or GAUSS_TWO, or
// GAUSS_STRIP where the caller has checked gauss_strip_fits and src != dst (vistaf_ftp_test_gauss_variant).  Returns the tier launched
enum GaussTier { GAUSS_TWO = 1, GAUSS_STRIP = 2, GAUSS_TILE = 3 };      // k_gauss_rows + k_gauss_cols[_lds]; k_gauss_strip; k_gauss_fused
int launch_gauss_blur(const float *src, float *tmp, float *dst, const float *kern, int ksize, int B, int h, int w, hipStream_t st, bool strip = false,
                      int force = 0);
void launch_gauss_cols(const float *src, float *dst, const float *kern, int ksize, int B, int h, int w, hipStream_t st);
void launch_illum_norm(const float *img, const float *blur, float *out, int B, int P, hipStream_t st);
void launch_mul_static(const float *a, const float *stat, float *out, int B, int P, hipStream_t st);
void launch_count_u8(const uint8_t *m, int *counts, int B, int P, hipStream_t st);

// ---- k_formats.hip: the camera formats (VISTAF_FMT_RGB_U8 .. VISTAF_FMT_BAYER_BGGR_U8) onto the gray plane; launch_to_gray dispatches here ----
// frames: B frames of h x w in `format`, one behind the other (host_util.hpp frame_layout states the stride and the pointer alignment relied
// on); gray: [B, h*w] float32, 8-byte aligned.  The caller has checked format and size with frame_layout.
void launch_camera_gray(const void *frames, int format, float *gray, int B, int h, int w, hipStream_t st);

constexpr int GF_MAXK = 15;    // longest Gaussian that takes the one-kernel LDS tile (gauss_tile.hpp); longer ones run a row and a column kernel

// ---- k_gauss_strip (k_basic.hip): both passes of a long Gaussian in one launch.  A workgroup owns GS_TX output columns of one frame over the full
// height: the row pass streams chunks of GS_CH rows x (GS_TX + 2r) columns through an LDS tile into an LDS plane mid[h][GS_TX], the column pass
// runs out of that plane.  GS_MAXK: the longest kernel whose chunk row two loads per lane cover (GS_TX + 2r <= 128)
constexpr int GS_TX = 32, GS_CH = 32, GS_MAXK = 97, GS_KPAD = 104;      // GS_KPAD: floats per LDS copy of the taps (GS_MAXK + 1 and a multiple of four, zero-filled)
constexpr size_t GS_LDS_MAX = 48 * 1024;      // what a kernel may hold beside the window march's 111 KB ("Sharing a CU")
// floats between the rows of the chunk tile: an ODD multiple of four, so that rows 8 apart lie 32 banks apart (the row pass pairs them in a
// ds_read_b128 lane group, gauss_strip_rows)
constexpr int gs_pitch(int ksize) { return 4 * (((GS_TX + 2 * (ksize / 2) + 3) / 4) | 1); }
inline size_t gauss_strip_lds(int h, int ksize) { return ((size_t)h * GS_TX + (size_t)GS_CH * gs_pitch(ksize) + 2 * GS_KPAD) * sizeof(float); }
// whether launch_gauss_blur may take k_gauss_strip for a ksize-tap blur of h x w frames (src != dst is the caller's to know)
inline bool gauss_strip_fits(int h, int w, int ksize)
{
    return h >= 1 && w >= 1 && ksize > GF_MAXK && ksize <= GS_MAXK && gauss_strip_lds(h, ksize) <= GS_LDS_MAX;
}

// ---- k_blurchain.hip: short blurs (ksize <= GF_MAXK) with their neighbouring element-wise passes fused in ------------------------------
// iw = blur(img / (blur_illum + 1e-6) - 1) * apo
void launch_illum_pre_apod(const float *img, const float *blur_illum, const float *apo, float *iw, const float *kern, int ksize, int B, int h,
                           int w, hipStream_t st);
// hmap = blur(z0) / (blur(m) + 1e-6), (z0, m) of launch_sub_scalar_mask
void launch_smooth_reliable(const float *detr, const float *bg_med, const uint8_t *reliable, float *hmap, const float *kern, int ksize, int B,
                            int h, int w, hipStream_t st);
// launch_frontier_compose, blur, launch_finalize_unitless and launch_to_mm in one; dist_out must not be a plane the kernel writes (unitless, depth, cand)
void launch_compose_finalize_mm(const float *hmap, const uint8_t *reliable, const uint8_t *roi, const float *dist_in, float taper_band,
                                const float *roi_den, const float *dist_out, float band, int use_band, Curve curve, int use_neg, float *unitless,
                                float *depth, uint8_t *cand, unsigned int *gmax_bits, const float *kern, int ksize, int B, int h, int w,
                                hipStream_t st);

// ---- k_select.hip -----------------------------------------------------------------------------
// Per frame: values vals[b*P+i] (|.| if use_abs) over pixels with mask != 0 (mask_stride 0: one static
// mask for all frames), finite, and (le_thr ? value <= le_thr[b] : true).
// reqs[j] >= 0: percentile with q32 = reqs[j];  reqs[j] < 0: median.   out[b*nreq+j], counts[b].
// big_scratch: k_big.hip's chain for large frames; resident: planes of up to 65536 pixels take k_select_resident (false: always the streaming k_select)
void launch_select(const float *vals, const uint8_t *mask, size_t mask_stride, const float *le_thr, bool use_abs,
                   const float *reqs_dev, int nreq, float *out, int *counts, int B, int P, hipStream_t st, void *big_scratch = nullptr,
                   bool resident = true);
// the kernel launch_select starts for (B, P, nreq); big: scratch for the k_big.hip chain is at hand.  SELV_RES<NS>: k_select_resident<NS>, planes of up to 1024 NS pixels
enum SelectVariant { SELV_BIG = 0, SELV_STREAM, SELV_RES16, SELV_RES32, SELV_RES49, SELV_RES64, SELV_COUNT };
int select_variant(int B, int P, int nreq, bool big, bool resident);
// A chain of selections in one launch of the resident kernel: request 0 as launch_select without a threshold, request j > 0 over the elements
// that also satisfy value <= result[j - 1] (what a second launch_select with le_thr = the first one's output computes); result j of frame b
// goes to outs[j][b] (nreq <= 4 host pointers to device arrays), counts[b] is the count of request 0.  Returns the instance launched, or -1
// with nothing launched when no resident instance takes P: the caller then runs one launch_select per link.
int launch_select_chained(const float *vals, const uint8_t *mask, size_t mask_stride, bool use_abs, const float *reqs_dev, int nreq,
                          float *const *outs, int *counts, int B, int P, hipStream_t st);

// ---- k_dft.hip / k_dft_tables.hip ----------------------------------------------------------------
// carrier of one reference frame (shape_ftp.py:878-913, :930-961)
struct CarrierGeom {
    double peak_x, peak_y;      // refined peak (fftshift layout)
    double kx, ky;              // carrier in bins
    double dpx, dpy;            // sub-bin remainder handled by the ramp (0 when both <= 1e-6)
    double period;              // Wf / |kx| (0: invalid)
    int x0, y0, ph, pw;         // patch origin and size in the shifted spectrum
    int px_i, py_i;
    int px_raw, py_raw;         // the chosen integer peak itself (before the sub-bin refinement)
    int ok;
    int keep_carrier;           // 0: the patch is re-centred at DC before the inverse transform (FTP, :945-948); 1: band-pass in place
};
// table strides are in elements per frame (0: one table for the whole batch).  ph / pw: the patch layout (pair mode: pmax x pmax, each sample's
// own extents inside it, tables and window zero beyond them); win_stride: elements per frame of the window (0: one window for the batch)
void launch_dft_forward(const float *iw, const float *mu, const double2 *Ex, const double2 *Ey, size_t tab_stride_x, size_t tab_stride_y,
                        const float *win, double2 *tmpT, double2 *patch, int patch_stride, int B, int h, int w, int ph, int pw, hipStream_t st,
                        int win_stride = 0, bool staged = true);
// field (may be null): float64 field out; cref/amp_ref (may be null): reference field -> wrapped phase difference and amp product.
// staged: Tiers::dft_staged.  geom (pair mode, may be null): the sums run over each sample's own geom[b].ph x geom[b].pw bins of the ph x pw layout, in the order of a
// ph x pw launch of that size (session mode), so a clipped patch gives the bits of its own session
void launch_dft_inverse(const double2 *patch, int patch_stride, const double2 *Gx, const double2 *Gy, size_t tab_stride_x, size_t tab_stride_y,
                        double2 *tmpQ, double2 *field, float *amp, const double2 *cref, const float *amp_ref, size_t ref_stride, float *prod,
                        float *wrapped, int B, int h, int w, int ph, int pw, hipStream_t st, const CarrierGeom *geom = nullptr, bool staged = true);
// the stages that run on the LDS-staged kernels at this shape when `staged` is set (Tiers::dft_staged), as bits; every other stage and shape
// takes the kernels that read their operands from global memory.  per_frame_tables: pair mode (table strides != 0)
enum DftStaged { DFT_STAGED_FWD1 = 1, DFT_STAGED_INV2 = 2 };     // stage 1: k_dft_fwd1_staged; stage 4: k_dft_inv2_staged
int dft_staged_fits(int h, int w, int ph, int pw, bool per_frame_tables);
void launch_dft_full_mag(const float *iw, const float *mu, const double2 *Ex_full, const double2 *Ey_full, double2 *tmp,
                         double *mag, int B, int h, int w, int Hf, int Wf, hipStream_t st);
// stage 1 of launch_dft_full_mag alone (the row transform of the pressure read-out too): T [B*h][nc] = (iw - mu) . Ex, Ex [w][nc]; mu may be null
void launch_dft_rows(const float *iw, const float *mu, const double2 *Ex, double2 *T, int B, int h, int w, int nc, hipStream_t st);
void launch_top_peaks(const double *mag, int B, int Hf, int Wf, int dc, int npeaks, double *out_xyv /* [B][192] */, hipStream_t st);
void launch_carrier_choose(const double *peaks, int npk, const double *mag, int Hf, int Wf, int bw, double max_dy_frac, CarrierGeom *geom, int B,
                           hipStream_t st);
// pair_hann (pair mode, may be null): hann(M)[i] as float32 at pair_hann[M * pmax + i], 1 <= M <= pmax.  Given, the tables are laid out for a
// pmax x pmax patch with zeros beyond each sample's ph / pw, and pair_win[b] (pmax x pmax) receives the sample's window hann(ph) x hann(pw)
// (zeros elsewhere) -- the float32 products hann_patch() forms on the host for a session
void launch_build_tables(const CarrierGeom *geom, int geom_stride, double2 *Ex, double2 *Ey, double2 *Gx, double2 *Gy, size_t stride_x,
                         size_t stride_y, int B, int h, int w, int pad, int Hf, int Wf, int pmax, hipStream_t st, const float *pair_hann = nullptr,
                         float *pair_win = nullptr);
// pair mode: frames without a usable carrier (no peak, or a non-positive period) get status VISTAF_FRAME_NO_CARRIER
void launch_pair_status(const CarrierGeom *geom, int pmax, int32_t *status, const int32_t *status2, int B, hipStream_t st);
void launch_build_full_tables(double2 *Exf, double2 *Eyf, int h, int w, int pad, int Hf, int Wf, hipStream_t st);

// ---- k_cc_dist.hip ----------------------------------------------------------------------------
void launch_threshold_mask(const float *q, const uint8_t *roi, const float *thr, uint8_t *out, int B, int P, hipStream_t st);
// the kernels launch_cc_label starts for an h x w frame: the LDS forest with the mask staged behind it, the LDS forest reading the mask from
// memory, or the union-find in global memory (init, merge, flatten); force_global: the last whatever the size (tests only)
enum CcLabelTier { CCT_LDS_MASK = 0, CCT_LDS = 1, CCT_GLOBAL = 2 };
int cc_label_tier(int h, int w, bool force_global = false);
void launch_cc_label(const uint8_t *mask, int32_t *labels, int B, int h, int w, hipStream_t st, bool force_global = false);
// the kernels launch_cc_largest starts: k_cc_largest (one workgroup per frame) or the three kernels over the whole batch (big_frames, and
// `best` at hand).  force: 0 dispatch, else the tier itself (tests only; CCL_BATCH needs `best`)
enum CcLargestTier { CCL_FRAME = 1, CCL_BATCH = 2 };
int cc_largest_tier(int B, int P, bool have_best, int force = 0);
void launch_cc_largest(const int32_t *labels, int32_t *area_scratch, unsigned long long *best, const uint8_t *and_static,
                       uint8_t *out, int B, int P, hipStream_t st, int force = 0);
// the kernels launch_chamfer / launch_chamfer_pair start: the closed form in LDS, the one-wave two-pass transform, or the closed form through
// the row-distance plane in memory
enum ChamferTier { CHT_LDS = 0, CHT_TWOPASS = 1, CHT_ROWCOL = 2 };
int chamfer_tier(int h, int w, int cap_px, bool force_twopass = false);
int chamfer_pair_tier(int B, int h, int w, int cap_px, bool force_twopass = false);
void launch_chamfer(const uint8_t *src, bool invert, int32_t *rowdist, float *dist, int B, int h, int w, int cap_px, hipStream_t st,
                    bool force_twopass = false);
void launch_chamfer_pair(const uint8_t *src, int32_t *tmp_a, float *dist_a, int32_t *tmp_b, float *dist_b, int B, int h, int w, int cap_px,
                         hipStream_t st, bool force_twopass = false);
void launch_erode_by_dist(const float *dist, const uint8_t *src, float margin, uint8_t *out, int B, int P, hipStream_t st);

// ---- k_inpaint.hip ----------------------------------------------------------------------------
// the whole-frame kernel's planes; inpaint_scratch_bytes: the buffer launch_inpaint_telea and launch_inpaint_big_clusters share (never both in
// one step), the larger of the two layouts
size_t telea_scratch_bytes(int B, int h, int w, ScratchRec *rec = nullptr);
size_t inpaint_scratch_bytes(int B, int h, int w);
// `only` (device, [B], may be null): process just the frames with only[b] != 0
void launch_inpaint_telea(float *img, const uint8_t *bad, int range, void *scratch, int32_t *status, const int32_t *only, int B, int h, int w,
                          hipStream_t st, bool round_u8 = false);      // round_u8: 8-bit image semantics (values 0..255 held as floats, OpenCV's rounding of every estimate)

// ---- k_inpaint_win.hip (LDS-resident window kernel; returns the per-frame fallback flags for launch_inpaint_telea)
size_t inpaint_win_scratch_bytes(int B, ScratchRec *rec = nullptr);
int inpaint_window_cells_cap();         // window cells of the full-size single-wave tier
int inpaint_cluster_cells_cap();        // window cells of one LDS cluster
// ---- k_inpaint_mw.hip (16 waves per frame: ordering pass, then the estimates as a dataflow; flags the frames it cannot take in fb[])
bool inpaint_window_mw_supported(int range);
void launch_telea_window_mw(float *img, const uint8_t *bad, const int32_t *box, int32_t *fb, int range, int B, int h, int w, hipStream_t st);
// alone (tests only): one first tier by itself, without the full-size retry behind it -- WNT_MW the 16-wave kernel (the caller has checked
// inpaint_window_mw_supported), WNT_FIRST the single-wave kernel at first-tier capacity; the full-size single-wave kernel by itself is
// two_tier = mw = false.  The flags returned are then that tier's own hand-backs.
enum WindowTierAlone { WNT_ALL = 0, WNT_MW = 1, WNT_FIRST = 2 };
int32_t *launch_inpaint_window(float *img, const uint8_t *bad, int range, void *scratch, int B, int h, int w, hipStream_t st,
                               hipEvent_t ev_march = nullptr, bool two_tier = true, bool mw = true, int alone = WNT_ALL);

// ---- k_inpaint_cl.hip (cluster-parallel front end; leaves oversized clusters in *bad_big_out) ----------
size_t inpaint_cl_scratch_bytes(int B, int h, int w, ScratchRec *rec = nullptr);
bool inpaint_clusters_supported(int range);
struct ClusterPlanes { const int32_t *labels, *list, *count, *xmin, *ymin, *xmax, *ymax; const uint8_t *dil; };     // [B, P] planes indexed by component root; dil = hole mask dilated by range + 1
// the clusters the LDS windows left over, each on its own wave over padded global planes with the queue in LDS (k_inpaint_big.hip)
// range 0: at the widest padding launch_inpaint_big_clusters takes, which is what a session allocates
size_t inpaint_big_scratch_bytes(int B, int h, int w, int range = 0, ScratchRec *rec = nullptr);
bool inpaint_big_supported(int range);
// gq_cap (test hook big_gq_cap): capacity the march checks its global queue slice against, a power of two <= the slice; 0: the slice's size
void launch_inpaint_big_clusters(float *img, const uint8_t *bad_big, int range, void *scratch, int32_t *status, const ClusterPlanes &left, int B, int h,
                                 int w, hipStream_t st, bool lds_queue = true, int gq_cap = 0);
// status[b] == 2 (a big cluster's queue overflowed) -> only[b] = 1 and status[b] = 0, else only[b] = 0: the frames for launch_inpaint_telea
void launch_inpaint_big_handback(int32_t *status, int32_t *only, int B, hipStream_t st);
void launch_inpaint_clusters(float *img, const uint8_t *bad, int range, void *scratch, uint8_t **bad_big_out, ClusterPlanes *left, int B, int h, int w,
                             hipStream_t st);

// ---- k_unwrap.hip -----------------------------------------------------------------------------
// (the family's own helpers, planes and inner launchers: unwrap.hpp)
bool unwrap_fast_supported(int h, int w);      // the shapes the consistency check takes; launch_unwrap floods every frame of any other
size_t unwrap_scratch_bytes(int B, int h, int w, ScratchRec *rec = nullptr);
// the priority flood launch_unwrap starts for an h x w frame: uint16 ranks and the batched flood in LDS, 32-bit ranks and the bitmap flood, or
// the generic one-wave flood; big_handback: the bitmap flood hands every frame to the generic one (a mask beyond its bitmap does so on its own)
enum UnwrapTier { UWT_RANK16 = 0, UWT_BITMAP = 1, UWT_GENERIC = 2 };
int unwrap_tier(int h, int w, bool big_handback = false);
void launch_unwrap(const float *wrapped, const float *quality, const uint8_t *mask, float *unwrapped, int32_t *parent,
                   void *scratch, int32_t *status, int B, int h, int w, hipStream_t st, hipEvent_t ev_mid,
                   hipEvent_t ev_flood = nullptr, bool big_handback = false, int32_t *need_buf = nullptr);      // need_buf [B]: enables the consistency check (k_unwrap_fast.hip)

// ---- k_fit.hip --------------------------------------------------------------------------------
// min_count: fitted (mask & finite) pixels needed (:1103); min_mask_count: mask pixels needed, NaN included (debug_ramp's own gate, :1364)
void launch_robust_polyfit(const float *z, const uint8_t *mask, int order, int iters, float c, int min_count, int min_mask_count, float *coef_out,
                           float *resid_out, int B, int h, int w, hipStream_t st, void *big_scratch = nullptr);
// the kernel launch_robust_polyfit starts for (B, h, w); big: scratch for the k_big.hip chain is at hand.  FITV_COL<RP>[_G4]: k_robust_polyfit_col<RP, 0 | 4>,
// FITV_GENERIC / FITV_GENERIC_DIV: k_robust_polyfit with the multiply-high row index / with a plain division (h * w * w >= 2^32)
enum FitVariant { FITV_BIG = 0, FITV_GENERIC, FITV_GENERIC_DIV, FITV_COL16, FITV_COL32, FITV_COL48, FITV_COL56, FITV_COL64, FITV_COL48_G4, FITV_COL56_G4,
                  FITV_COL64_G4, FITV_WIN16, FITV_WIN32, FITV_WIN48, FITV_WIN56, FITV_WIN32_G4, FITV_WIN48_G4, FITV_WIN56_G4, FITV_COUNT };
int polyfit_variant(int B, int h, int w, bool big, int *cols_pad_out = nullptr, int *groups_out = nullptr);   // the column kernels' launch geometry, if asked
// FITV_WIN<RP>[_G4]: k_robust_polyfit_colwin<RP, 0 | 4>, the window kernel that stands in for the plain column variant one ladder step up (64 -> 56,
// 56 -> 48, 48 -> 32, 32 -> 16, same GT) on frames whose mask rows span at most RP slots in every thread; -1: the variant has none
int polyfit_window_variant(int B, int h, int w, bool big);
struct FitSecond { int order, min_mask_count; float *resid_out; };      // the second fit of a chained launch: it fits the first fit's output plane
enum FitForce { FIT_WINDOW_ONLY = 1, FIT_PLAIN = 2 };
int launch_robust_polyfit_window(const float *z, const uint8_t *mask, int order, int iters, float c, int min_count, int min_mask_count, float *coef_out,
                                 float *resid_out, const FitSecond *second, int *need_flag, bool window, int force, int B, int h, int w, hipStream_t st,
                                 void *big_scratch);

// ---- k_holes.hip (hole stage, shape_ftp.py:1153-1204, :1770-1801; live only when reliable_smooth_sigma_px == 0) ----------------------
void launch_zeroed_keep_nan(const float *detr, const float *bg_med, const uint8_t *reliable, float *hmap, int B, int P, hipStream_t st);
void launch_hole_candidates(const float *hmap, const uint8_t *reliable, const float *dist, int ksize, float frac_thr, float min_dist, uint8_t *cand,
                            int B, int h, int w, hipStream_t st);
void launch_hole_tmp(const float *hmap, const uint8_t *reliable, const uint8_t *cand, const float *med, float *tmp, int B, int P, hipStream_t st);
void launch_hole_zin(float *tmp_zin, const float *fill, int B, int P, hipStream_t st);
void launch_hole_merge(float *hmap, const uint8_t *reliable, const uint8_t *cand, const float *zin, uint8_t *out_rel, int B, int P, hipStream_t st);

// ---- k_lab.hip (temperature modality: feature planes and colour support, temperature_sensor.py:278-293, :790-799) --------------------
constexpr int LAB_SHIFT = 12, LAB_SHIFT2 = 15, LAB_GAMMA_SHIFT = 3, LAB_CBRT_N = 256 * 3 / 2 * (1 << LAB_GAMMA_SHIFT);
struct LabCoef { int c[9]; int lscale, lshift; };     // sRGB -> XYZ / white point in 2^12 fixed point, rows X, Y, Z, columns R, G, B
void launch_feature_planes(const uint8_t *bgr, const uint16_t *gamma_tab, const uint16_t *cbrt_tab, const LabCoef &cf, bool blur, float *L, float *a,
                           float *b, float *gray, int H, int W, hipStream_t st);
void launch_color_support(const float *a, const float *b, const uint8_t *light_d, const uint8_t *roi_eff, const uint8_t *sat, float chroma_min,
                          float *chroma, uint8_t *support, size_t n, hipStream_t st);

// ---- k_post.hip -------------------------------------------------------------------------------
struct PostParams {
    double mm_per_px, depth_eps_mm, period_px;
    Curve force_curve;
    const CarrierGeom *pair_geom = nullptr;     // pair mode: per-frame period (mm_per_px = grating_pitch_mm / period, force_sensor.py:173-187)
    double grating_pitch_mm = 0.0;
};
void launch_contact_mask(const float *res, const uint8_t *reliable, const float *thr3, const int *rel_count, int *contact_count,
                         double min_frac, double max_frac, uint8_t *contact, float *thr_used, int B, int P, hipStream_t st);
void launch_background(const uint8_t *reliable, const uint8_t *contact_d, const int *rel_count, int *bg_count, uint8_t *background,
                       int B, int P, hipStream_t st);
void launch_sub_scalar_mask(const float *src, const float *scalar, const uint8_t *mask, float *z0, float *m_out, int B, int P,
                            hipStream_t st);
void launch_div_planes(const float *num, const float *den, float *out, int B, int P, hipStream_t st);
void launch_core_flip(float *hmap, const float *core_med, int *flipped, int B, int P, hipStream_t st);
void launch_frontier_compose(const float *hmap, const uint8_t *reliable, const uint8_t *roi, const float *dist_in, float band,
                             float *hfinal_z0, int B, int P, hipStream_t st);
void launch_finalize_unitless(const float *hfinal_z0, const float *smooth_num, const float *roi_den, const uint8_t *reliable,
                              const uint8_t *roi, const float *dist_out, float band, int use_band, float *unitless, int B, int P,
                              hipStream_t st);
void launch_to_mm(const float *unitless, const uint8_t *roi, Curve curve, int use_neg, float *depth, uint8_t *cand,
                  unsigned int *gmax_bits, int B, int P, hipStream_t st);
void launch_blob_filter(float *depth, const uint8_t *cand, const int32_t *labels, unsigned int *peak_bits,
                        const unsigned int *gmax_bits, double min_peak_mm, double rel_frac, uint8_t *kept, int B, int P,
                        hipStream_t st);
// the kernels launch_tail starts: k_tail (one workgroup per frame) or k_tail_part + k_tail_final (big_frames, and scratch of
// tail_scratch_bytes at hand).  force: 0 dispatch, else the tier itself (tests only; TAIL_BLOCKS without that scratch runs TAIL_FRAME)
enum TailTier { TAIL_FRAME = 1, TAIL_BLOCKS = 2 };
size_t tail_scratch_bytes(int B, int P);
int tail_tier(int B, int P, bool have_scratch, size_t scratch_bytes, int force = 0);
void launch_tail(const float *height_mm, const uint8_t *roi_or_null, const float *unitless_or_null, const uint8_t *roi_static,
                 PostParams pp, double *scalars, int nscal, double *out3_or_null, int B, int P, hipStream_t st, void *scratch = nullptr,
                 size_t scratch_bytes = 0, int force = 0);
void launch_fill_scalars(double *scalars, int nscal, const int *rel_count, const int *flipped, const float *amp_thr,
                         const float *contact_thr, const float *bg_med, const int *bad_count, int B, hipStream_t st);
void launch_mark_empty(const int *rel_count, int32_t *status, int B, hipStream_t st);
void launch_copy_out(const float *depth, const uint8_t *reliable, const int32_t *status, float *out_h, uint8_t *out_r, int B, int P,
                     hipStream_t st);

// ---- k_contacts.hip (per-contact read-out of the planes a predict leaves behind: vistaf_ftp_contacts) ------------------------------------
struct ContactScratch {
    int32_t *arg;                    // [B, P] by root: first pixel of the component's peak, then the contact's row (-1 beyond max_contacts)
    int32_t *list; int cap;          // [B, cap] kept roots of the frame, cap = contact_root_capacity(h, w)
    int *nroots, *nsel;              // [B] kept roots found / contacts of the frame (0 for a frame whose status is not OK)
    unsigned long long *selkey;      // [B, 64] peak bits << 32 | ~argmax of the ranked contacts
    unsigned long long *part;        // contact_part_words(max_batch, P) partial records
};
int contact_root_capacity(int h, int w);
size_t contact_part_words(int max_batch, int P);
bool ct_chunked(int B, int P);       // chunk tier (workgroups over CT_CHUNK pixels) instead of one workgroup per frame; k_tracks.hip splits the same frames
// contacts [B, K, nfield] double (nfield >= 13, fields as VISTAF_CONTACT_*), count [B], index [B, P] int8 or null
void launch_contacts(const float *depth, const uint8_t *kept, const int32_t *labels, const unsigned int *peak_bits, const int32_t *status,
                     PostParams pp, const ContactScratch &cs, int K, double *contacts, int nfield, int32_t *count, int8_t *index, int B, int h, int w,
                     hipStream_t st);

// ---- k_big.hip (large frames: selection and IRLS fit as chains of streaming kernels over all pixels of the batch)
size_t big_scratch_bytes(int B, int h, int w, ScratchRec *rec = nullptr);
bool big_frames(int B, int P);      // large_frame(P) in a batch small enough that one workgroup per frame cannot fill the chip
void launch_select_big(const float *vals, const uint8_t *mask, size_t mask_stride, const float *le_thr, bool use_abs, const float *reqs_dev, int nreq,
                       float *out, int *counts, int B, int P, void *scratch, hipStream_t st);
void launch_robust_polyfit_big(const float *z, const uint8_t *mask, int order, int iters, float c, int min_count, int min_mask_count, float *coef_out,
                               float *resid_out, int B, int h, int w, void *scratch, hipStream_t st);

// ---- k_tempmap.hip (map-domain stages of the temperature modality; parity unpinned, see the file)
using TmAff = Aff;                      // the inverse map of the two warps (common.hpp)
struct TmFuse { float color_lo, color_hi, low_th, high_th, final_lo, final_hi; };
void launch_tm_clamp(const float *m, const uint8_t *roi, float lo, float hi, float *out, size_t P, hipStream_t st);
void launch_tm_stats(const float *m, const uint8_t *roi, uint32_t *stats, size_t P, hipStream_t st);
void launch_tm_scale(const float *m, const uint8_t *roi, const uint32_t *stats, float *scaled, uint8_t *miss, size_t P, hipStream_t st);
void launch_tm_unscale(const float *m, const uint8_t *roi, const uint32_t *stats, const float *filled, float *out, size_t P, hipStream_t st);
void launch_tm_fuse(const uint8_t *roi, const float *wide, const float *color, const TmFuse &c, float *fin, uint8_t *source, unsigned long long *counts, size_t P,
                    hipStream_t st);
void launch_tm_zero_nonfinite(const float *m, float *out, size_t P, hipStream_t st);
void launch_tm_warp_linear(const float *src, float *dst, const TmAff &a, int h, int w, hipStream_t st);
void launch_tm_warp_nearest(const uint8_t *src, uint8_t *dst, const TmAff &a, int h, int w, hipStream_t st);
void launch_tm_mask_nan(const float *m, const uint8_t *keep, float *out, size_t P, hipStream_t st);

// ---- k_tempstats.hip (NumPy-exact mean / median / std / min / max / count of a float32 map over a valid mask, or isfinite when NULL):
// out[6] doubles on the device; scratch of tstats_scratch_bytes, plus big_scratch_bytes(1, h, w) when tstats_needs_big_scratch (else NULL)
size_t tstats_scratch_bytes(int h, int w, ScratchRec *rec = nullptr);
bool tstats_needs_big_scratch(int h, int w);
void launch_tstats(const float *map, const uint8_t *valid, int h, int w, void *scratch, void *big_scratch, double *out, hipStream_t st);

// ---- k_maskchain.hip (the three binary-mask chains of frames mask_chain_fits takes, mask_bits.hpp: the fused_masks tier) -------------------
// bad1 = iters dilations by se of valid & (img >= thr_hi | grad >= thr_g); bad_count[b] its pixels (a plain store)
void launch_bad_chain(const float *img, const float *grad, const uint8_t *valid, const float *thr_hi, const float *thr_g, const RowSpanSE &se,
                      int iters, uint8_t *bad1, int *bad_count, int B, int h, int w, hipStream_t st);
// rel0 = roi & finite(q) & (q >= amp_thr); reliable = erosion by `ball` (null: none) of roi & the largest component of roi & closing of rel0;
// rel_count[b] its pixels; status[b] = 1 where that is 0 and the status was 0.  area: a [B, P] plane, written at component roots only
void launch_reliable_chain(const float *quality, const uint8_t *roi, const float *amp_thr, const RowSpanSE &se_close, int close_iters,
                           const RowSpanSE *ball, int32_t *area, uint8_t *rel0, uint8_t *reliable, int *rel_count, int32_t *status, int B, int h,
                           int w, hipStream_t st);
// launch_contact_mask, iters dilations by se & reliable -> contact_d, launch_background
void launch_contact_chain(const float *res, const uint8_t *reliable, const float *thr3, const int *rel_count, double min_frac, double max_frac,
                          const RowSpanSE &se, int iters, int *contact_count, float *thr_used, uint8_t *contact_d, uint8_t *background,
                          int *bg_count, int B, int h, int w, hipStream_t st);

// ---- k_backend.hip (blob filter, force tail and output copy of LDS-sized frames in one launch: the fused_backend tier) -------------------
bool backend_fused_fits(int h, int w);      // the frames launch_cc_label labels with the mask staged in LDS, less the tail's reduction scratch
void launch_backend_fused(float *depth, const uint8_t *cand, const unsigned int *gmax_bits, const float *unitless, const uint8_t *roi_static,
                          const uint8_t *reliable, const int32_t *status, double min_peak_mm, double rel_frac, PostParams pp, int32_t *labels,
                          unsigned int *peak_bits, uint8_t *kept, double *scalars, int nscal, float *out_h, uint8_t *out_r, int B, int h, int w,
                          hipStream_t st);

// ---- k_pressure.hip (the pressure read-out, include/vistaf_pressure.h): its workspace of max_batch frames of h x w with pad_px of zero fill
size_t pressure_scratch_bytes(int B, int h, int w, int pad, ScratchRec *rec = nullptr);

// ---- k_outline.hip (the contact outline read-out, include_ext/vistaf_outline.h): the workspace its caller hands in, for B frames of h x w and
// tables of K rows.  Its three launches are made by vistaf_outline_measure itself
size_t outline_scratch_bytes(int B, int h, int w, int K, ScratchRec *rec = nullptr);

// ---- k_texture.hip (the surface texture read-out, include_ext/vistaf_texture.h): the workspace its caller hands in, for B frames, tables of K
// rows and windows of L lags (the half-plane sums of the autocorrelation).  Its four launches (k_texture_form, k_texture_stats, k_texture_acf,
// k_texture_rows) are made by vistaf_texture_measure itself
size_t texture_scratch_bytes(int B, int K, int L, ScratchRec *rec = nullptr);

}  // namespace vf
