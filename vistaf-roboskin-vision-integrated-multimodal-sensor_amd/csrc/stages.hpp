// The stages of a predict that choose between kernel tiers, as plain functions on planes of the caller's: post_demod and preprocess (api.hip)
// call them with the session's planes and its Tiers, the vistaf_ftp_test_* hooks (api_hooks.hip) with planes of a test.  One copy of each
// dispatch, so a direct test runs what a session runs.  Each function takes its inputs and outputs, a small struct of the scratch planes of its
// separate-kernel tier, the tier flags it depends on, and B, h, w, st; it returns the tier it ran or a negative VISTAF_E_* code.  Definitions:
// stages.hip.  Host only.
#pragma once
#include "host_util.hpp"

namespace vf {

// ---- constant tables and rules both files state
// cv2.getStructuringElement(MORPH_ELLIPSE, (k, k)), anchor at (k/2, k/2).  force_odd: the callers that first do `max(3, k | 1)`
// (shape_ftp.py:641-644, :756-758); the contact dilation passes DILATE_KERNEL_SIZE as it is (:1734), even sizes included.
int make_se(int k, RowSpanSE *se, bool force_odd = true);
// np.hanning(ph)[:,None] * np.hanning(pw)[None,:] in float32 (shape_ftp.py:800-807)
std::vector<float> hann_patch(int ph, int pw);
// every 1-D window a patch of up to pmax bins can need, as hann_patch() rounds it: hann(M)[i] at [M * pmax + i], M = 1..pmax (row 0 unused).
// The device forms each pair-mode sample's window from these (launch_build_tables).
std::vector<float> hann_table(int pmax);
inline int inpaint_range(double radius) { return std::min(100, std::max(1, cv_round(radius))); }      // cv::inpaint clamps the radius
// the longest Gaussian the blur kernels take
constexpr int GAUSS_MAX_TAPS = 511;
inline bool gauss_fits(double sigma) { return gauss_ksize(sigma) <= GAUSS_MAX_TAPS; }
int gauss_refused();      // the refusal of a sigma beyond it
// whether the element-wise passes around a blur of k taps run inside its tile (k_blurchain.hip): short kernels only, Tiers::fused_chains
inline bool fuses(bool fused_chains, int k) { return fused_chains && k > 0 && k <= GF_MAXK; }
inline bool fuses(const Tiers &tiers, int k) { return fuses(tiers.fused_chains != 0, k); }

// ---- Telea.  The launches of a stage: what the bad-pixel stage (clusters_ok) and the hole stage (!clusters_ok) of a session start for `tiers`,
// and what vistaf_ftp_test_inpaint runs under variants 0, 5 and 6.  Returns the plane [B] that marks the frames the whole-frame kernel took (null
// under Tiers::inpaint 1, where it takes them all).  ev_march (stage timing, may be null): recorded where the march proper starts.
struct InpaintBuffers { void *scratch, *cl_scratch, *win_scratch; int32_t *big_only; };
const int32_t *inpaint_dispatch(float *img, const uint8_t *bad, int range, const Tiers &tiers, bool clusters_ok, const InpaintBuffers &buf,
                                int32_t *status, int B, int h, int w, hipStream_t st, hipEvent_t ev_march);

// ---- the three binary-mask chains.  fused: the chain's bit of Tiers::fused_masks.  Each returns the tier taken -- 1 the one-launch kernel of
// k_maskchain.hip (frames mask_chain_fits takes), 0 the separate kernels.
int bad_chain_ops(int ksize, int iters);
int bad_mask_chain(const float *img, const float *grad, const uint8_t *valid, const float *thr_hi, const float *thr_g, const RowSpanSE &se, int ksize,
                   int iters, uint8_t *bad0, uint8_t *bad1, int *bad_count, bool fused, int B, int h, int w, hipStream_t st);
struct ReliableScratch {        // planes [B, P] of the separate kernels (rel1, rel2: bytes; labels, area, rowdist: int32; dist: float), cc_best [B]
    uint8_t *rel1, *rel2;
    int32_t *labels, *area, *rowdist;
    float *dist;
    unsigned long long *cc_best;
    uint16_t *morph_pre;
};
int reliable_mask_chain(const float *qual, const uint8_t *roi, const float *amp_thr, const RowSpanSE &se_close, int close_iters, int margin_px,
                        const ReliableScratch &ws, bool chamfer_twopass, uint8_t *rel0, uint8_t *reliable, int *rel_count, int32_t *status, bool fused,
                        int B, int h, int w, hipStream_t st);
struct ContactScratchPlanes { uint8_t *contact, *tmp; uint16_t *morph_pre; };      // planes [B, P] of the separate kernels
int contact_mask_chain(const float *resid, const uint8_t *reliable, const float *thr3, const int *rel_count, double min_frac, double max_frac,
                       const RowSpanSE &se, int iters, const ContactScratchPlanes &ws, int *contact_count, float *thr_used, uint8_t *contact_d,
                       uint8_t *background, int *bg_count, bool fused, int B, int h, int w, hipStream_t st);

// ---- reliable-only smoothing (shape_ftp.py:1753-1768): hmap = blur((detr - bg_med) * reliable) / blur(reliable) with the `k` taps at `taps`.
// Tier 3: k == 0, no smoothing, the unreliable pixels are zeroed and NaN stays NaN; 2: one tile kernel (fuses(fused_chains, k)); 1: subtract,
// two blurs, divide.
struct SmoothScratch { float *z0, *mplane, *num, *den, *tmp; };      // planes [B, P] of tier 1
int smooth_stage(const float *detr, const float *bg_med, const uint8_t *reliable, const float *taps, int k, const SmoothScratch &ws, float *hmap,
                 bool fused_chains, bool gauss_strip, int B, int h, int w, hipStream_t st);

// ---- core threshold, then the median of the elements up to it: one chained launch where the keys stay in registers (returns 2), else two
// launches (1).  req_chain: the two requests of the chained launch; req_core, req_med: those of the two.  chain: scratch of the k_big.hip
// chains or null.
int core_medians(const float *hmap, const uint8_t *reliable, const float *req_chain, const float *req_core, const float *req_med, float *core_thr,
                 float *core_med, void *chain, bool select_resident, int B, int P, hipStream_t st);

// ---- frontier taper, composition, unreliable-region smoothing, clamp, mm curve (shape_ftp.py:1770-1873).  dist_in / dist_out: distance of a pixel
// to the outside / the inside of `reliable`; taper_band: `band`, or 1 with use_band == 0.  Tier 2: one kernel (fuses(fused_chains, k)), which
// reads dist_out and writes depth in one pass, so the two must be apart; 1: compose, blur, finalize, curve, where dist_out may be `depth` and
// must not be a plane of `ws`.  ev_mm (stage timing, may be null): recorded where the mm curve starts (after the one kernel of tier 2).
struct HeightScratch { float *z0f, *snum, *tmp; };      // planes [B, P] of tier 1; snum, tmp: only with k > 0
int height_finish_stage(const float *hmap, const uint8_t *reliable, const uint8_t *roi, const float *dist_in, float taper_band, const float *roi_den,
                        const float *dist_out, float band, int use_band, const Curve &curve, int use_neg, const float *taps, int k,
                        const HeightScratch &ws, float *unitless, float *depth, uint8_t *cand, unsigned int *gmax_bits, bool fused_chains,
                        bool gauss_strip, hipEvent_t ev_mm, int B, int h, int w, hipStream_t st);

// ---- blob filter, force tail + arg-extrema, copy to the caller's planes (shape_ftp.py:1850-1873, multimodal_sensor.py:388-419).  Tier 2: frames
// whose label forest fits LDS (fused_backend and backend_fused_fits): one launch; 1: labels, blob filter, tail, copy.  chain, chain_bytes: the
// tail's chain scratch (null: its one-workgroup kernel).  A session also has its per-frame records filled here, between the tail and the copy
// where they always were: rec (may be null), and ev_tail (stage timing, may be null), recorded where the tail starts (after the one launch of
// tier 2, so that the whole launch counts as mm_blob).
struct FrameRecords { const int *rel_count, *flipped; const float *amp_thr, *contact_thr, *bg_med; const int *bad_count; };      // launch_fill_scalars
int backend_stage(float *depth, const uint8_t *cand, const unsigned int *gmax_bits, const float *unitless, const uint8_t *roi_static,
                  const uint8_t *reliable, const int32_t *status, double min_peak_mm, double rel_frac, const PostParams &pp, int32_t *labels,
                  unsigned int *peak_bits, uint8_t *kept, double *scalars, int nscal, float *out_h, uint8_t *out_r, void *chain, size_t chain_bytes,
                  bool fused_backend, const FrameRecords *rec, hipEvent_t ev_tail, int B, int h, int w, hipStream_t st);

}  // namespace vf
