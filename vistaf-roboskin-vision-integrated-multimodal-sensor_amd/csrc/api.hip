// C ABI of the MI355X-native VISTAF FTP path (see include/vistaf_ftp.h).  Host orchestration only:
// every image operation runs in a HIP kernel of this library; the host builds constant tables
// (Gaussian taps, Hann window, DFT twiddles, ROI / apodisation planes) in double precision.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "host_util.hpp"
#include "mask_rules.hpp"      // chamfer_ball
#include "mask_bits.hpp"       // mask_chain_fits

using namespace vf;
#include "test_hooks.h"
#include "test_hooks_masks.h"
#include "test_hooks_dft.h"
#include "test_hooks_gauss.h"
#include "test_hooks_fit.h"
#include "test_hooks_post.h"
#ifdef VISTAF_DEBUG
namespace vf { void telea_debug_dump(); void telea_window_debug_dump(int B); void telea_window_mw_debug_dump(int B); void fit_debug_dump(); void unwrap_big_debug_dump(); void unwrap_batch_debug_dump(); }
#endif

static thread_local std::string g_err;
static int fail(int code, const std::string &msg) { g_err = msg; return code; }
namespace vf { int set_error(int code, const std::string &msg) { return fail(code, msg); } }   // for the other translation units of the ABI

namespace {

struct GKern { float *d = nullptr; int k = 0; };

enum Stage { ST_GRAY_BAD = 0, ST_INPAINT, ST_PREPROC, ST_DEMOD, ST_RELIABLE, ST_UNWRAP_RANK, ST_UNWRAP, ST_UNWRAP_TREE, ST_DETREND, ST_SMOOTH_FLIP, ST_COMPOSE, ST_MM_BLOB,
             ST_TAIL, ST_COUNT };
const char *kStageNames[ST_COUNT] = {"gray+badpix", "inpaint (k_telea_window_mw)", "illum+blur+apod+median", "pruned-dft demod", "reliable mask",
                                     "unwrap check (k_unwrap_fast)", "unwrap flood (fallback)", "unwrap tree (fallback)", "detrend (3x IRLS)", "smooth+flip", "frontier+compose", "mm+blob filter", "tail"};

}  // namespace

struct vistaf_ftp_handle {
    vistaf_ftp_config cfg;
    int h = 0, w = 0, P = 0, cx = 0, cy = 0, r = 0, maxB = 0;
    Curve hcurve, fcurve;
    int use_neg = 1;
    bool have_ref = false;

    // static planes
    uint8_t *roi = nullptr, *valid = nullptr;
    float *apo = nullptr, *roi_den = nullptr;
    GKern g_illum, g_pre, g_qual, g_rel, g_unrel;
    RowSpanSE se_bad, se_close, se_contact;

    // reference state (session mode: one carrier, tables shared by the batch)
    double peak_x = 0, peak_y = 0, kx = 0, ky = 0, period = 0, mm_per_px = 0;
    int Hf = 0, Wf = 0, ph = 0, pw = 0, pmax = 0;
    double2 *Ex = nullptr, *Ey = nullptr, *Gx = nullptr, *Gy = nullptr, *cref = nullptr;
    float *win = nullptr, *amp_ref = nullptr;
    CarrierGeom *geom = nullptr;                      // [1] session carrier, device
    // carrier search (full spectrum), allocated on first use for `search_cap` frames
    double2 *Exf = nullptr, *Eyf = nullptr, *search_tmp = nullptr;
    double *search_mag = nullptr, *search_peaks = nullptr;
    int search_cap = 0;
    // uncached-pair mode (vistaf_ftp_predict_pairs): per-frame carriers, tables and reference fields, allocated on first use
    CarrierGeom *pgeom = nullptr;
    double2 *pEx = nullptr, *pEy = nullptr, *pGx = nullptr, *pGy = nullptr, *pcref = nullptr;
    float *pamp_ref = nullptr, *pwin = nullptr, *hann_tab = nullptr;     // pwin: [maxB][pmax^2] per-sample windows; hann_tab: hann(M)[i] at [M * pmax + i]
    bool pairs_ready = false;
    Tiers tiers;                                       // kernel tier selection (test hook; defaults = production kernels)
    bool keep_planes = false;                          // test hook: also write planes that only the parity tests read (float64 field)

    // workspace (maxB frames)
    struct Named { void *p; size_t bytes; bool per_frame; };   // bytes: per frame, or of the whole plane when it is static
    std::map<std::string, Named> named;
    DeviceAllocs allocs;
    float *img, *grad, *tmpf, *blurA, *inorm, *iw, *amp, *prod, *quality, *wrapped, *unwrapped, *phase1, *resid0, *detr, *z0, *mplane,
        *num, *den, *hmap, *dist, *z0f, *snum, *unitless, *depth;
    double2 *field, *patch;
    double2 *tmpT;
    uint8_t *bad0, *bad1, *rel0, *rel1, *rel2, *reliable, *contact, *contact_d, *background, *cand, *kept;
    uint8_t *out_rel = nullptr, *hole_cand = nullptr;      // hole stage only (reliable_smooth_sigma_px == 0)
    float *hole_med = nullptr, *hole_fill = nullptr;
    int32_t *labels, *area, *rowdist, *parent;
    unsigned int *peak_bits;    // by component ROOT only: the component's peak (float bits) of the last predict.  Other entries are 0 after the separate
                                // kernels and stale after the fused back end (which sets the roots only): never index it by pixel
    uint16_t *morph_pre;
    void *inpaint_scratch, *inpaint_cl_scratch, *inpaint_win_scratch, *unwrap_scratch;
    void *big_scratch = nullptr;      // k_big.hip (large_frame), else null
    size_t big_scratch_bytes = 0;
    int32_t *fit_need;          // [max_batch] of the window kernel of the detrend's chained first two fits: 1 the frame's mask rows did not fit the window and the plain-size kernel ran it, 0 the window kernel did, -1 never written
    int32_t *unwrap_need;       // [max_batch] 1: the frame went through the priority flood, 0: the consistency check settled it
    // small per-frame arrays
    float *thr_hi, *thr_g, *mu, *amp_thr, *thr3, *thr_used, *bg_med, *core_thr, *core_med, *coef;
    int *cnt_a, *cnt_valid, *rel_count, *contact_count, *bg_count, *bad_count, *flipped;
    unsigned int *gmax;
    int32_t *status;
    int32_t *big_only;                  // [maxB] frames handed from the big-cluster march to the whole-frame kernel (launch_inpaint_big_handback)
    unsigned long long *cc_best;        // [maxB] largest-component key of launch_cc_largest on large frames
    double *scalars;
    float *req_hi, *req_g, *req_med, *req_amp, *req_contact, *req_core, *req_core_med;   // device percentile requests

    // per-contact read-out (vistaf_ftp_contacts): buffers sized by max_batch, and what the last predict was
    ContactScratch contacts_ws{};
    int last_batch = 0;                 // 0: no predict yet
    bool last_pairs = false;

    bool timing = false;
    hipEvent_t ev[ST_COUNT + 1];
    bool ev_made = false;
    float stage_ms[ST_COUNT];
};

namespace {

template <typename T>
int dalloc(vistaf_ftp_handle *hd, T **p, size_t count, const char *name = nullptr, size_t per_frame = 0)
{
    const int rc = hd->allocs.alloc(p, count);
    if (!rc && name) hd->named[name] = {*p, per_frame, true};
    return rc;
}

int make_gkern(vistaf_ftp_handle *hd, double sigma, GKern *g)
{
    g->k = 0; g->d = nullptr;
    if (!(sigma > 0)) return 0;
    if (gauss_ksize(sigma) > 511) return fail(VISTAF_E_INVALID, "gaussian sigma too large (ksize > 511)");
    const std::vector<float> f = gauss_taps(sigma);
    TRY(hd->allocs.upload(&g->d, f));
    g->k = (int)f.size();
    return 0;
}

// cv2.getStructuringElement(MORPH_ELLIPSE, (k, k)), anchor at (k/2, k/2).  force_odd: the callers that first do `max(3, k | 1)`
// (shape_ftp.py:641-644, :756-758); the contact dilation passes DILATE_KERNEL_SIZE as it is (:1734), even sizes included.
int make_se(int k, RowSpanSE *se, bool force_odd = true)
{
    if (force_odd) k = std::max(3, k | 1);
    if (k > 33) return fail(VISTAF_E_INVALID, "structuring element larger than 33");
    *se = ellipse_se(k);
    return 0;
}

void blur(vistaf_ftp_handle *hd, const float *src, float *dst, const GKern &g, int B, hipStream_t st)
{
    launch_gauss_blur(src, hd->tmpf, dst, g.d, g.k, B, hd->h, hd->w, st, hd->tiers.gauss_strip != 0);
}

// whether the element-wise passes around this blur run inside its tile (k_blurchain.hip): short kernels only, Tiers::fused_chains
bool fuses(const vistaf_ftp_handle *hd, const GKern &g) { return hd->tiers.fused_chains && g.k > 0 && g.k <= GF_MAXK; }

// scratch of the k_big.hip chains, or null when the one-workgroup kernels are to run (Tiers::big_chain)
void *chain_scratch(const vistaf_ftp_handle *hd) { return hd->tiers.big_chain ? hd->big_scratch : nullptr; }

float q32_of(double pct) { return (float)pct / 100.0f; }   // np.true_divide(q, float32(100))

// launch_select with the session's chain scratch and selection tier
void select(vistaf_ftp_handle *hd, const float *vals, const uint8_t *mask, size_t mask_stride, const float *le_thr, bool use_abs, const float *reqs, int nreq,
            float *out, int *counts, int B, hipStream_t st)
{
    launch_select(vals, mask, mask_stride, le_thr, use_abs, reqs, nreq, out, counts, B, hd->P, st, chain_scratch(hd), hd->tiers.select_resident != 0);
}

// the frames of a predict or a reference against the session's size: a format the size cannot hold or a pointer below the format's
// alignment is refused here, before any launch (frame_layout, host_util.hpp)
int check_frames(const vistaf_ftp_handle *hd, int format, const void *a, const void *b)
{
    const FrameLayout fl = frame_layout(format, hd->h, hd->w);
    if (fl.refusal) return fail(VISTAF_E_INVALID, std::string(fl.refusal) + " (format " + std::to_string(format) + ", frames of " + std::to_string(hd->h) + " x " + std::to_string(hd->w) + ")");
    if (((uintptr_t)a | (uintptr_t)b) & (uintptr_t)(fl.align - 1))
        return fail(VISTAF_E_INVALID, "frame format " + std::to_string(format) + " needs frames aligned to " + std::to_string(fl.align) + " bytes");
    return 0;
}

// The Telea launches of a stage: what the bad-pixel stage (clusters_ok) and the hole stage (!clusters_ok) of a session start for `tiers`, and what
// vistaf_ftp_test_inpaint runs under variants 0, 5 and 6.  Returns the plane [B] that marks the frames the whole-frame kernel took (null
// under Tiers::inpaint 1, where it takes them all).  ev_march (stage timing, may be null): recorded where the march proper starts.
struct InpaintBuffers { void *scratch, *cl_scratch, *win_scratch; int32_t *big_only; };
const int32_t *inpaint_dispatch(float *img, const uint8_t *bad, int range, const Tiers &tiers, bool clusters_ok, const InpaintBuffers &buf,
                                int32_t *status, int B, int h, int w, hipStream_t st, hipEvent_t ev_march)
{
    // default (Tiers::inpaint 2): the frame-window kernel (LDS-resident march), then the whole-frame kernel for the frames it hands
    // back; 1: whole-frame kernel only; 0: cluster by cluster -- every independent cluster of hole pixels on its own wave, in an LDS
    // window when it fits, on the frame's global planes otherwise.  At 224 x 224 the hole pixels form ONE cluster per frame, so the
    // frame window is the better tool; frames much larger than its capacity (14 464 cells) -- the native 1182 x 1182 crops -- never
    // fit one window, and there the crests are ~60 px apart: many independent clusters (march of eight native crops: 1.95 s with the
    // whole-frame kernel, 0.54 s with LDS clusters + whole-frame kernel for the rest, 18 ms since k_inpaint_big.hip: DESIGN.md section 5a).
    int mode = tiers.inpaint;
    if (clusters_ok && mode == 2 && (size_t)h * w > (size_t)8 * inpaint_window_cells_cap()) mode = 0;
    if (clusters_ok && mode == 0 && inpaint_clusters_supported(range)) {
        // every independent cluster of hole pixels on its own wave: LDS windows for those that fit, the frame's global planes for the rest
        uint8_t *bad_big = nullptr;
        ClusterPlanes left;
        launch_inpaint_clusters(img, bad, range, buf.cl_scratch, &bad_big, &left, B, h, w, st);
        if (ev_march) hipEventRecord(ev_march, st);      // (after the LDS cluster pass: its bookkeeping counts as mask work)
        launch_inpaint_big_clusters(img, bad_big, range, buf.scratch, status, left, B, h, w, st, tiers.big_queue_lds != 0, tiers.big_gq_cap);
        // a frame whose big-cluster queue overflowed (status 2) goes whole to the whole-frame kernel, whose queue cannot overflow
        // (~0.25 s per native crop: a rare path); the other frames only pay for the hand-back launch and two early-exit grids
        if (!tiers.big_fallback) return nullptr;
        launch_inpaint_big_handback(status, buf.big_only, B, st);
        launch_inpaint_telea(img, bad_big, range, buf.scratch, status, buf.big_only, B, h, w, st);
        return buf.big_only;
    }
    const int32_t *only = nullptr;
    if (ev_march && mode == 1) hipEventRecord(ev_march, st);
    if (mode != 1) only = launch_inpaint_window(img, bad, range, buf.win_scratch, B, h, w, st, ev_march, tiers.telea_two_tier != 0, tiers.telea_mw != 0);
    launch_inpaint_telea(img, bad, range, buf.scratch, status, only, B, h, w, st);
    return only;
}
InpaintBuffers inpaint_buffers(const vistaf_ftp_handle *hd) { return {hd->inpaint_scratch, hd->inpaint_cl_scratch, hd->inpaint_win_scratch, hd->big_only}; }

// ---- the three binary-mask chains: what a session launches for them, and what the vistaf_ftp_test_*_chain hooks run on planes of the caller.
// fused: the chain's bit of Tiers::fused_masks.  Each returns the tier taken -- 1 the one-launch kernel of k_maskchain.hip (frames
// mask_chain_fits takes), 0 the separate kernels -- or a negative VISTAF_E_* code.
int bad_chain_ops(int ksize, int iters) { return ksize > 1 ? std::max(0, iters) : 0; }
int bad_mask_chain(const float *img, const float *grad, const uint8_t *valid, const float *thr_hi, const float *thr_g, const RowSpanSE &se, int ksize,
                   int iters, uint8_t *bad0, uint8_t *bad1, int *bad_count, bool fused, int B, int h, int w, hipStream_t st)
{
    const int P = h * w;
    if (fused && mask_chain_fits(MCH_BAD, h, w, se, bad_chain_ops(ksize, iters))) {
        launch_bad_chain(img, grad, valid, thr_hi, thr_g, se, bad_chain_ops(ksize, iters), bad1, bad_count, B, h, w, st);
        return 1;
    }
    launch_bad_flags(img, grad, valid, thr_hi, thr_g, bad0, B, P, st);
    uint8_t *src = bad0, *dst = bad1;
    if (ksize > 1)
        for (int it = 0; it < iters; it++) { launch_morph(src, dst, B, h, w, se, true, nullptr, nullptr, st); std::swap(src, dst); }
    if (src != bad1) HIPCHK(hipMemcpyAsync(bad1, src, (size_t)B * P, hipMemcpyDeviceToDevice, st));
    launch_count_u8(bad1, bad_count, B, P, st);
    return 0;
}

struct ReliableScratch {        // planes [B, P] of the separate kernels (rel1, rel2: bytes; labels, area, rowdist: int32; dist: float), cc_best [B]
    uint8_t *rel1, *rel2;
    int32_t *labels, *area, *rowdist;
    float *dist;
    unsigned long long *cc_best;
    uint16_t *morph_pre;
};
int reliable_mask_chain(const float *qual, const uint8_t *roi, const float *amp_thr, const RowSpanSE &se_close, int close_iters, int margin_px,
                        const ReliableScratch &ws, bool chamfer_twopass, uint8_t *rel0, uint8_t *reliable, int *rel_count, int32_t *status, bool fused,
                        int B, int h, int w, hipStream_t st)
{
    const int P = h * w;
    // erode_by_distance (shape_ftp.py:368-377): keep a pixel when its 3x3-chamfer distance to the nearest zero pixel exceeds the margin,
    // i.e. when no zero pixel lies in the chamfer ball of that radius: an erosion by the ball (image border: nothing to erode, as in
    // cv::distanceTransform where the outside holds no zero pixel).  The ball is a symmetric row-span element: bit-plane kernel.
    RowSpanSE ball;
    const bool have_ball = margin_px > 0 && chamfer_ball((float)margin_px, &ball);
    if (fused && mask_chain_fits(MCH_RELIABLE, h, w, se_close, 2 * std::max(0, close_iters), (float)margin_px)) {
        launch_reliable_chain(qual, roi, amp_thr, se_close, std::max(0, close_iters), have_ball ? &ball : nullptr, ws.area, rel0, reliable, rel_count,
                              status, B, h, w, st);
        return 1;
    }
    launch_threshold_mask(qual, roi, amp_thr, rel0, B, P, st);
    {
        // MORPH_CLOSE with n iterations = n dilations then n erosions; the eroded-ROI mask applies to the result
        uint8_t *src = rel0, *dst = ws.rel1;
        if (close_iters >= 1 && 2 * close_iters <= 4) {
            int ops[4];
            for (int it = 0; it < close_iters; it++) { ops[it] = 1; ops[close_iters + it] = 0; }
            launch_morph_seq(rel0, ws.rel1, ws.rel2, B, h, w, se_close, ops, 2 * close_iters, roi, nullptr, st, ws.morph_pre);
            src = ws.rel1;
        } else {
            // rel1 / rel2 alternate; rel0 keeps the thresholded mask (the "rel0" intermediate)
            for (int it = 0; it < 2 * close_iters; it++) {
                const bool dil = it < close_iters;
                launch_morph(src, dst, B, h, w, se_close, dil, it == 2 * close_iters - 1 ? roi : nullptr, nullptr, st, ws.morph_pre);
                src = dst;
                dst = dst == ws.rel1 ? ws.rel2 : ws.rel1;
            }
        }
        launch_cc_label(src, ws.labels, B, h, w, st);
        launch_cc_largest(ws.labels, ws.area, ws.cc_best, roi, ws.rel2, B, P, st);
    }
    if (margin_px > 0) {
        if (have_ball) launch_morph(ws.rel2, reliable, B, h, w, ball, false, nullptr, nullptr, st, ws.morph_pre);
        else {
            launch_chamfer(ws.rel2, false, ws.rowdist, ws.dist, B, h, w, margin_px + 1, st, chamfer_twopass);
            launch_erode_by_dist(ws.dist, ws.rel2, (float)margin_px, reliable, B, P, st);
        }
    } else HIPCHK(hipMemcpyAsync(reliable, ws.rel2, (size_t)B * P, hipMemcpyDeviceToDevice, st));
    launch_count_u8(reliable, rel_count, B, P, st);
    launch_mark_empty(rel_count, status, B, st);
    return 0;
}

struct ContactScratchPlanes { uint8_t *contact, *tmp; uint16_t *morph_pre; };      // planes [B, P] of the separate kernels
int contact_mask_chain(const float *resid, const uint8_t *reliable, const float *thr3, const int *rel_count, double min_frac, double max_frac,
                       const RowSpanSE &se, int iters, const ContactScratchPlanes &ws, int *contact_count, float *thr_used, uint8_t *contact_d,
                       uint8_t *background, int *bg_count, bool fused, int B, int h, int w, hipStream_t st)
{
    const int P = h * w;
    if (fused && mask_chain_fits(MCH_CONTACT, h, w, se, std::max(0, iters))) {
        launch_contact_chain(resid, reliable, thr3, rel_count, min_frac, max_frac, se, std::max(0, iters), contact_count, thr_used, contact_d,
                             background, bg_count, B, h, w, st);
        return 1;
    }
    launch_contact_mask(resid, reliable, thr3, rel_count, contact_count, min_frac, max_frac, ws.contact, thr_used, B, P, st);
    // cv2.dilate with 0 iterations is a copy (contact is inside reliable already)
    if (iters <= 0) HIPCHK(hipMemcpyAsync(contact_d, ws.contact, (size_t)B * P, hipMemcpyDeviceToDevice, st));
    else if (iters <= 4) {
        int ops[4] = {1, 1, 1, 1};
        launch_morph_seq(ws.contact, contact_d, ws.tmp, B, h, w, se, ops, iters, nullptr, reliable, st, ws.morph_pre);
    } else {
        uint8_t *src = ws.contact, *dst = contact_d;
        uint8_t *bufs[2] = {contact_d, ws.tmp};
        for (int it = 0; it < iters; it++) {
            dst = bufs[it & 1];
            launch_morph(src, dst, B, h, w, se, true, nullptr, it == iters - 1 ? reliable : nullptr, st, ws.morph_pre);
            src = dst;
        }
        if (src != contact_d) HIPCHK(hipMemcpyAsync(contact_d, src, (size_t)B * P, hipMemcpyDeviceToDevice, st));
    }
    launch_background(reliable, contact_d, rel_count, bg_count, background, B, P, st);
    return 0;
}

// preprocessing shared by reference and deformed frames: frames -> iw (apodised, normalised) and mu
// frames2 (pair mode, when the workspace holds 2 * nframes): a second set of nframes frames preprocessed in the SAME launches, as frames
// [nframes, 2 * nframes) of every plane -- the one-wave-per-frame march then runs once over twice as many CUs instead of twice
void preprocess(vistaf_ftp_handle *hd, const void *frames, int format, int nframes, hipStream_t st, bool timed, const void *frames2 = nullptr)
{
    const vistaf_ftp_config &c = hd->cfg;
    int h = hd->h, w = hd->w, P = hd->P;
    if (timed) hipEventRecord(hd->ev[ST_GRAY_BAD], st);
    launch_to_gray(frames, format, hd->img, nframes, P, st, w);
    if (frames2) launch_to_gray(frames2, format, hd->img + (size_t)nframes * P, nframes, P, st, w);
    const int B = frames2 ? 2 * nframes : nframes;
    const bool fused_bad = c.bad_pixel_enable && (hd->tiers.fused_masks & MCH_BAD) &&
                           mask_chain_fits(MCH_BAD, h, w, hd->se_bad, bad_chain_ops(c.bad_dilate_ksize, c.bad_dilate_iters));
    if (!fused_bad) hipMemsetAsync(hd->bad_count, 0, sizeof(int) * B, st);      // (the fused chain stores the count)
    if (c.bad_pixel_enable) {
        launch_sobel_mag(hd->img, hd->grad, B, h, w, st);
        select(hd, hd->img, hd->valid, 0, nullptr, false, hd->req_hi, 1, hd->thr_hi, hd->cnt_valid, B, st);
        select(hd, hd->grad, hd->valid, 0, nullptr, false, hd->req_g, 1, hd->thr_g, nullptr, B, st);
        (void)bad_mask_chain(hd->img, hd->grad, hd->valid, hd->thr_hi, hd->thr_g, hd->se_bad, c.bad_dilate_ksize, c.bad_dilate_iters, hd->bad0, hd->bad1,
                             hd->bad_count, fused_bad, B, h, w, st);
        inpaint_dispatch(hd->img, hd->bad1, std::min(100, std::max(1, cv_round((double)c.bad_inpaint_radius))),   // cv::inpaint clamps the radius
                         hd->tiers, true, inpaint_buffers(hd), hd->status, B, h, w, st, timed ? hd->ev[ST_INPAINT] : nullptr);
    } else if (timed) hipEventRecord(hd->ev[ST_INPAINT], st);
    if (timed) hipEventRecord(hd->ev[ST_PREPROC], st);
    blur(hd, hd->img, hd->blurA, hd->g_illum, B, st);
    if (fuses(hd, hd->g_pre)) launch_illum_pre_apod(hd->img, hd->blurA, hd->apo, hd->iw, hd->g_pre.d, hd->g_pre.k, B, h, w, st);
    else {
        launch_illum_norm(hd->img, hd->blurA, hd->inorm, B, P, st);
        const float *in = hd->inorm;
        if (hd->g_pre.k) { blur(hd, hd->inorm, hd->blurA, hd->g_pre, B, st); in = hd->blurA; }
        launch_mul_static(in, hd->apo, hd->iw, B, P, st);
    }
    select(hd, hd->iw, hd->valid, 0, nullptr, false, hd->req_med, 1, hd->mu, nullptr, B, st);
}

// np.hanning(ph)[:,None] * np.hanning(pw)[None,:] in float32 (shape_ftp.py:800-807); np.hanning(M) = 0.5 + 0.5*cos(pi*n/(M-1)), n = 1-M, 3-M, ...
std::vector<float> hann_patch(int ph, int pw)
{
    auto hann = [](int M, int i) -> float { return M == 1 ? 1.0f : (float)(0.5 + 0.5 * std::cos(3.14159265358979323846 * (double)(1 - M + 2 * i) / (double)(M - 1))); };
    std::vector<float> win((size_t)ph * pw);
    for (int a = 0; a < ph; a++)
        for (int c = 0; c < pw; c++) win[(size_t)a * pw + c] = hann(ph, a) * hann(pw, c);
    return win;
}

// scale, calibration and carriers of the force tail and the per-contact read-out; pair_geom: per-frame carriers (pair mode) or null
PostParams post_params(const vistaf_ftp_handle *hd, const CarrierGeom *pair_geom)
{
    PostParams pp;
    pp.mm_per_px = hd->mm_per_px; pp.depth_eps_mm = hd->cfg.depth_eps_mm; pp.period_px = hd->period; pp.force_curve = hd->fcurve;
    pp.pair_geom = pair_geom; pp.grating_pitch_mm = hd->cfg.grating_pitch_mm;
    return pp;
}

// the stage-timing events, created when a timed predict first needs them
void ensure_events(vistaf_ftp_handle *hd)
{
    if (hd->ev_made) return;
    for (int i = 0; i <= ST_COUNT; i++) hipEventCreate(&hd->ev[i]);
    hd->ev_made = true;
}

}  // namespace

extern "C" {

int vistaf_ftp_abi_version(void) { return VISTAF_FTP_ABI_VERSION; }
const char *vistaf_ftp_last_error(void) { return g_err.c_str(); }

int vistaf_ftp_default_config(vistaf_ftp_config *c)
{
    if (!c) return fail(VISTAF_E_INVALID, "null config");
    memset(c, 0, sizeof(*c));
    c->patch_half_width_bins = 10; c->dc_exclusion = 10; c->fft_pad_px = 96; c->roi_erode_px = 0; c->apod_taper_px = 120;
    c->reliable_edge_margin_px = 6; c->poly_order = 2; c->frontier_zero_band_px = 200; c->valid_close_kernel = 7;
    c->valid_close_iters = 1; c->bad_pixel_enable = 1; c->bad_dilate_ksize = 5; c->bad_dilate_iters = 1; c->bad_inpaint_radius = 3;
    c->dilate_kernel_size = 15; c->dilate_iters = 2; c->n_fft_peaks = 12; c->plane_order_for_removal = 1; c->irls_iters = 6;
    c->pre_blur_sigma_px = 1.5; c->amp_valid_percentile = 25.0; c->quality_smooth_sigma_px = 6.0; c->reliable_smooth_sigma_px = 2.5;
    c->illum_sigma_px = 45.0; c->bad_intensity_percentile = 99.9; c->bad_gradient_percentile = 99.7; c->contact_core_percentile = 8.0;
    c->contact_percentile = 92.0; c->min_contact_frac = 0.002; c->max_contact_frac = 0.40; c->unreliable_smooth_sigma_px = 9.0;
    c->contact_blob_min_peak_mm = 0.1; c->contact_blob_min_peak_rel_frac = 1.0 / 3.0; c->peak_max_dy_from_center = 0.12;
    c->irls_c = 4.685; c->grating_pitch_mm = 2.0; c->depth_eps_mm = 0.01;
    c->hole_neighborhood_px = 11; c->hole_min_dist_px = 4; c->inpaint_radius = 5; c->hole_known_fraction = 0.70;
    return 0;
}

void vistaf_ftp_destroy(vistaf_ftp_handle *hd)
{
    if (!hd) return;
    hd->allocs.free_all();
    if (hd->ev_made) for (int i = 0; i <= ST_COUNT; i++) hipEventDestroy(hd->ev[i]);
    delete hd;
}

int vistaf_ftp_create(const vistaf_ftp_config *cfg, int h, int w, int cx, int cy, int r, int max_batch,
                      const vistaf_curve *height_curve, int use_negated_height, const vistaf_curve *force_curve,
                      vistaf_ftp_handle **out)
{
    if (!cfg || !out || !height_curve || !force_curve) return fail(VISTAF_E_INVALID, "null argument");
    if (h < 8 || w < 8 || max_batch < 1 || r < 1) return fail(VISTAF_E_INVALID, "bad geometry");
    if (height_curve->type < 0 || height_curve->type > 5 || force_curve->type < 0 || force_curve->type > 5)
        return fail(VISTAF_E_INVALID, "Unknown model type in calibration");
    if (cfg->poly_order < 1 || cfg->poly_order > 2 || cfg->plane_order_for_removal < 0 || cfg->plane_order_for_removal > 2)
        return fail(VISTAF_E_INVALID, "polynomial order must be 1 or 2 (plane_order_for_removal: 0 = no pre-removal)");
    if (cfg->irls_iters < 1) return fail(VISTAF_E_INVALID, "irls_iters must be >= 1 (robust_polyfit2d binds no coefficients otherwise)");
    if (cfg->n_fft_peaks < 1 || cfg->n_fft_peaks > 64) return fail(VISTAF_E_INVALID, "n_fft_peaks must be 1..64");
    int bwp = std::max(3, cfg->patch_half_width_bins);
    if (2 * bwp + 1 > 255) return fail(VISTAF_E_INVALID, "patch too wide");
    Created<vistaf_ftp_handle> own(new vistaf_ftp_handle(), vistaf_ftp_destroy);
    vistaf_ftp_handle *hd = own.get();
    DeviceAllocs &mem = hd->allocs;
    hd->cfg = *cfg; hd->h = h; hd->w = w; hd->P = h * w; hd->cx = cx; hd->cy = cy; hd->r = r; hd->maxB = max_batch;
    hd->hcurve = Curve{height_curve->type, height_curve->a, height_curve->b, height_curve->c};
    hd->fcurve = Curve{force_curve->type, force_curve->a, force_curve->b, force_curve->c};
    hd->use_neg = use_negated_height ? 1 : 0;
    int P = hd->P;
    size_t n = (size_t)max_batch * P;
    // static planes (shape_ftp.py:383-403, :1519-1528)
    std::vector<uint8_t> roi(P), valid(P);
    std::vector<float> apo(P), roif(P);
    int r_valid = std::max(0, r - cfg->roi_erode_px);
    double r_in = std::max(0.0, (double)(r - cfg->apod_taper_px));
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            long d2 = (long)(x - cx) * (x - cx) + (long)(y - cy) * (y - cy);
            roi[(size_t)y * w + x] = d2 <= (long)r_valid * r_valid;
            double d = std::sqrt((double)d2);
            float a = 0.f;
            if (d <= r_in) a = 1.0f;
            else if (d <= r && cfg->apod_taper_px > 0) {
                double t = (d - r_in) / std::max(1e-6, (double)cfg->apod_taper_px);
                a = (float)(0.5 * (1.0 + std::cos(3.14159265358979323846 * t)));
            }
            apo[(size_t)y * w + x] = a;
            valid[(size_t)y * w + x] = a > 1e-6f;
            roif[(size_t)y * w + x] = roi[(size_t)y * w + x] ? 1.f : 0.f;
        }
    TRY(mem.upload(&hd->roi, roi)); TRY(mem.upload(&hd->valid, valid)); TRY(mem.upload(&hd->apo, apo));
    hd->named["roi"] = {hd->roi, (size_t)P, false};
    TRY(make_gkern(hd, cfg->illum_sigma_px, &hd->g_illum));
    if (!hd->g_illum.k) return fail(VISTAF_E_INVALID, "illum_sigma_px must be > 0");
    TRY(make_gkern(hd, cfg->pre_blur_sigma_px, &hd->g_pre));
    TRY(make_gkern(hd, cfg->quality_smooth_sigma_px, &hd->g_qual));
    TRY(make_gkern(hd, cfg->reliable_smooth_sigma_px, &hd->g_rel));
    TRY(make_gkern(hd, cfg->unreliable_smooth_sigma_px, &hd->g_unrel));
    TRY(make_se(cfg->bad_dilate_ksize, &hd->se_bad));
    TRY(make_se(cfg->valid_close_kernel, &hd->se_close));
    {   // cv2.getStructuringElement(ELLIPSE, (k,k)) with k as given (shape_ftp.py:1734)
        int k = cfg->dilate_kernel_size;
        if (k < 1 || k > 33) return fail(VISTAF_E_INVALID, "dilate_kernel_size out of range");
        TRY(make_se(k, &hd->se_contact, false));
    }
    if (!(cfg->reliable_smooth_sigma_px > 0)) {     // the hole stage is live (shape_ftp.py:1770-1801)
        if (cfg->hole_neighborhood_px < 1 || cfg->hole_neighborhood_px > 255 || cfg->hole_min_dist_px < 0 || cfg->inpaint_radius < 1 ||
            !(cfg->hole_known_fraction >= 0.0))
            return fail(VISTAF_E_INVALID, "hole-stage constants out of range");
    }
    // workspace
#define PLANE(T, name) TRY(dalloc(hd, &hd->name, n, #name, (size_t)P * sizeof(T)))
    PLANE(float, img); PLANE(float, grad); PLANE(float, tmpf); PLANE(float, blurA); PLANE(float, inorm); PLANE(float, iw);
    PLANE(float, amp); PLANE(float, prod); PLANE(float, quality); PLANE(float, wrapped); PLANE(float, unwrapped); PLANE(float, phase1);
    PLANE(float, resid0); PLANE(float, detr); PLANE(float, z0); PLANE(float, mplane); PLANE(float, num); PLANE(float, den);
    PLANE(float, hmap); PLANE(float, dist); PLANE(float, z0f); PLANE(float, snum); PLANE(float, unitless); PLANE(float, depth);
    PLANE(double2, field);
    PLANE(uint8_t, bad0); PLANE(uint8_t, bad1); PLANE(uint8_t, rel0); PLANE(uint8_t, rel1); PLANE(uint8_t, rel2); PLANE(uint8_t, reliable);
    PLANE(uint8_t, contact); PLANE(uint8_t, contact_d); PLANE(uint8_t, background); PLANE(uint8_t, cand); PLANE(uint8_t, kept);
    if (!(cfg->reliable_smooth_sigma_px > 0)) { PLANE(uint8_t, out_rel); PLANE(uint8_t, hole_cand); }
    PLANE(int32_t, labels); PLANE(int32_t, area); PLANE(int32_t, rowdist); PLANE(int32_t, parent);
    PLANE(unsigned int, peak_bits);
    PLANE(uint16_t, morph_pre);
#undef PLANE
    {
        void *p = nullptr;
        TRY(dalloc(hd, (uint8_t **)&p, inpaint_scratch_bytes(max_batch, h, w))); hd->inpaint_scratch = p;
        TRY(dalloc(hd, (uint8_t **)&p, inpaint_cl_scratch_bytes(max_batch, h, w))); hd->inpaint_cl_scratch = p;
        TRY(dalloc(hd, (uint8_t **)&p, inpaint_win_scratch_bytes(max_batch))); hd->inpaint_win_scratch = p;
        TRY(dalloc(hd, (uint8_t **)&p, unwrap_scratch_bytes(max_batch, h, w))); hd->unwrap_scratch = p;
        if (large_frame((size_t)P)) {
            hd->big_scratch_bytes = big_scratch_bytes(max_batch, h, w);
            TRY(dalloc(hd, (uint8_t **)&p, hd->big_scratch_bytes)); hd->big_scratch = p;
        }
        TRY(dalloc(hd, &hd->unwrap_need, (size_t)max_batch, "unwrap_need", sizeof(int32_t)));
        HIPCHK(hipMemset(hd->unwrap_need, 0xff, (size_t)max_batch * sizeof(int32_t)));        // -1: never written (the check is off or does not cover this frame size)
        TRY(dalloc(hd, &hd->fit_need, (size_t)max_batch, "fit_need", sizeof(int32_t)));
        HIPCHK(hipMemset(hd->fit_need, 0xff, (size_t)max_batch * sizeof(int32_t)));           // -1: never written (no window instance for this frame size, or "fit_window" = 0)
    }
    int pmax = 2 * bwp + 1;
    hd->pmax = pmax;
    TRY(dalloc(hd, &hd->patch, (size_t)max_batch * pmax * pmax, "patch", (size_t)pmax * pmax * sizeof(double2)));
    TRY(dalloc(hd, &hd->tmpT, (size_t)max_batch * (size_t)std::max(h, w) * pmax));
    TRY(dalloc(hd, &hd->Ex, (size_t)w * pmax)); TRY(dalloc(hd, &hd->Gx, (size_t)w * pmax));
    TRY(dalloc(hd, &hd->Ey, (size_t)h * pmax)); TRY(dalloc(hd, &hd->Gy, (size_t)h * pmax));
    TRY(dalloc(hd, &hd->win, (size_t)pmax * pmax)); TRY(dalloc(hd, &hd->geom, 1));
    TRY(dalloc(hd, &hd->cref, (size_t)P)); TRY(dalloc(hd, &hd->amp_ref, (size_t)P));
    hd->named["cref"] = {hd->cref, (size_t)P * sizeof(double2), false}; hd->named["amp_ref"] = {hd->amp_ref, (size_t)P * sizeof(float), false};
    size_t mb = max_batch;
    TRY(dalloc(hd, &hd->thr_hi, mb)); TRY(dalloc(hd, &hd->thr_g, mb)); TRY(dalloc(hd, &hd->mu, mb)); TRY(dalloc(hd, &hd->amp_thr, mb));
    TRY(dalloc(hd, &hd->thr3, mb * 3)); TRY(dalloc(hd, &hd->thr_used, mb)); TRY(dalloc(hd, &hd->bg_med, mb));
    TRY(dalloc(hd, &hd->core_thr, mb)); TRY(dalloc(hd, &hd->core_med, mb)); TRY(dalloc(hd, &hd->coef, mb * 6));
    TRY(dalloc(hd, &hd->cnt_a, mb)); TRY(dalloc(hd, &hd->cnt_valid, mb)); TRY(dalloc(hd, &hd->rel_count, mb));
    TRY(dalloc(hd, &hd->contact_count, mb)); TRY(dalloc(hd, &hd->bg_count, mb)); TRY(dalloc(hd, &hd->bad_count, mb));
    TRY(dalloc(hd, &hd->flipped, mb)); TRY(dalloc(hd, &hd->gmax, mb)); TRY(dalloc(hd, &hd->status, mb)); TRY(dalloc(hd, &hd->cc_best, mb));
    TRY(dalloc(hd, &hd->big_only, mb));
    TRY(dalloc(hd, &hd->scalars, mb * VISTAF_NSCALARS));
    TRY(dalloc(hd, &hd->hole_med, mb)); TRY(dalloc(hd, &hd->hole_fill, mb));
    {
        ContactScratch &cs = hd->contacts_ws;
        cs.cap = contact_root_capacity(h, w);
        TRY(dalloc(hd, &cs.arg, n)); TRY(dalloc(hd, &cs.list, mb * cs.cap)); TRY(dalloc(hd, &cs.nroots, mb)); TRY(dalloc(hd, &cs.nsel, mb));
        TRY(dalloc(hd, &cs.selkey, mb * VISTAF_MAX_CONTACTS)); TRY(dalloc(hd, &cs.part, contact_part_words(max_batch, P)));
    }
    hd->named["mu"] = {hd->mu, sizeof(float), true}; hd->named["thr_hi"] = {hd->thr_hi, sizeof(float), true}; hd->named["thr_g"] = {hd->thr_g, sizeof(float), true};
    hd->named["coef"] = {hd->coef, 6 * sizeof(float), true}; hd->named["thr3"] = {hd->thr3, 3 * sizeof(float), true};
    hd->named["thr_used"] = {hd->thr_used, sizeof(float), true};
    hd->named["core_thr"] = {hd->core_thr, sizeof(float), true}; hd->named["core_med"] = {hd->core_med, sizeof(float), true};
    TRY(mem.upload(&hd->req_hi, std::vector<float>{q32_of(cfg->bad_intensity_percentile)}));
    TRY(mem.upload(&hd->req_g, std::vector<float>{q32_of(cfg->bad_gradient_percentile)}));
    TRY(mem.upload(&hd->req_med, std::vector<float>{-1.0f}));
    TRY(mem.upload(&hd->req_amp, std::vector<float>{q32_of(cfg->amp_valid_percentile)}));
    TRY(mem.upload(&hd->req_contact, std::vector<float>{q32_of(cfg->contact_percentile), q32_of(95.0), q32_of(98.0)}));
    TRY(mem.upload(&hd->req_core, std::vector<float>{q32_of(cfg->contact_core_percentile)}));
    TRY(mem.upload(&hd->req_core_med, std::vector<float>{q32_of(cfg->contact_core_percentile), -1.0f}));      // the chained pair: core threshold, median below it
    // den of the ROI-wide masked smooth is frame independent: blur(roi) + 1e-6 (shape_ftp.py:1146, :1821)
    TRY(dalloc(hd, &hd->roi_den, (size_t)P));
    if (hd->g_unrel.k) {
        float *tmp_roi = nullptr;
        TRY(mem.upload(&tmp_roi, roif));
        launch_gauss_rows(tmp_roi, hd->tmpf, hd->g_unrel.d, hd->g_unrel.k, 1, h, w, 0);
        launch_gauss_cols(hd->tmpf, hd->roi_den, hd->g_unrel.d, hd->g_unrel.k, 1, h, w, 0);
        std::vector<float> hden(P);
        HIPCHK(hipMemcpy(hden.data(), hd->roi_den, P * sizeof(float), hipMemcpyDeviceToHost));
        for (int i = 0; i < P; i++) hden[i] = hden[i] + 1e-6f;
        HIPCHK(hipMemcpy(hd->roi_den, hden.data(), P * sizeof(float), hipMemcpyHostToDevice));
    }
    hd->Hf = h + 2 * std::max(0, cfg->fft_pad_px);
    hd->Wf = w + 2 * std::max(0, cfg->fft_pad_px);
    HIPCHK(hipDeviceSynchronize());
    *out = own.release();
    return 0;
}

// carrier search + tables + demodulation of nb reference frames that preprocess() has left in hd->iw / hd->mu (shape_ftp.py:867-961).
// Asynchronous; geometry lands in geom_dev[0..nb).  ph / pw: patch size the DFT launches use (session mode: read back from the geometry
// between the two halves; pair mode: every sample's own ph x pw inside the full 2*bw+1 square, clipped patches included).
static int reference_search(vistaf_ftp_handle *hd, int nb, CarrierGeom *geom_dev, hipStream_t st)
{
    const vistaf_ftp_config &c = hd->cfg;
    const int h = hd->h, w = hd->w, Hf = hd->Hf, Wf = hd->Wf, pad = std::max(0, c.fft_pad_px);
    if (hd->search_cap < nb) {
        int rc;
        if (!hd->Exf) {
            if ((rc = dalloc(hd, &hd->Exf, (size_t)w * (Wf / 2 + 1))) || (rc = dalloc(hd, &hd->Eyf, (size_t)Hf * h))) return rc;
            launch_build_full_tables(hd->Exf, hd->Eyf, h, w, pad, Hf, Wf, st);
        }
        // The search buffers grow geometrically (at least doubling, at most max_batch frames) and the previous set is RELEASED here, not
        // kept until destroy: a caller whose pair batches grow (1, 2, ..., max_batch) holds one set of <= max_batch frames at any time
        // instead of piling up O(max_batch^2) frames of Hf x Wf doubles.  (The first pair-mode call and every growth allocate, i.e. synchronise.)
        const int cap = std::min(std::max(nb, 2 * hd->search_cap), std::max(nb, hd->maxB));
        if (hd->search_cap > 0) {
            HIPCHK(hipStreamSynchronize(st));          // earlier searches on this stream may still read the old set
            hd->allocs.release(hd->search_tmp); hd->allocs.release(hd->search_mag); hd->allocs.release(hd->search_peaks);
            hd->search_tmp = nullptr; hd->search_mag = nullptr; hd->search_peaks = nullptr; hd->search_cap = 0;
        }
        if ((rc = dalloc(hd, &hd->search_tmp, (size_t)cap * h * (Wf / 2 + 1) + 64)) || (rc = dalloc(hd, &hd->search_mag, (size_t)cap * Hf * Wf)) ||
            (rc = dalloc(hd, &hd->search_peaks, (size_t)cap * 192)))
            return rc;
        hd->search_cap = cap;
    }
    const int npk = c.n_fft_peaks;                  // 1..64, checked by vistaf_ftp_create
    launch_dft_full_mag(hd->iw, hd->mu, hd->Exf, hd->Eyf, hd->search_tmp, hd->search_mag, nb, h, w, Hf, Wf, st);
    launch_top_peaks(hd->search_mag, nb, Hf, Wf, c.dc_exclusion, npk, hd->search_peaks, st);
    launch_carrier_choose(hd->search_peaks, npk, hd->search_mag, Hf, Wf, std::max(3, c.patch_half_width_bins), c.peak_max_dy_from_center, geom_dev, nb, st);
    return 0;
}

int vistaf_ftp_set_reference(vistaf_ftp_handle *hd, const void *d_ref, int format, void *stream)
{
    if (!hd || !d_ref) return fail(VISTAF_E_INVALID, "null argument");
    TRY(check_frames(hd, format, d_ref, nullptr));
    hipStream_t st = (hipStream_t)stream;
    const vistaf_ftp_config &c = hd->cfg;
    int h = hd->h, w = hd->w, Hf = hd->Hf, Wf = hd->Wf, pad = std::max(0, c.fft_pad_px);
    hd->have_ref = false;
    HIPCHK(hipMemsetAsync(hd->status, 0, sizeof(int32_t) * hd->maxB, st));
    preprocess(hd, d_ref, format, 1, st, false);
    int rc = reference_search(hd, 1, hd->geom, st);
    if (rc) return rc;
    CarrierGeom g;
    HIPCHK(hipMemcpyAsync(&g, hd->geom, sizeof(g), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (!g.ok) return fail(VISTAF_E_NOCARRIER, "no carrier peak in the reference spectrum");
    hd->peak_x = g.peak_x; hd->peak_y = g.peak_y; hd->kx = g.kx; hd->ky = g.ky;
    hd->ph = g.ph; hd->pw = g.pw;
    {
        std::vector<float> win = hann_patch(g.ph, g.pw);
        HIPCHK(hipMemcpyAsync(hd->win, win.data(), win.size() * sizeof(float), hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));         // `win` is a host temporary
    }
    launch_build_tables(hd->geom, 0, hd->Ex, hd->Ey, hd->Gx, hd->Gy, 0, 0, 1, h, w, pad, Hf, Wf, hd->pmax, st);
    launch_dft_forward(hd->iw, hd->mu, hd->Ex, hd->Ey, 0, 0, hd->win, hd->tmpT, hd->patch, hd->pmax * hd->pmax, 1, h, w, hd->ph, hd->pw, st, 0, hd->tiers.dft_staged != 0);
    launch_dft_inverse(hd->patch, hd->pmax * hd->pmax, hd->Gx, hd->Gy, 0, 0, hd->tmpT, hd->cref, hd->amp_ref, nullptr, nullptr, 0, nullptr, nullptr,
                       1, h, w, hd->ph, hd->pw, st, nullptr, hd->tiers.dft_staged != 0);
    HIPCHK(hipStreamSynchronize(st));
    // period estimate (shape_ftp.py:2015-2027) and scale (force_sensor.py:173-187); carrier is locked so k_def == k_ref
    hd->period = g.period;
    hd->mm_per_px = hd->period > 1e-12 ? c.grating_pitch_mm / hd->period : 0.0;
    hd->have_ref = true;
    return 0;
}

int vistaf_ftp_get_reference_info(const vistaf_ftp_handle *hd, double *o)
{
    if (!hd || !o) return fail(VISTAF_E_INVALID, "null argument");
    if (!hd->have_ref) return fail(VISTAF_E_STATE, "set_reference has not been called");
    o[0] = hd->peak_x; o[1] = hd->peak_y; o[2] = hd->kx; o[3] = hd->ky; o[4] = hd->Hf; o[5] = hd->Wf; o[6] = hd->period; o[7] = hd->mm_per_px;
    return 0;
}

// Everything after the demodulation (shape_ftp.py:1655-2037 + the force tail), shared by the session mode and the uncached-pair mode.
// In: hd->amp-independent planes `prod` (amp_ref * amp_def) and `wrapped`.  pair_geom: per-frame carriers (pair mode) or null.
static int post_demod(vistaf_ftp_handle *hd, int B, float *d_height_mm, uint8_t *d_reliable, double *d_scalars, int32_t *d_status,
                      const CarrierGeom *pair_geom, hipStream_t st, const int *bad_count = nullptr)
{
    if (!bad_count) bad_count = hd->bad_count;
    const vistaf_ftp_config &c = hd->cfg;
    int h = hd->h, w = hd->w, P = hd->P;
    bool timed = hd->timing;

    // ---- reliable mask (shape_ftp.py:739-775)
    if (timed) hipEventRecord(hd->ev[ST_RELIABLE], st);
    if (hd->g_qual.k) blur(hd, hd->prod, hd->quality, hd->g_qual, B, st);
    else HIPCHK(hipMemcpyAsync(hd->quality, hd->prod, (size_t)B * P * sizeof(float), hipMemcpyDeviceToDevice, st));
    const float *qual = hd->quality;
    select(hd, qual, hd->roi, 0, nullptr, false, hd->req_amp, 1, hd->amp_thr, nullptr, B, st);
    {
        const ReliableScratch ws = {hd->rel1, hd->rel2, hd->labels, hd->area, hd->rowdist, hd->dist, hd->cc_best, hd->morph_pre};
        const int tier = reliable_mask_chain(qual, hd->roi, hd->amp_thr, hd->se_close, c.valid_close_iters, c.reliable_edge_margin_px, ws,
                                             hd->tiers.chamfer_twopass != 0, hd->rel0, hd->reliable, hd->rel_count, hd->status,
                                             (hd->tiers.fused_masks & MCH_RELIABLE) != 0, B, h, w, st);
        if (tier < 0) return tier;
    }

    // ---- unwrap (shape_ftp.py:1702)
    if (timed) hipEventRecord(hd->ev[ST_UNWRAP_RANK], st);
    launch_unwrap(hd->wrapped, qual, hd->reliable, hd->unwrapped, hd->parent, hd->unwrap_scratch, hd->status, B, h, w, st,
                  timed ? hd->ev[ST_UNWRAP_TREE] : nullptr, timed ? hd->ev[ST_UNWRAP] : nullptr, hd->tiers.big_flood_handback != 0, hd->tiers.unwrap_fast ? hd->unwrap_need : nullptr);

    // ---- plane removal + two-pass detrend (shape_ftp.py:1706, :1716-1751)
    if (timed) hipEventRecord(hd->ev[ST_DETREND], st);
    const bool fit_win = hd->tiers.fit_window != 0;
    if (c.plane_order_for_removal > 0) {
        // debug_ramp gates on the reliable count, NaN pixels included (:1364-1366), robust_polyfit2d on 200 finite samples (:1103); the first detrend
        // fit takes its output under the same mask: one chained launch where a column kernel applies, else the two launches
        const FitSecond detrend1 = {c.poly_order, 0, hd->resid0};
        launch_robust_polyfit_window(hd->unwrapped, hd->reliable, c.plane_order_for_removal, c.irls_iters, (float)c.irls_c, 200, 500, hd->coef, hd->phase1, &detrend1,
                                     hd->fit_need, fit_win, 0, B, h, w, st, chain_scratch(hd));
    } else {   // no debug_ramp (the constants of Code/phase_to_height.py): the unwrapped phase goes to the detrend as it is
        HIPCHK(hipMemcpyAsync(hd->phase1, hd->unwrapped, (size_t)B * P * sizeof(float), hipMemcpyDeviceToDevice, st));
        launch_robust_polyfit(hd->phase1, hd->reliable, c.poly_order, c.irls_iters, (float)c.irls_c, 200, 0, hd->coef, hd->resid0, B, h, w, st, chain_scratch(hd));
    }
    select(hd, hd->resid0, hd->reliable, (size_t)P, nullptr, true, hd->req_contact, 3, hd->thr3, nullptr, B, st);
    {
        const ContactScratchPlanes ws = {hd->contact, hd->cand, hd->morph_pre};      // cand is free until the blob filter
        const int tier = contact_mask_chain(hd->resid0, hd->reliable, hd->thr3, hd->rel_count, c.min_contact_frac, c.max_contact_frac, hd->se_contact,
                                            c.dilate_iters, ws, hd->contact_count, hd->thr_used, hd->contact_d, hd->background, hd->bg_count,
                                            (hd->tiers.fused_masks & MCH_CONTACT) != 0, B, h, w, st);
        if (tier < 0) return tier;
    }
    // (the window kernel alone does not pay on a single fit, DESIGN.md section 6: the third fit keeps the plain kernel)
    launch_robust_polyfit(hd->phase1, hd->background, c.poly_order, c.irls_iters, (float)c.irls_c, 200, 0, hd->coef, hd->detr, B, h, w, st, chain_scratch(hd));
    select(hd, hd->detr, hd->background, (size_t)P, nullptr, false, hd->req_med, 1, hd->bg_med, nullptr, B, st);

    // ---- reliable-only smoothing + sign flip (shape_ftp.py:1753-1768)
    if (timed) hipEventRecord(hd->ev[ST_SMOOTH_FLIP], st);
    const bool smooth_rel = hd->g_rel.k > 0;
    if (fuses(hd, hd->g_rel)) launch_smooth_reliable(hd->detr, hd->bg_med, hd->reliable, hd->hmap, hd->g_rel.d, hd->g_rel.k, B, h, w, st);
    else if (smooth_rel) {
        launch_sub_scalar_mask(hd->detr, hd->bg_med, hd->reliable, hd->z0, hd->mplane, B, P, st);
        blur(hd, hd->z0, hd->num, hd->g_rel, B, st);
        blur(hd, hd->mplane, hd->den, hd->g_rel, B, st);
        launch_div_planes(hd->num, hd->den, hd->hmap, B, P, st);
    } else launch_zeroed_keep_nan(hd->detr, hd->bg_med, hd->reliable, hd->hmap, B, P, st);      // NaN stays NaN: the hole stage below is live
    // core threshold, then the median of the elements up to it: one chained launch where the keys stay in registers, else two launches
    float *const core_outs[2] = {hd->core_thr, hd->core_med};
    if (select_variant(B, P, 2, chain_scratch(hd) != nullptr, hd->tiers.select_resident != 0) < SELV_RES16 ||
        launch_select_chained(hd->hmap, hd->reliable, (size_t)P, false, hd->req_core_med, 2, core_outs, nullptr, B, P, st) < 0) {
        select(hd, hd->hmap, hd->reliable, (size_t)P, nullptr, false, hd->req_core, 1, hd->core_thr, nullptr, B, st);
        select(hd, hd->hmap, hd->reliable, (size_t)P, hd->core_thr, false, hd->req_med, 1, hd->core_med, nullptr, B, st);
    }
    launch_core_flip(hd->hmap, hd->core_med, hd->flipped, B, P, st);

    // ---- internal holes of the reliable region (shape_ftp.py:1770-1801): with the smoothing every reliable pixel is finite here and
    // upstream's compute_internal_holes_within_mask returns at its first test; without it the unreached pixels are NaN
    const uint8_t *orel = hd->reliable;                      // output_reliable (:1801)
    if (!smooth_rel) {
        const int ksz = std::max(3, c.hole_neighborhood_px | 1);
        launch_chamfer(hd->reliable, false, hd->rowdist, hd->dist, B, h, w, c.hole_min_dist_px + 1, st, hd->tiers.chamfer_twopass != 0);
        launch_hole_candidates(hd->hmap, hd->reliable, hd->dist, ksz, (float)c.hole_known_fraction, (float)c.hole_min_dist_px, hd->hole_cand, B, h, w, st);
        select(hd, hd->hmap, hd->reliable, (size_t)P, nullptr, false, hd->req_med, 1, hd->hole_med, nullptr, B, st);
        launch_hole_tmp(hd->hmap, hd->reliable, hd->hole_cand, hd->hole_med, hd->z0, B, P, st);
        select(hd, hd->z0, hd->reliable, (size_t)P, nullptr, false, hd->req_med, 1, hd->hole_fill, nullptr, B, st);
        launch_hole_zin(hd->z0, hd->hole_fill, B, P, st);
        {
            const int range = std::min(100, std::max(1, cv_round((double)c.inpaint_radius)));
            inpaint_dispatch(hd->z0, hd->hole_cand, range, hd->tiers, false, inpaint_buffers(hd), hd->status, B, h, w, st, nullptr);
        }
        launch_hole_merge(hd->hmap, hd->reliable, hd->hole_cand, hd->z0, hd->out_rel, B, P, st);
        orel = hd->out_rel;
    }

    // ---- frontier taper, composition, unreliable-region smoothing, clamp (shape_ftp.py:1770-1841)
    if (timed) hipEventRecord(hd->ev[ST_COMPOSE], st);
    bool use_band = c.frontier_zero_band_px > 0;
    float band = (float)c.frontier_zero_band_px;
    // both distance transforms of the reliable mask (to its outside for the taper, to its inside for the final blend) in one launch; the
    // second one lands in a plane that is idle at this point (`area` is the integer temporary): `depth`, which to_mm writes below, or, when
    // the fused compose runs, `snum`, which only the kernel sequence writes -- the fused kernel reads the distance and writes `depth` in one
    // pass, and with the two apart none of its pointers alias
    const bool fuse_compose = fuses(hd, hd->g_unrel);      // then the mm curve runs in the same kernel and counts as composition
    float *dist2 = fuse_compose ? hd->snum : hd->depth;
    if (use_band) launch_chamfer_pair(orel, hd->rowdist, hd->dist, hd->area, dist2, B, h, w, c.frontier_zero_band_px + 2, st, hd->tiers.chamfer_twopass != 0);
    else HIPCHK(hipMemsetAsync(hd->dist, 0x7f, (size_t)B * P * sizeof(float), st));   // huge distance: taper weight 1
    if (fuse_compose)
        launch_compose_finalize_mm(hd->hmap, orel, hd->roi, hd->dist, use_band ? band : 1.0f, hd->roi_den, use_band ? dist2 : hd->dist, band,
                                   use_band ? 1 : 0, hd->hcurve, hd->use_neg, hd->unitless, hd->depth, hd->cand, hd->gmax, hd->g_unrel.d, hd->g_unrel.k,
                                   B, h, w, st);
    else {
        launch_frontier_compose(hd->hmap, orel, hd->roi, hd->dist, use_band ? band : 1.0f, hd->z0f, B, P, st);
        if (hd->g_unrel.k) blur(hd, hd->z0f, hd->snum, hd->g_unrel, B, st);
        launch_finalize_unitless(hd->z0f, hd->g_unrel.k ? hd->snum : nullptr, hd->roi_den, orel, hd->roi, use_band ? hd->depth : hd->dist, band, use_band ? 1 : 0,
                                 hd->unitless, B, P, st);
    }

    // ---- unitless -> mm, blob filter (shape_ftp.py:1850-1873)
    if (timed) hipEventRecord(hd->ev[ST_MM_BLOB], st);
    if (!fuse_compose) launch_to_mm(hd->unitless, hd->roi, hd->hcurve, hd->use_neg, hd->depth, hd->cand, hd->gmax, B, P, st);
    const PostParams pp = post_params(hd, pair_geom);
    // frames whose label forest fits LDS: labels, blob filter, force tail + arg-extrema and the copy to the caller's planes in one launch
    // (stage timing: the whole launch counts as mm_blob, and the tail stage below is left with k_fill_scalars and the two small copies)
    const bool fused_backend = hd->tiers.fused_backend && backend_fused_fits(h, w);
    if (fused_backend)
        launch_backend_fused(hd->depth, hd->cand, hd->gmax, hd->unitless, hd->roi, orel, hd->status, c.contact_blob_min_peak_mm,
                             c.contact_blob_min_peak_rel_frac, pp, hd->labels, hd->peak_bits, hd->kept, hd->scalars, VISTAF_NSCALARS, d_height_mm,
                             d_reliable, B, h, w, st);
    else {
        launch_cc_label(hd->cand, hd->labels, B, h, w, st);
        launch_blob_filter(hd->depth, hd->cand, hd->labels, hd->peak_bits, hd->gmax, c.contact_blob_min_peak_mm,
                           c.contact_blob_min_peak_rel_frac, hd->kept, B, P, st);
    }

    // ---- force tail (multimodal_sensor.py:388-419) + arg-extrema
    if (timed) hipEventRecord(hd->ev[ST_TAIL], st);
    if (!fused_backend)
        launch_tail(hd->depth, nullptr, hd->unitless, hd->roi, pp, hd->scalars, VISTAF_NSCALARS, nullptr, B, P, st, chain_scratch(hd),
                    hd->big_scratch_bytes);
    launch_fill_scalars(hd->scalars, VISTAF_NSCALARS, hd->rel_count, hd->flipped, hd->amp_thr, hd->thr_used, hd->bg_med, bad_count, B, st);
    if (!fused_backend) launch_copy_out(hd->depth, orel, hd->status, d_height_mm, d_reliable, B, P, st);
    if (d_scalars) HIPCHK(hipMemcpyAsync(d_scalars, hd->scalars, sizeof(double) * VISTAF_NSCALARS * B, hipMemcpyDeviceToDevice, st));
    if (d_status) HIPCHK(hipMemcpyAsync(d_status, hd->status, sizeof(int32_t) * B, hipMemcpyDeviceToDevice, st));
    if (timed) {
        hipEventRecord(hd->ev[ST_COUNT], st);
        hipEventSynchronize(hd->ev[ST_COUNT]);
        for (int i = 0; i < ST_COUNT; i++) hipEventElapsedTime(&hd->stage_ms[i], hd->ev[i], hd->ev[i + 1]);
    }
#ifdef VISTAF_DEBUG
    if (getenv("VISTAF_TELEA_DBG")) { hipStreamSynchronize(st); telea_debug_dump(); telea_window_debug_dump(B); telea_window_mw_debug_dump(B); fit_debug_dump(); unwrap_big_debug_dump(); unwrap_batch_debug_dump(); }
#endif
    if (const int rc = launch_ok("launch")) return rc;
    hd->last_batch = B; hd->last_pairs = pair_geom != nullptr;
    return 0;
}

int vistaf_ftp_predict_batch(vistaf_ftp_handle *hd, const void *d_frames, int format, int B, float *d_height_mm, uint8_t *d_reliable,
                             double *d_scalars, int32_t *d_status, void *stream)
{
    if (!hd || !d_frames) return fail(VISTAF_E_INVALID, "null argument");
    if (!hd->have_ref) return fail(VISTAF_E_STATE, "set_reference has not been called");
    if (B < 1 || B > hd->maxB) return fail(VISTAF_E_STATE, "batch exceeds max_batch");
    TRY(check_frames(hd, format, d_frames, nullptr));
    if (!(hd->period > 1e-12)) return fail(VISTAF_E_STATE, "Invalid estimated_grating_period_px");
    hipStream_t st = (hipStream_t)stream;
    int h = hd->h, w = hd->w;
    bool timed = hd->timing;
    if (timed) ensure_events(hd);
    HIPCHK(hipMemsetAsync(hd->status, 0, sizeof(int32_t) * B, st));

    preprocess(hd, d_frames, format, B, st, timed);

    // ---- demodulation, carrier locked to the reference (shape_ftp.py:1643-1653, :1681-1689)
    if (timed) hipEventRecord(hd->ev[ST_DEMOD], st);
    launch_dft_forward(hd->iw, hd->mu, hd->Ex, hd->Ey, 0, 0, hd->win, hd->tmpT, hd->patch, hd->pmax * hd->pmax, B, h, w, hd->ph, hd->pw, st, 0, hd->tiers.dft_staged != 0);
    launch_dft_inverse(hd->patch, hd->pmax * hd->pmax, hd->Gx, hd->Gy, 0, 0, hd->tmpT, hd->keep_planes ? hd->field : nullptr, hd->amp, hd->cref,
                       hd->amp_ref, 0, hd->prod, hd->wrapped, B, h, w, hd->ph, hd->pw, st, nullptr, hd->tiers.dft_staged != 0);
    return post_demod(hd, B, d_height_mm, d_reliable, d_scalars, d_status, nullptr, st);
}

// Uncached pairs: every sample brings its own reference frame, as Code/height_to_force.py:384 runs shape_ftp.main per image (reference
// demodulation with carrier search :1632-1639, then the deformed frame locked to it :1643-1653).  BASELINE configs[4] restated
// (SURVEY.md 8d): B (reference, deformed) pairs, two demodulations per sample, no fusion of any kind exists upstream.
int vistaf_ftp_predict_pairs(vistaf_ftp_handle *hd, const void *d_refs, const void *d_defs, int format, int B, float *d_height_mm,
                             uint8_t *d_reliable, double *d_scalars, int32_t *d_status, void *stream)
{
    if (!hd || !d_refs || !d_defs) return fail(VISTAF_E_INVALID, "null argument");
    if (B < 1 || B > hd->maxB) return fail(VISTAF_E_STATE, "batch exceeds max_batch");
    TRY(check_frames(hd, format, d_refs, d_defs));
    hipStream_t st = (hipStream_t)stream;
    const vistaf_ftp_config &c = hd->cfg;
    int h = hd->h, w = hd->w, P = hd->P, pad = std::max(0, c.fft_pad_px), pm = hd->pmax;
    bool timed = hd->timing;
    if (timed) ensure_events(hd);
    if (!hd->pairs_ready) {
        int rc;
        size_t mb = hd->maxB;
        if ((rc = dalloc(hd, &hd->pgeom, mb)) || (rc = dalloc(hd, &hd->pEx, mb * w * pm)) || (rc = dalloc(hd, &hd->pGx, mb * w * pm)) ||
            (rc = dalloc(hd, &hd->pEy, mb * h * pm)) || (rc = dalloc(hd, &hd->pGy, mb * h * pm)) || (rc = dalloc(hd, &hd->pcref, mb * P)) ||
            (rc = dalloc(hd, &hd->pamp_ref, mb * P)) || (rc = dalloc(hd, &hd->pwin, mb * pm * pm)) || (rc = dalloc(hd, &hd->hann_tab, (size_t)(pm + 1) * pm)))
            return rc;
        // every 1-D window a patch of up to pmax bins can need, as hann_patch() rounds it: the device forms each sample's window from these
        std::vector<float> tab((size_t)(pm + 1) * pm, 0.0f);
        for (int M = 1; M <= pm; M++) {
            const std::vector<float> row = hann_patch(1, M);
            std::copy(row.begin(), row.end(), tab.begin() + (size_t)M * pm);
        }
        HIPCHK(hipMemcpy(hd->hann_tab, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
        hd->pairs_ready = true;
    }
    HIPCHK(hipMemsetAsync(hd->status, 0, sizeof(int32_t) * B, st));
    const size_t sx = (size_t)w * pm, sy = (size_t)h * pm;
    const bool together = 2 * B <= hd->maxB;      // room for both frame sets in the workspace: preprocess them in the same launches
    const float *iw_def = hd->iw, *mu_def = hd->mu;
    const int *bad_def = hd->bad_count;
    if (together) {
        HIPCHK(hipMemsetAsync(hd->status + B, 0, sizeof(int32_t) * B, st));
        preprocess(hd, d_refs, format, B, st, timed, d_defs);
        iw_def = hd->iw + (size_t)B * P; mu_def = hd->mu + B; bad_def = hd->bad_count + B;
    } else preprocess(hd, d_refs, format, B, st, false);
    // ---- reference frames: carrier search, tables, demodulation
    int rc = reference_search(hd, B, hd->pgeom, st);
    if (rc) return rc;
    launch_pair_status(hd->pgeom, pm, hd->status, together ? hd->status + B : nullptr, B, st);
    // every sample's patch in a pmax x pmax slot: its own ph x pw bins (fewer where the spectrum border clips it), zeros beyond
    launch_build_tables(hd->pgeom, 1, hd->pEx, hd->pEy, hd->pGx, hd->pGy, sx, sy, B, h, w, pad, hd->Hf, hd->Wf, pm, st, hd->hann_tab, hd->pwin);
    launch_dft_forward(hd->iw, hd->mu, hd->pEx, hd->pEy, sx, sy, hd->pwin, hd->tmpT, hd->patch, pm * pm, B, h, w, pm, pm, st, pm * pm, hd->tiers.dft_staged != 0);
    launch_dft_inverse(hd->patch, pm * pm, hd->pGx, hd->pGy, sx, sy, hd->tmpT, hd->pcref, hd->pamp_ref, nullptr, nullptr, 0, nullptr, nullptr, B, h, w,
                       pm, pm, st, hd->pgeom, hd->tiers.dft_staged != 0);
    // ---- deformed frames, carrier locked to their own reference
    if (!together) preprocess(hd, d_defs, format, B, st, timed);
    if (timed) hipEventRecord(hd->ev[ST_DEMOD], st);
    launch_dft_forward(iw_def, mu_def, hd->pEx, hd->pEy, sx, sy, hd->pwin, hd->tmpT, hd->patch, pm * pm, B, h, w, pm, pm, st, pm * pm, hd->tiers.dft_staged != 0);
    launch_dft_inverse(hd->patch, pm * pm, hd->pGx, hd->pGy, sx, sy, hd->tmpT, hd->keep_planes ? hd->field : nullptr, hd->amp, hd->pcref, hd->pamp_ref,
                       (size_t)P, hd->prod, hd->wrapped, B, h, w, pm, pm, st, hd->pgeom, hd->tiers.dft_staged != 0);
    return post_demod(hd, B, d_height_mm, d_reliable, d_scalars, d_status, hd->pgeom, st, bad_def);
}

int vistaf_ftp_get_pair_info(vistaf_ftp_handle *hd, int batch, double *out /* [batch][VISTAF_NREFINFO] */, void *stream)
{
    if (!hd || !out) return fail(VISTAF_E_INVALID, "null argument");
    if (!hd->pairs_ready || batch < 1 || batch > hd->maxB) return fail(VISTAF_E_STATE, "predict_pairs has not been called");
    std::vector<CarrierGeom> g(batch);
    HIPCHK(hipMemcpyAsync(g.data(), hd->pgeom, sizeof(CarrierGeom) * batch, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    for (int b = 0; b < batch; b++) {
        double *o = out + (size_t)b * VISTAF_NREFINFO;
        o[0] = g[b].peak_x; o[1] = g[b].peak_y; o[2] = g[b].kx; o[3] = g[b].ky; o[4] = hd->Hf; o[5] = hd->Wf; o[6] = g[b].period;
        o[7] = g[b].period > 1e-12 ? hd->cfg.grating_pitch_mm / g[b].period : 0.0;
    }
    return 0;
}

int vistaf_ftp_contacts(vistaf_ftp_handle *hd, int B, int max_contacts, double *d_contacts, int32_t *d_count, int8_t *d_contact_index, void *stream)
{
    if (!hd || !d_contacts || !d_count) return fail(VISTAF_E_INVALID, "null argument");
    if (max_contacts < 1 || max_contacts > VISTAF_MAX_CONTACTS) return fail(VISTAF_E_INVALID, "max_contacts must be 1..64");
    if (hd->last_batch == 0) return fail(VISTAF_E_STATE, "no predict_batch / predict_pairs before contacts");
    if (B != hd->last_batch) return fail(VISTAF_E_STATE, "batch differs from the last predict's");
    const PostParams pp = post_params(hd, hd->last_pairs ? hd->pgeom : nullptr);      // as the tail took them
    launch_contacts(hd->depth, hd->kept, hd->labels, hd->peak_bits, hd->status, pp, hd->contacts_ws, max_contacts, d_contacts, VISTAF_NCONTACT, d_count,
                    d_contact_index, B, hd->h, hd->w, (hipStream_t)stream);
    return launch_ok("launch");
}

int vistaf_ftp_get_intermediate(vistaf_ftp_handle *hd, const char *name, void *d_dst, int batch, size_t *bytes_per_frame, void *stream)
{
    if (!hd || !name) return fail(VISTAF_E_INVALID, "null argument");
    auto it = hd->named.find(name);
    if (it == hd->named.end()) return fail(VISTAF_E_INVALID, std::string("unknown intermediate: ") + name);
    const vistaf_ftp_handle::Named &pl = it->second;
    if (bytes_per_frame) *bytes_per_frame = pl.bytes;
    if (d_dst) HIPCHK(hipMemcpyAsync(d_dst, pl.p, pl.per_frame ? pl.bytes * (size_t)batch : pl.bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

int vistaf_ftp_stage_count(void) { return ST_COUNT; }
const char *vistaf_ftp_stage_name(int i) { return (i >= 0 && i < ST_COUNT) ? kStageNames[i] : ""; }
int vistaf_ftp_enable_stage_timing(vistaf_ftp_handle *hd, int enable)
{
    if (!hd) return fail(VISTAF_E_INVALID, "null handle");
    hd->timing = enable != 0;
    return 0;
}
int vistaf_ftp_get_stage_times(vistaf_ftp_handle *hd, float *ms_out, int n)
{
    if (!hd || !ms_out) return fail(VISTAF_E_INVALID, "null argument");
    for (int i = 0; i < n && i < ST_COUNT; i++) ms_out[i] = hd->stage_ms[i];
    return 0;
}

// csrc/test_hooks.h (not part of the public header): kernel tier selection and debug planes for the parity tests
int vistaf_ftp_test_set(vistaf_ftp_handle *hd, const char *name, int value)
{
    if (!hd || !name) return fail(VISTAF_E_INVALID, "null argument");
    const std::string n(name);
    if (n == "inpaint_tier" && value >= 0 && value <= 2) hd->tiers.inpaint = value;
    else if (n == "big_flood_handback") hd->tiers.big_flood_handback = value != 0;
    else if (n == "chamfer_twopass") hd->tiers.chamfer_twopass = value != 0;
    else if (n == "telea_two_tier") hd->tiers.telea_two_tier = value != 0;
    else if (n == "telea_mw") hd->tiers.telea_mw = value != 0;
    else if (n == "big_queue_lds") hd->tiers.big_queue_lds = value != 0;
    else if (n == "big_gq_cap" && (value == 0 || (value >= 64 && (value & (value - 1)) == 0))) hd->tiers.big_gq_cap = value;
    else if (n == "big_fallback") hd->tiers.big_fallback = value != 0;
    else if (n == "unwrap_fast") hd->tiers.unwrap_fast = value != 0;
    else if (n == "big_chain") hd->tiers.big_chain = value != 0;
    else if (n == "select_resident") hd->tiers.select_resident = value != 0;
    else if (n == "dft_staged") hd->tiers.dft_staged = value != 0;
    else if (n == "fused_chains") hd->tiers.fused_chains = value != 0;
    else if (n == "gauss_strip") hd->tiers.gauss_strip = value != 0;
    else if (n == "fit_window") hd->tiers.fit_window = value != 0;
    else if (n == "fused_backend") hd->tiers.fused_backend = value != 0;
    else if (n == "fused_masks" && value >= 0 && value <= 7) hd->tiers.fused_masks = value;
    else if (n == "keep_planes") hd->keep_planes = value != 0;
    else return fail(VISTAF_E_INVALID, "unknown test hook or value: " + n);
    return 0;
}

// ---- the selection, IRLS fit and plain blur launchers on caller-supplied device planes (csrc/test_hooks.h).  Not on the predict path.
namespace {
// scratch of the k_big.hip chain for one call, by `variant`: 0 as vistaf_ftp_create allocates it (frames of 512 x 512 and more), 1 none, 2 required
int hook_scratch(int variant, int B, int h, int w, bool chain_ok, void **scratch)
{
    *scratch = nullptr;
    if (variant < 0 || variant > 2) return fail(VISTAF_E_INVALID, "variant must be 0, 1 or 2");
    if (variant == 2 && !chain_ok) return fail(VISTAF_E_INVALID, "variant 2: the k_big.hip chain does not take this batch");
    if (variant == 1 || (variant == 0 && !large_frame((size_t)h * w))) return 0;
    HIPCHK(hipMalloc(scratch, big_scratch_bytes(B, h, w)));
    return 0;
}
int hook_finish(void *a, void *b, hipStream_t st)
{
    const hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(st);
    if (a) (void)hipFree(a);
    if (b) (void)hipFree(b);
    if (e1 != hipSuccess) return fail(VISTAF_E_HIP, std::string("launch: ") + hipGetErrorString(e1));
    if (e2 != hipSuccess) return fail(VISTAF_E_HIP, std::string("sync: ") + hipGetErrorString(e2));
    return 0;
}
}  // namespace

int vistaf_ftp_test_select(const float *vals, const uint8_t *mask, size_t mask_stride, const float *le_thr, int use_abs, const float *reqs, int nreq,
                           float *out, int *counts, int B, int P, int variant, void *stream)
{
    if (!vals || !mask || !reqs || !out || B < 1 || P < 1 || nreq < 1 || (mask_stride != 0 && mask_stride != (size_t)P))
        return fail(VISTAF_E_INVALID, "bad argument");
    if (variant < 0 || variant > 3) return fail(VISTAF_E_INVALID, "variant must be 0, 1, 2 or 3");
    void *scratch = nullptr;
    int rc = hook_scratch(variant == 3 ? 1 : variant, B, 1, P, nreq <= 4 && big_frames(B, P), &scratch);
    if (rc) return rc;
    launch_select(vals, mask, mask_stride, le_thr, use_abs != 0, reqs, nreq, out, counts, B, P, (hipStream_t)stream, scratch, variant != 3);
    return hook_finish(scratch, nullptr, (hipStream_t)stream);
}

int vistaf_ftp_test_select_instance(int B, int P, int nreq, int variant)
{
    if (B < 1 || P < 1 || nreq < 1 || variant < 0 || variant > 3) return fail(VISTAF_E_INVALID, "bad argument");
    const bool chain_ok = nreq <= 4 && big_frames(B, P);
    if (variant == 2 && !chain_ok) return fail(VISTAF_E_INVALID, "variant 2: the k_big.hip chain does not take this batch");
    return select_variant(B, P, nreq, variant == 2 || (variant == 0 && large_frame((size_t)P)), variant != 3);
}

int vistaf_ftp_test_select_chained(const float *vals, const uint8_t *mask, size_t mask_stride, int use_abs, const float *reqs, int nreq, float *out,
                                   int *counts, int B, int P, void *stream)
{
    if (!vals || !mask || !reqs || !out || B < 1 || P < 1 || nreq < 1 || nreq > 4 || (mask_stride != 0 && mask_stride != (size_t)P))
        return fail(VISTAF_E_INVALID, "bad argument");
    float *outs[4] = {out, out + B, out + 2 * (size_t)B, out + 3 * (size_t)B};
    const int inst = launch_select_chained(vals, mask, mask_stride, use_abs != 0, reqs, nreq, outs, counts, B, P, (hipStream_t)stream);
    if (inst < 0) return fail(VISTAF_E_INVALID, "no resident instance takes this plane size");
    const int rc = hook_finish(nullptr, nullptr, (hipStream_t)stream);
    return rc ? rc : inst;
}

int vistaf_ftp_test_polyfit(const float *z, const uint8_t *mask, int order, int iters, float c, int min_count, int min_mask_count, float *coef,
                            float *resid, int B, int h, int w, int variant, void *stream)
{
    if (!z || !mask || !coef || !resid || B < 1 || h < 1 || w < 1 || (size_t)h * w > 0x7fffffffull || order < 1 || order > 2 || iters < 1)
        return fail(VISTAF_E_INVALID, "bad argument");
    void *scratch = nullptr;
    int rc = hook_scratch(variant, B, h, w, big_frames(B, h * w), &scratch);
    if (rc) return rc;
    const int inst = polyfit_variant(B, h, w, scratch != nullptr);
    launch_robust_polyfit(z, mask, order, iters, c, min_count, min_mask_count, coef, resid, B, h, w, (hipStream_t)stream, scratch);
    rc = hook_finish(scratch, nullptr, (hipStream_t)stream);
    return rc ? rc : inst;
}

// csrc/test_hooks_fit.h
static int fit_window_hook(const float *z, const uint8_t *mask, int order, int iters, float c, int min_count, int min_mask_count, float *coef, float *resid,
                           const FitSecond *second, int B, int h, int w, int variant, int32_t *need_out, void *stream)
{
    if (!z || !mask || !coef || !resid || (second && !second->resid_out) || B < 1 || h < 1 || w < 1 || (size_t)h * w > 0x7fffffffull || order < 1 || order > 2 ||
        (second && (second->order < 1 || second->order > 2)) || iters < 1)
        return fail(VISTAF_E_INVALID, "bad argument");
    if (variant < 0 || variant > 2) return fail(VISTAF_E_INVALID, "variant must be 0, 1 or 2");
    void *scratch = nullptr;
    int rc = hook_scratch(0, B, h, w, big_frames(B, h * w), &scratch);
    if (rc) return rc;
    const bool has_window = polyfit_window_variant(B, h, w, scratch != nullptr) >= 0;
    if (variant == 1 && !has_window) { if (scratch) (void)hipFree(scratch); return fail(VISTAF_E_INVALID, "variant 1: no window instance for this frame size"); }
    int32_t *need = nullptr;
    if (hipMalloc((void **)&need, (size_t)B * sizeof(int32_t)) != hipSuccess) { if (scratch) (void)hipFree(scratch); return fail(VISTAF_E_HIP, "hipMalloc"); }
    hipError_t e = hipMemsetAsync(need, 0xff, (size_t)B * sizeof(int32_t), (hipStream_t)stream);       // -1: no window kernel ran
    const int inst = launch_robust_polyfit_window(z, mask, order, iters, c, min_count, min_mask_count, coef, resid, second, need, Tiers().fit_window != 0, variant,
                                                  B, h, w, (hipStream_t)stream, scratch);
    if (e == hipSuccess && need_out) e = hipMemcpyAsync(need_out, need, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream);
    rc = hook_finish(scratch, need, (hipStream_t)stream);
    if (!rc && e != hipSuccess) rc = fail(VISTAF_E_HIP, std::string("need: ") + hipGetErrorString(e));
    return rc ? rc : inst;
}
int vistaf_ftp_test_polyfit_window(const float *z, const uint8_t *mask, int order, int iters, float c, int min_count, int min_mask_count, float *coef,
                                   float *resid, int B, int h, int w, int variant, int32_t *need_out, void *stream)
{
    return fit_window_hook(z, mask, order, iters, c, min_count, min_mask_count, coef, resid, nullptr, B, h, w, variant, need_out, stream);
}
int vistaf_ftp_test_polyfit_chain(const float *z, const uint8_t *mask, int order1, int order2, int iters, float c, int min_count, int min_mask_count1,
                                  int min_mask_count2, float *coef, float *resid1, float *resid2, int B, int h, int w, int variant, int32_t *need_out, void *stream)
{
    const FitSecond second = {order2, min_mask_count2, resid2};
    return fit_window_hook(z, mask, order1, iters, c, min_count, min_mask_count1, coef, resid1, &second, B, h, w, variant, need_out, stream);
}
int vistaf_ftp_test_polyfit_window_instance(int B, int h, int w)
{
    if (B < 1 || h < 1 || w < 1 || (size_t)h * w > 0x7fffffffull) return fail(VISTAF_E_INVALID, "bad argument");
    const bool big = large_frame((size_t)h * w);
    const int plain = polyfit_variant(B, h, w, big), win = polyfit_window_variant(B, h, w, big);
    return win >= 0 ? win : plain;
}

int vistaf_ftp_test_gauss_variant(const float *src, float *dst, double sigma, int B, int h, int w, int variant, void *stream)
{
    if (!src || !dst || src == dst || B < 1 || h < 1 || w < 1 || !(sigma > 0)) return fail(VISTAF_E_INVALID, "bad argument");
    if (variant < 0 || variant > 2) return fail(VISTAF_E_INVALID, "variant must be 0, 1 or 2");
    if (gauss_ksize(sigma) > 511) return fail(VISTAF_E_INVALID, "gaussian sigma too large (ksize > 511)");
    const std::vector<float> f = gauss_taps(sigma);
    if (variant == 2 && !gauss_strip_fits(h, w, (int)f.size())) return fail(VISTAF_E_INVALID, "variant 2: the strip kernel does not take this blur");
    float *taps = nullptr, *tmp = nullptr;
    HIPCHK(hipMalloc((void **)&taps, f.size() * sizeof(float)));
    if (hipMalloc((void **)&tmp, (size_t)B * h * w * sizeof(float)) != hipSuccess) { (void)hipFree(taps); return fail(VISTAF_E_HIP, "hipMalloc"); }
    if (hipMemcpy(taps, f.data(), f.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(taps); (void)hipFree(tmp);
        return fail(VISTAF_E_HIP, "memcpy taps");
    }
    const int tier = launch_gauss_blur(src, tmp, dst, taps, (int)f.size(), B, h, w, (hipStream_t)stream, Tiers().gauss_strip != 0, variant);
    const int rc = hook_finish(taps, tmp, (hipStream_t)stream);
    return rc ? rc : tier;
}
int vistaf_ftp_test_gauss_strip_fits(int h, int w, int ksize)
{
    if (h < 1 || w < 1 || ksize < 1 || !(ksize & 1)) return fail(VISTAF_E_INVALID, "bad argument");
    return gauss_strip_fits(h, w, ksize) ? 1 : 0;
}
int vistaf_ftp_test_gauss(const float *src, float *dst, double sigma, int B, int h, int w, void *stream)
{
    const int rc = vistaf_ftp_test_gauss_variant(src, dst, sigma, B, h, w, 0, stream);
    return rc < 0 ? rc : 0;
}

// The two chamfer hooks.  force: the one-wave two-pass kernel, which has no instance for every width; otherwise the dispatch, whose tier is
// the return value
static int chamfer_hook(const uint8_t *mask, int pair, int invert, float *dist_a, float *dist_b, int B, int h, int w, int cap_px, void *stream, bool force)
{
    if (!mask || !dist_a || (pair && !dist_b) || B < 1 || h < 1 || w < 1 || (size_t)h * w > 0x7fffffffull || cap_px < 0)
        return fail(VISTAF_E_INVALID, "bad argument");
    if (force && w > 512 && !(pair && w <= 1280)) return fail(VISTAF_E_INVALID, "no two-pass instance for this width");
    const int tier = force ? 0 : pair ? chamfer_pair_tier(B, h, w, cap_px) : chamfer_tier(h, w, cap_px);
    const size_t n = (size_t)B * h * w;
    int32_t *tmp_a = nullptr, *tmp_b = nullptr;
    HIPCHK(hipMalloc((void **)&tmp_a, n * sizeof(int32_t)));
    if (pair && hipMalloc((void **)&tmp_b, n * sizeof(int32_t)) != hipSuccess) { (void)hipFree(tmp_a); return fail(VISTAF_E_HIP, "hipMalloc"); }
    if (pair) launch_chamfer_pair(mask, tmp_a, dist_a, tmp_b, dist_b, B, h, w, cap_px, (hipStream_t)stream, force);
    else launch_chamfer(mask, invert != 0, tmp_a, dist_a, B, h, w, cap_px, (hipStream_t)stream, force);
    const int rc = hook_finish(tmp_a, tmp_b, (hipStream_t)stream);
    return rc ? rc : tier;
}
int vistaf_ftp_test_chamfer(const uint8_t *mask, int pair, int invert, float *dist_a, float *dist_b, int B, int h, int w, int cap_px, void *stream)
{
    return chamfer_hook(mask, pair, invert, dist_a, dist_b, B, h, w, cap_px, stream, true);
}

// ---- the mask topology launchers (labelling, largest component, chamfer dispatch, blob filter) on caller-supplied device planes
int vistaf_ftp_test_cc_label(const uint8_t *mask, int32_t *labels, int B, int h, int w, int variant, void *stream)
{
    if (!mask || !labels || B < 1 || h < 1 || w < 1 || (size_t)h * w > 0x7fffffffull) return fail(VISTAF_E_INVALID, "bad argument");
    if (variant < 0 || variant > 1) return fail(VISTAF_E_INVALID, "variant must be 0 or 1");
    const int tier = cc_label_tier(h, w, variant == 1);
    launch_cc_label(mask, labels, B, h, w, (hipStream_t)stream, variant == 1);
    const int rc = hook_finish(nullptr, nullptr, (hipStream_t)stream);
    return rc ? rc : tier;
}

int vistaf_ftp_test_cc_largest(const int32_t *labels, const uint8_t *and_static, uint8_t *out, int B, int P, int variant, void *stream)
{
    if (!labels || !out || B < 1 || P < 1) return fail(VISTAF_E_INVALID, "bad argument");
    if (variant < 0 || variant > 2) return fail(VISTAF_E_INVALID, "variant must be 0, 1 or 2");
    int32_t *area = nullptr;
    unsigned long long *best = nullptr;
    HIPCHK(hipMalloc((void **)&area, (size_t)B * P * sizeof(int32_t)));
    if (hipMalloc((void **)&best, (size_t)B * sizeof(unsigned long long)) != hipSuccess) { (void)hipFree(area); return fail(VISTAF_E_HIP, "hipMalloc"); }
    const int tier = cc_largest_tier(B, P, true, variant);
    launch_cc_largest(labels, area, best, and_static, out, B, P, (hipStream_t)stream, variant);
    const int rc = hook_finish(area, best, (hipStream_t)stream);
    return rc ? rc : tier;
}

int vistaf_ftp_test_chamfer_dispatch(const uint8_t *mask, int pair, int invert, float *dist_a, float *dist_b, int B, int h, int w, int cap_px, void *stream)
{
    return chamfer_hook(mask, pair, invert, dist_a, dist_b, B, h, w, cap_px, stream, false);
}

int vistaf_ftp_test_blob_filter(float *depth_inout, const uint8_t *cand, const int32_t *labels, const float *gmax, double min_peak_mm, double rel_frac,
                                uint8_t *kept, int B, int P, void *stream)
{
    if (!depth_inout || !cand || !labels || !gmax || !kept || B < 1 || P < 1) return fail(VISTAF_E_INVALID, "bad argument");
    unsigned int *peak_bits = nullptr;
    HIPCHK(hipMalloc((void **)&peak_bits, (size_t)B * P * sizeof(unsigned int)));
    launch_blob_filter(depth_inout, cand, labels, peak_bits, (const unsigned int *)gmax, min_peak_mm, rel_frac, kept, B, P, (hipStream_t)stream);
    return hook_finish(peak_bits, nullptr, (hipStream_t)stream);
}

// ---- launch_morph on caller-supplied device planes, each of its three kernels forced or dispatched
namespace {
// A test element no cv shape gives: row i spans |i - k / 2| either side of the anchor (widest at the first and last row, the anchor alone in
// the middle).  Its rows are not nested towards the centre, so a pixel outside the image that wrongly took part would show.
RowSpanSE hourglass_se(int k)
{
    RowSpanSE se;
    se.k = k;
    for (int i = 0; i < 33; i++) { se.lo[i] = 1; se.hi[i] = -1; }
    for (int i = 0; i < k; i++) { const int a = std::abs(i - k / 2); se.lo[i] = (int8_t)(-a); se.hi[i] = (int8_t)a; }
    return se;
}
}  // namespace
int vistaf_ftp_test_morph(const uint8_t *src, uint8_t *dst, int B, int h, int w, int shape, int kx, int ky, int dilate, const uint8_t *and_static,
                          const uint8_t *and_frame, int tier, void *stream)
{
    if (!src || !dst || src == dst || B < 1 || B > 65535 || h < 1 || h > 65535 || w < 1 || (size_t)B * h * w > 0x7fffffffull)
        return fail(VISTAF_E_INVALID, "bad argument");
    if (shape < 0 || shape > 2) return fail(VISTAF_E_INVALID, "shape must be 0 (ellipse), 1 (rectangle) or 2 (hourglass)");
    if (shape == 2 && (kx < 3 || kx > 33 || kx % 2 == 0)) return fail(VISTAF_E_INVALID, "hourglass size must be odd, 3..33");
    if (shape == 0 && (kx < 1 || kx > 33)) return fail(VISTAF_E_INVALID, "ellipse size must be 1..33");
    if (shape == 1 && (kx < 1 || kx > 127 || ky < 1 || ky > 33)) return fail(VISTAF_E_INVALID, "rectangle must be 1..127 wide and 1..33 tall");
    if (tier < 0 || tier > 4) return fail(VISTAF_E_INVALID, "tier must be 0..4");
    const RowSpanSE se = shape == 0 ? ellipse_se(kx) : shape == 1 ? rect_se(odd_up(kx), odd_up(ky)) : hourglass_se(kx);
    if (tier == MORPH_PREFIX && w >= 65536) return fail(VISTAF_E_INVALID, "tier 2: the uint16 row counts take rows shorter than 65536");
    if (tier == MORPH_BITS && !morph_bits_ok(se, h, w)) return fail(VISTAF_E_INVALID, "tier 3: the bit-plane kernel does not take this frame or element");
    const bool scratch = tier == 0 || tier == MORPH_PREFIX;
    const int ran = (tier == 0 || tier == 4) ? morph_tier(se, h, w, scratch) : tier;
    uint16_t *prefix = nullptr;
    if (scratch) HIPCHK(hipMalloc((void **)&prefix, (size_t)B * h * w * sizeof(uint16_t)));
    launch_morph(src, dst, B, h, w, se, dilate != 0, and_static, and_frame, (hipStream_t)stream, prefix, (tier == 0 || tier == 4) ? 0 : tier);
    const int rc = hook_finish(prefix, nullptr, (hipStream_t)stream);
    return rc ? rc : ran;
}

// ---- the three binary-mask chains (bad_mask_chain, reliable_mask_chain, contact_mask_chain above: the session's own functions) on
// caller-supplied device planes
namespace {
// one allocation carved into regions of the given sizes (256-byte aligned)
int hook_carve(const std::vector<size_t> &bytes, std::vector<void *> &out, void **base)
{
    size_t total = 0;
    for (size_t b : bytes) total += (b + 255) & ~(size_t)255;
    *base = nullptr;
    HIPCHK(hipMalloc(base, total ? total : 256));
    size_t off = 0;
    out.clear();
    for (size_t b : bytes) { out.push_back((char *)*base + off); off += (b + 255) & ~(size_t)255; }
    return 0;
}
bool chain_shape_ok(int B, int h, int w, int ksize, int iters, int fused)
{
    return B >= 1 && h >= 1 && w >= 1 && (size_t)h * w <= 0x7fffffffull / 4 && ksize >= 1 && ksize <= 33 && iters >= 0 && iters <= 16 && (fused == 0 || fused == 1);
}
}  // namespace

int vistaf_ftp_test_mask_chain_fits(int chain, int h, int w, int ksize, int nops, int margin_px)
{
    if (ksize < 1 || ksize > 33) return fail(VISTAF_E_INVALID, "bad argument");
    RowSpanSE se;
    TRY(make_se(ksize, &se, chain != MCH_CONTACT));
    return mask_chain_fits(chain, h, w, se, nops, (float)margin_px) ? 1 : 0;
}

int vistaf_ftp_test_bad_chain(const float *img, const float *grad, const uint8_t *valid, const float *thr_hi, const float *thr_g, int ksize, int iters,
                              uint8_t *bad1, int *bad_count, int B, int h, int w, int fused, void *stream)
{
    if (!img || !grad || !valid || !thr_hi || !thr_g || !bad1 || !bad_count || !chain_shape_ok(B, h, w, ksize, iters, fused))
        return fail(VISTAF_E_INVALID, "bad argument");
    RowSpanSE se;
    TRY(make_se(ksize, &se));
    void *base = nullptr;
    std::vector<void *> r;
    TRY(hook_carve({(size_t)B * h * w}, r, &base));
    const int tier = bad_mask_chain(img, grad, valid, thr_hi, thr_g, se, ksize, iters, (uint8_t *)r[0], bad1, bad_count, fused != 0, B, h, w, (hipStream_t)stream);
    const int rc = hook_finish(base, nullptr, (hipStream_t)stream);
    return tier < 0 ? tier : rc ? rc : tier;
}

int vistaf_ftp_test_reliable_chain(const float *quality, const uint8_t *roi, const float *amp_thr, int close_ksize, int close_iters, int margin_px,
                                   uint8_t *rel0, uint8_t *reliable, int *rel_count, int32_t *status, int B, int h, int w, int fused, void *stream)
{
    if (!quality || !roi || !amp_thr || !rel0 || !reliable || !rel_count || !status || !chain_shape_ok(B, h, w, close_ksize, close_iters, fused) ||
        margin_px < 0 || margin_px > 1024)
        return fail(VISTAF_E_INVALID, "bad argument");
    RowSpanSE se;
    TRY(make_se(close_ksize, &se));
    const size_t n = (size_t)B * h * w;
    void *base = nullptr;
    std::vector<void *> r;
    TRY(hook_carve({n, n, n * 4, n * 4, n * 4, n * 4, (size_t)B * 8, n * 2}, r, &base));
    const ReliableScratch ws = {(uint8_t *)r[0], (uint8_t *)r[1], (int32_t *)r[2], (int32_t *)r[3], (int32_t *)r[4], (float *)r[5], (unsigned long long *)r[6],
                                (uint16_t *)r[7]};
    const int tier = reliable_mask_chain(quality, roi, amp_thr, se, close_iters, margin_px, ws, false, rel0, reliable, rel_count, status, fused != 0, B, h, w,
                                         (hipStream_t)stream);
    const int rc = hook_finish(base, nullptr, (hipStream_t)stream);
    return tier < 0 ? tier : rc ? rc : tier;
}

int vistaf_ftp_test_contact_chain(const float *resid, const uint8_t *reliable, const float *thr3, const int *rel_count, double min_frac, double max_frac,
                                  int ksize, int iters, float *thr_used, uint8_t *contact_d, uint8_t *background, int *bg_count, int B, int h, int w,
                                  int fused, void *stream)
{
    if (!resid || !reliable || !thr3 || !rel_count || !thr_used || !contact_d || !background || !bg_count || !chain_shape_ok(B, h, w, ksize, iters, fused))
        return fail(VISTAF_E_INVALID, "bad argument");
    RowSpanSE se;
    TRY(make_se(ksize, &se, false));
    const size_t n = (size_t)B * h * w;
    void *base = nullptr;
    std::vector<void *> r;
    TRY(hook_carve({n, n, n * 2, (size_t)B * sizeof(int)}, r, &base));
    const ContactScratchPlanes ws = {(uint8_t *)r[0], (uint8_t *)r[1], (uint16_t *)r[2]};
    const int tier = contact_mask_chain(resid, reliable, thr3, rel_count, min_frac, max_frac, se, iters, ws, (int *)r[3], thr_used, contact_d, background,
                                        bg_count, fused != 0, B, h, w, (hipStream_t)stream);
    const int rc = hook_finish(base, nullptr, (hipStream_t)stream);
    return tier < 0 ? tier : rc ? rc : tier;
}

// ---- the unwrap launcher (consistency check, rank kernels, floods, replay / tree) on caller-supplied device planes
int vistaf_ftp_test_unwrap(const float *wrapped, const float *quality, const uint8_t *mask, float *unwrapped, int32_t *parent, int32_t *need,
                           int32_t *status, int B, int h, int w, int variant, void *stream)
{
    if (!wrapped || !quality || !mask || !unwrapped || !parent || !status || B < 1 || h < 8 || w < 8 || (size_t)h * w > 0x7fffffffull)
        return fail(VISTAF_E_INVALID, "bad argument");
    if (variant < 0 || variant > 2) return fail(VISTAF_E_INVALID, "variant must be 0, 1 or 2");
    if (variant == 0 && (!need || !unwrap_fast_supported(h, w)))
        return fail(VISTAF_E_INVALID, "variant 0: need is null, or the consistency check does not take this shape");
    const int tier = unwrap_tier(h, w, variant == 2);
    void *scratch = nullptr;
    HIPCHK(hipMalloc(&scratch, unwrap_scratch_bytes(B, h, w)));
    launch_unwrap(wrapped, quality, mask, unwrapped, parent, scratch, status, B, h, w, (hipStream_t)stream, nullptr, nullptr, variant == 2,
                  variant == 0 ? need : nullptr);
    const int rc = hook_finish(scratch, nullptr, (hipStream_t)stream);
    return rc ? rc : tier;
}

// ---- the Telea launchers (window tiers, cluster front end, big-cluster march, whole-frame kernel) on caller-supplied device planes
int vistaf_ftp_test_inpaint(float *img_inout, const uint8_t *bad, int range, int round_u8, int32_t *fb, int32_t *status, int B, int h, int w, int variant,
                            void *stream)
{
    if (!img_inout || !bad || !fb || !status || B < 1 || h < 8 || w < 8 || (size_t)h * w > 0x7fffffffull || range < 1 || range > 100)
        return fail(VISTAF_E_INVALID, "bad argument");
    if (variant < 0 || variant > 6) return fail(VISTAF_E_INVALID, "variant must be 0 .. 6");
    if (round_u8 && variant != 1) return fail(VISTAF_E_INVALID, "round_u8: the whole-frame kernel (variant 1) only");
    if (variant == 2 && !inpaint_window_mw_supported(range)) return fail(VISTAF_E_INVALID, "variant 2: the 16-wave window kernel does not take this range");
    if ((variant == 5 || variant == 6) && !inpaint_clusters_supported(range))
        return fail(VISTAF_E_INVALID, "variants 5 and 6: the cluster kernels do not take this range");
    hipStream_t st = (hipStream_t)stream;
    const bool dispatch = variant == 0 || variant >= 5;
    auto up = [](size_t n) { return (n + 255) & ~(size_t)255; };
    const size_t n_tel = variant <= 1 || variant >= 5 ? up(inpaint_scratch_bytes(B, h, w)) : 0, n_cl = dispatch ? up(inpaint_cl_scratch_bytes(B, h, w)) : 0,
                 n_win = variant != 1 ? up(inpaint_win_scratch_bytes(B)) : 0, n_only = up((size_t)B * sizeof(int32_t));
    uint8_t *base = nullptr;
    HIPCHK(hipMalloc((void **)&base, n_tel + n_cl + n_win + n_only));
    const InpaintBuffers buf = {base, base + n_tel, base + n_tel + n_cl, (int32_t *)(base + n_tel + n_cl + n_win)};
    const int32_t *only = nullptr;
    if (dispatch) {
        Tiers tiers;                                        // the defaults of a session
        if (variant >= 5) tiers.inpaint = 0;
        if (variant == 6) tiers.big_queue_lds = 0;
        only = inpaint_dispatch(img_inout, bad, range, tiers, true, buf, status, B, h, w, st, nullptr);
    } else if (variant == 1) launch_inpaint_telea(img_inout, bad, range, buf.scratch, status, nullptr, B, h, w, st, round_u8 != 0);
    else only = launch_inpaint_window(img_inout, bad, range, buf.win_scratch, B, h, w, st, nullptr, false, false, variant == 2 ? WNT_MW : variant == 3 ? WNT_FIRST : WNT_ALL);
    if (only) (void)hipMemcpyAsync(fb, only, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, st);
    return hook_finish(base, nullptr, st);
}

int vistaf_ftp_test_scratch_regions(const char *stage, int B, int h, int w, int range, int cap, char *names, size_t *offset, size_t *bytes, size_t *align,
                                    size_t *total)
{
    if (!stage || !names || !offset || !bytes || !align || !total || B < 1 || h < 1 || w < 1 || range < 1 || cap < 1) return fail(VISTAF_E_INVALID, "bad argument");
    const std::string s(stage);
    std::vector<ScratchRegion> regions;
    if (s == "unwrap") *total = unwrap_scratch_bytes(B, h, w, &regions);
    else if (s == "telea") *total = telea_scratch_bytes(B, h, w, &regions);
    else if (s == "inpaint_big") *total = inpaint_big_scratch_bytes(B, h, w, range, &regions);
    else if (s == "inpaint_cl") *total = inpaint_cl_scratch_bytes(B, h, w, &regions);
    else if (s == "inpaint_win") *total = inpaint_win_scratch_bytes(B, &regions);
    else if (s == "big") *total = big_scratch_bytes(B, h, w, &regions);
    else if (s == "tstats") *total = tstats_scratch_bytes(h, w, &regions);
    else if (s == "pressure") *total = pressure_scratch_bytes(B, h, w, range, &regions);      // range: pad_px
    if (regions.empty()) return fail(VISTAF_E_INVALID, "unknown stage: " + s);
    if ((int)regions.size() > cap) return fail(VISTAF_E_INVALID, "more regions than cap");
    for (size_t i = 0; i < regions.size(); i++) {
        snprintf(names + 32 * i, 32, "%s", regions[i].name ? regions[i].name : "");
        offset[i] = regions[i].offset; bytes[i] = regions[i].bytes; align[i] = regions[i].align;
    }
    return (int)regions.size();
}

int vistaf_ftp_test_dft_full_mag(const float *planes, const void *Ex_half, const void *Ey_full, void *tmp, double *mag, int B, int h, int w, int Hf,
                                 int Wf, void *stream)
{
    if (!planes || !Ex_half || !Ey_full || !tmp || !mag || B < 1 || h < 1 || w < 1 || Hf < h || Wf < w) return fail(VISTAF_E_INVALID, "bad argument");
    launch_dft_full_mag(planes, nullptr, (const double2 *)Ex_half, (const double2 *)Ey_full, (double2 *)tmp, mag, B, h, w, Hf, Wf, (hipStream_t)stream);
    return launch_ok("launch_dft_full_mag");
}

// ---- the demodulation launchers (k_dft.hip, k_dft_tables.hip) on caller-supplied device planes and tables
namespace {
// CarrierGeom <-> the two caller arrays of the hooks, in struct order: gd[7] = peak_x, peak_y, kx, ky, dpx, dpy, period;
// gi[10] = x0, y0, ph, pw, px_i, py_i, px_raw, py_raw, ok, keep_carrier
CarrierGeom geom_pack(const double *gd, const int32_t *gi)
{
    CarrierGeom g;
    g.peak_x = gd[0]; g.peak_y = gd[1]; g.kx = gd[2]; g.ky = gd[3]; g.dpx = gd[4]; g.dpy = gd[5]; g.period = gd[6];
    g.x0 = gi[0]; g.y0 = gi[1]; g.ph = gi[2]; g.pw = gi[3]; g.px_i = gi[4]; g.py_i = gi[5]; g.px_raw = gi[6]; g.py_raw = gi[7];
    g.ok = gi[8]; g.keep_carrier = gi[9];
    return g;
}
void geom_unpack(const CarrierGeom &g, double *gd, int32_t *gi)
{
    gd[0] = g.peak_x; gd[1] = g.peak_y; gd[2] = g.kx; gd[3] = g.ky; gd[4] = g.dpx; gd[5] = g.dpy; gd[6] = g.period;
    gi[0] = g.x0; gi[1] = g.y0; gi[2] = g.ph; gi[3] = g.pw; gi[4] = g.px_i; gi[5] = g.py_i; gi[6] = g.px_raw; gi[7] = g.py_raw;
    gi[8] = g.ok; gi[9] = g.keep_carrier;
}
// the sizes every launcher of the family indexes with 32-bit integers, and the grid limits of a batch
bool dft_sizes_ok(int B, int h, int w) { return B >= 1 && B <= 65535 && h >= 1 && w >= 1 && (size_t)B * h * w <= 0x7fffffffull; }
bool padded_ok(int h, int w, int pad, int Hf, int Wf) { return pad >= 0 && pad <= (1 << 20) && Hf == h + 2 * pad && Wf == w + 2 * pad && (size_t)Hf * Wf <= 0x7fffffffull; }
}  // namespace

int vistaf_ftp_test_top_peaks(const double *mag, int B, int Hf, int Wf, int dc, int npeaks, double *out, void *stream)
{
    if (!mag || !out || !dft_sizes_ok(B, Hf, Wf) || dc < 0 || npeaks < 1 || npeaks > 64 || (size_t)Hf * Wf < (size_t)npeaks)
        return fail(VISTAF_E_INVALID, "bad argument");
    launch_top_peaks(mag, B, Hf, Wf, dc, npeaks, out, (hipStream_t)stream);
    return hook_finish(nullptr, nullptr, (hipStream_t)stream);
}

int vistaf_ftp_test_carrier_choose(const double *peaks, int npk, const double *mag, int Hf, int Wf, int bw, double max_dy_frac, double *gd, int32_t *gi,
                                   int B, void *stream)
{
    if (!peaks || !mag || !gd || !gi || !dft_sizes_ok(B, Hf, Wf) || npk < 1 || npk > 64 || bw < 0 || bw > (1 << 20) || !(max_dy_frac >= 0.0) ||
        !(max_dy_frac <= 1e6))
        return fail(VISTAF_E_INVALID, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    // the kernel reads the magnitude plane at the listed positions: a list that points outside the plane is refused, not launched
    std::vector<double> pk((size_t)B * 192);
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipMemcpy(pk.data(), peaks, pk.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int b = 0; b < B; b++)
        for (int i = 0; i < npk; i++) {
            const double x = pk[(size_t)b * 192 + 3 * i], y = pk[(size_t)b * 192 + 3 * i + 1];
            if (!(x >= 0.0 && x < (double)Wf && y >= 0.0 && y < (double)Hf)) return fail(VISTAF_E_INVALID, "a listed peak lies outside the plane");
        }
    CarrierGeom *geom = nullptr;
    HIPCHK(hipMalloc((void **)&geom, (size_t)B * sizeof(CarrierGeom)));
    launch_carrier_choose(peaks, npk, mag, Hf, Wf, bw, max_dy_frac, geom, B, st);
    std::vector<CarrierGeom> g((size_t)B);
    const hipError_t e0 = hipGetLastError();
    const hipError_t e1 = e0 == hipSuccess ? hipMemcpyAsync(g.data(), geom, g.size() * sizeof(CarrierGeom), hipMemcpyDeviceToHost, st) : e0;
    const int rc = hook_finish(geom, nullptr, st);
    if (e1 != hipSuccess) return fail(VISTAF_E_HIP, std::string("launch_carrier_choose: ") + hipGetErrorString(e1));
    if (rc) return rc;
    for (int b = 0; b < B; b++) geom_unpack(g[b], gd + 7 * (size_t)b, gi + 10 * (size_t)b);
    return 0;
}

int vistaf_ftp_test_build_tables(const double *gd, const int32_t *gi, int geom_stride, int B, int h, int w, int pad, int Hf, int Wf, int pmax, int pair,
                                 void *Ex, void *Ey, void *Gx, void *Gy, float *win, void *stream)
{
    if (!gd || !gi || !Ex || !Ey || !Gx || !Gy || (pair && !win) || !dft_sizes_ok(B, h, w) || !padded_ok(h, w, pad, Hf, Wf) || pmax < 1 || pmax > 4096 ||
        (geom_stride != 0 && geom_stride != 1) || (size_t)std::max(std::max(h, w), pmax) * pmax > 0x7fffffffull)
        return fail(VISTAF_E_INVALID, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    const int ng = geom_stride ? B : 1;
    std::vector<CarrierGeom> g((size_t)ng);
    for (int b = 0; b < ng; b++) g[b] = geom_pack(gd + 7 * (size_t)b, gi + 10 * (size_t)b);
    std::vector<float> tab;
    if (pair) {                                             // as vistaf_ftp_predict_pairs builds hann_tab
        tab.assign((size_t)(pmax + 1) * pmax, 0.0f);
        for (int M = 1; M <= pmax; M++) {
            const std::vector<float> row = hann_patch(1, M);
            std::copy(row.begin(), row.end(), tab.begin() + (size_t)M * pmax);
        }
    }
    CarrierGeom *geom = nullptr;
    float *hann = nullptr;
    HIPCHK(hipMalloc((void **)&geom, g.size() * sizeof(CarrierGeom)));
    if (pair && hipMalloc((void **)&hann, tab.size() * sizeof(float)) != hipSuccess) { (void)hipFree(geom); return fail(VISTAF_E_HIP, "hipMalloc"); }
    if (hipMemcpy(geom, g.data(), g.size() * sizeof(CarrierGeom), hipMemcpyHostToDevice) != hipSuccess ||
        (pair && hipMemcpy(hann, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)) {
        (void)hipFree(geom); (void)hipFree(hann);
        return fail(VISTAF_E_HIP, "memcpy geometry");
    }
    launch_build_tables(geom, geom_stride, (double2 *)Ex, (double2 *)Ey, (double2 *)Gx, (double2 *)Gy, (size_t)w * pmax, (size_t)h * pmax, B, h, w, pad, Hf,
                        Wf, pmax, st, pair ? hann : nullptr, pair ? win : nullptr);
    return hook_finish(geom, hann, st);
}

int vistaf_ftp_test_build_full_tables(void *Exf, void *Eyf, int h, int w, int pad, int Hf, int Wf, void *stream)
{
    if (!Exf || !Eyf || !dft_sizes_ok(1, h, w) || !padded_ok(h, w, pad, Hf, Wf)) return fail(VISTAF_E_INVALID, "bad argument");
    launch_build_full_tables((double2 *)Exf, (double2 *)Eyf, h, w, pad, Hf, Wf, (hipStream_t)stream);
    return hook_finish(nullptr, nullptr, (hipStream_t)stream);
}

namespace {
// the `staged` flag of the demodulation launchers for a hook's `variant`: 0 as a session dispatches (staged where dft_staged_fits says so), 1 the
// kernels that read global memory, 2 the staged kernel of stage `bit`, an error where the shape does not take it
int dft_hook_variant(int variant, int bit, int h, int w, int ph, int pw, bool per_frame, bool *staged)
{
    if (variant < 0 || variant > 2) return fail(VISTAF_E_INVALID, "variant must be 0, 1 or 2");
    if (variant == 2 && !(dft_staged_fits(h, w, ph, pw, per_frame) & bit)) return fail(VISTAF_E_INVALID, "variant 2: the staged kernel does not take this shape");
    *staged = variant != 1;
    return 0;
}
}  // namespace

int vistaf_ftp_test_dft_forward(const float *iw, const float *mu, const void *Ex, const void *Ey, size_t tab_stride_x, size_t tab_stride_y, const float *win,
                                int win_stride, void *T, void *patch, int patch_stride, int B, int h, int w, int ph, int pw, void *stream)
{
    return vistaf_ftp_test_dft_forward_v(iw, mu, Ex, Ey, tab_stride_x, tab_stride_y, win, win_stride, T, patch, patch_stride, B, h, w, ph, pw, 0, stream);
}

int vistaf_ftp_test_dft_forward_v(const float *iw, const float *mu, const void *Ex, const void *Ey, size_t tab_stride_x, size_t tab_stride_y, const float *win,
                                  int win_stride, void *T, void *patch, int patch_stride, int B, int h, int w, int ph, int pw, int variant, void *stream)
{
    if (!iw || !Ex || !Ey || !win || !T || !patch || !dft_sizes_ok(B, h, w) || ph < 1 || pw < 1 || ph > 4096 || pw > 4096 ||
        (size_t)B * h * pw > 0x7fffffffull)
        return fail(VISTAF_E_INVALID, "bad argument");
    if ((tab_stride_x == 0) != (tab_stride_y == 0) || (tab_stride_x && (tab_stride_x < (size_t)w * pw || tab_stride_y < (size_t)ph * h)) ||
        (win_stride != 0 && win_stride < ph * pw) || patch_stride < ph * pw)
        return fail(VISTAF_E_INVALID, "a stride is smaller than what it strides over, or only one table stride is zero");
    bool staged;
    if (int rc = dft_hook_variant(variant, DFT_STAGED_FWD1, h, w, ph, pw, tab_stride_x != 0, &staged)) return rc;
    launch_dft_forward(iw, mu, (const double2 *)Ex, (const double2 *)Ey, tab_stride_x, tab_stride_y, win, (double2 *)T, (double2 *)patch, patch_stride, B, h, w,
                       ph, pw, (hipStream_t)stream, win_stride, staged);
    return hook_finish(nullptr, nullptr, (hipStream_t)stream);
}

int vistaf_ftp_test_dft_inverse(const void *patch, int patch_stride, const void *Gx, const void *Gy, size_t tab_stride_x, size_t tab_stride_y, void *Q, void *field,
                                float *amp, const void *cref, const float *amp_ref, size_t ref_stride, float *prod, float *wrapped, const int32_t *gi_or_null,
                                int B, int h, int w, int ph, int pw, void *stream)
{
    return vistaf_ftp_test_dft_inverse_v(patch, patch_stride, Gx, Gy, tab_stride_x, tab_stride_y, Q, field, amp, cref, amp_ref, ref_stride, prod, wrapped,
                                         gi_or_null, B, h, w, ph, pw, 0, stream);
}

int vistaf_ftp_test_dft_staged_fits(int h, int w, int ph, int pw, int per_frame_tables)
{
    if (h < 1 || w < 1 || ph < 1 || pw < 1) return fail(VISTAF_E_INVALID, "bad argument");
    return dft_staged_fits(h, w, ph, pw, per_frame_tables != 0);
}

int vistaf_ftp_test_dft_inverse_v(const void *patch, int patch_stride, const void *Gx, const void *Gy, size_t tab_stride_x, size_t tab_stride_y, void *Q,
                                  void *field, float *amp, const void *cref, const float *amp_ref, size_t ref_stride, float *prod, float *wrapped,
                                  const int32_t *gi_or_null, int B, int h, int w, int ph, int pw, int variant, void *stream)
{
    if (!patch || !Gx || !Gy || !Q || !amp || (cref && (!amp_ref || !prod || !wrapped)) || !dft_sizes_ok(B, h, w) || ph < 1 || pw < 1 || ph > 4096 ||
        pw > 4096 || (size_t)B * ph * w > 0x7fffffffull)
        return fail(VISTAF_E_INVALID, "bad argument");
    if ((tab_stride_x == 0) != (tab_stride_y == 0) || (tab_stride_x && (tab_stride_x < (size_t)w * pw || tab_stride_y < (size_t)ph * h)) ||
        patch_stride < ph * pw || (ref_stride != 0 && ref_stride < (size_t)h * w))
        return fail(VISTAF_E_INVALID, "a stride is smaller than what it strides over, or only one table stride is zero");
    bool staged;
    if (int rc = dft_hook_variant(variant, DFT_STAGED_INV2, h, w, ph, pw, tab_stride_x != 0, &staged)) return rc;
    hipStream_t st = (hipStream_t)stream;
    CarrierGeom *geom = nullptr;
    if (gi_or_null) {
        const double zeros[7] = {0, 0, 0, 0, 0, 0, 0};
        std::vector<CarrierGeom> g((size_t)B);
        for (int b = 0; b < B; b++) g[b] = geom_pack(zeros, gi_or_null + 10 * (size_t)b);
        HIPCHK(hipMalloc((void **)&geom, g.size() * sizeof(CarrierGeom)));
        if (hipMemcpy(geom, g.data(), g.size() * sizeof(CarrierGeom), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(geom);
            return fail(VISTAF_E_HIP, "memcpy geometry");
        }
    }
    launch_dft_inverse((const double2 *)patch, patch_stride, (const double2 *)Gx, (const double2 *)Gy, tab_stride_x, tab_stride_y, (double2 *)Q, (double2 *)field, amp,
                       (const double2 *)cref, amp_ref, ref_stride, prod, wrapped, B, h, w, ph, pw, st, geom, staged);
    return hook_finish(geom, nullptr, st);
}

// ---- csrc/test_hooks_post.h: the back end of post_demod (smoothing, sign flip, hole glue, composition and mm curve, blob filter, force tail,
// output copy) on caller-supplied device planes
}  // extern "C"
namespace {
// the scratch planes of one hook call: all allocated before the first launch, all freed after the stream has drained
struct HookBufs {
    std::vector<void *> p;
    template <typename T>
    bool get(T **out, size_t count)
    {
        void *q = nullptr;
        if (hipMalloc(&q, count * sizeof(T)) != hipSuccess) return false;
        p.push_back(q);
        *out = (T *)q;
        return true;
    }
    void release() { for (void *q : p) (void)hipFree(q); p.clear(); }
    int no_memory() { release(); return fail(VISTAF_E_HIP, "hipMalloc or the upload of the taps failed"); }
    int finish(hipStream_t st, int tier)
    {
        const int rc = hook_finish(nullptr, nullptr, st);
        release();
        return rc ? rc : tier;
    }
};
bool sigma_ok(double sigma) { return sigma >= 0 && sigma <= 1e6 && gauss_ksize(sigma > 0 ? sigma : 1.0) <= 511; }
// the session's taps for `sigma` on the device (none for sigma == 0)
bool upload_taps(HookBufs &bufs, const std::vector<float> &f, float **taps)
{
    *taps = nullptr;
    if (f.empty()) return true;
    return bufs.get(taps, f.size()) && hipMemcpy(*taps, f.data(), f.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
}
// B is a grid's y extent; the pixel count leaves room for the launchers' rounding up to whole workgroups in int
bool frame_ok(int B, int h, int w) { return B >= 1 && B <= 65535 && h >= 1 && w >= 1 && (size_t)h * w <= 0x40000000ull; }
bool curve_ok(int type, double a, double b, double c) { return type >= 0 && type <= 5 && a == a && b == b && c == c; }
PostParams hook_post_params(double mm_per_px, double depth_eps_mm, double period_px, const Curve &force)
{
    PostParams pp;
    pp.mm_per_px = mm_per_px; pp.depth_eps_mm = depth_eps_mm; pp.period_px = period_px; pp.force_curve = force;
    return pp;
}
// the chain scratch of launch_tail as a session of frames of P pixels holds it: none below large_frame
bool tail_hook_scratch(HookBufs &bufs, int B, int P, bool want, unsigned long long **scratch, size_t *bytes)
{
    *scratch = nullptr; *bytes = 0;
    if (!want) return true;
    *bytes = tail_scratch_bytes(B, P);
    return bufs.get(scratch, *bytes / sizeof(unsigned long long));
}
}  // namespace
extern "C" {

int vistaf_ftp_test_smooth_reliable(const float *detr, const float *bg_med, const uint8_t *reliable, double sigma, float *hmap, int B, int h, int w,
                                    int variant, void *stream)
{
    if (!detr || !bg_med || !reliable || !hmap || !frame_ok(B, h, w) || !sigma_ok(sigma)) return fail(VISTAF_E_INVALID, "bad argument");
    if (variant < 0 || variant > 2) return fail(VISTAF_E_INVALID, "variant must be 0, 1 or 2");
    const std::vector<float> f = sigma > 0 ? gauss_taps(sigma) : std::vector<float>();
    const int k = (int)f.size(), P = h * w;
    const bool tile_ok = k > 0 && k <= GF_MAXK;
    if (variant == 2 && !tile_ok) return fail(VISTAF_E_INVALID, "variant 2: the tile kernel takes 1..15 taps");
    hipStream_t st = (hipStream_t)stream;
    HookBufs bufs;
    if (k == 0) {
        launch_zeroed_keep_nan(detr, bg_med, reliable, hmap, B, P, st);
        return bufs.finish(st, 3);
    }
    float *taps = nullptr;
    if (!upload_taps(bufs, f, &taps)) return bufs.no_memory();
    if (variant == 2 || (variant == 0 && Tiers().fused_chains && tile_ok)) {
        launch_smooth_reliable(detr, bg_med, reliable, hmap, taps, k, B, h, w, st);
        return bufs.finish(st, 2);
    }
    const size_t n = (size_t)B * P;
    float *z0 = nullptr, *m = nullptr, *num = nullptr, *den = nullptr, *tmp = nullptr;
    if (!bufs.get(&z0, n) || !bufs.get(&m, n) || !bufs.get(&num, n) || !bufs.get(&den, n) || !bufs.get(&tmp, n)) return bufs.no_memory();
    launch_sub_scalar_mask(detr, bg_med, reliable, z0, m, B, P, st);
    launch_gauss_blur(z0, tmp, num, taps, k, B, h, w, st, Tiers().gauss_strip != 0);
    launch_gauss_blur(m, tmp, den, taps, k, B, h, w, st, Tiers().gauss_strip != 0);
    launch_div_planes(num, den, hmap, B, P, st);
    return bufs.finish(st, 1);
}

int vistaf_ftp_test_core_flip(float *hmap_inout, const float *core_med, int32_t *flipped, int B, int P, void *stream)
{
    if (!hmap_inout || !core_med || !flipped || !frame_ok(B, 1, P)) return fail(VISTAF_E_INVALID, "bad argument");
    launch_core_flip(hmap_inout, core_med, flipped, B, P, (hipStream_t)stream);
    return hook_finish(nullptr, nullptr, (hipStream_t)stream);
}

int vistaf_ftp_test_hole_candidates(const float *hmap, const uint8_t *reliable, const float *dist, int ksize, float frac_thr, float min_dist, uint8_t *cand,
                                    int B, int h, int w, void *stream)
{
    if (!hmap || !reliable || !dist || !cand || !frame_ok(B, h, w) || h > 65535 || ksize < 3 || ksize > 511 || !(ksize & 1))
        return fail(VISTAF_E_INVALID, "bad argument");
    launch_hole_candidates(hmap, reliable, dist, ksize, frac_thr, min_dist, cand, B, h, w, (hipStream_t)stream);
    return hook_finish(nullptr, nullptr, (hipStream_t)stream);
}

int vistaf_ftp_test_hole_tmp(const float *hmap, const uint8_t *reliable, const uint8_t *cand, const float *med, float *tmp, int B, int P, void *stream)
{
    if (!hmap || !reliable || !cand || !med || !tmp || !frame_ok(B, 1, P)) return fail(VISTAF_E_INVALID, "bad argument");
    launch_hole_tmp(hmap, reliable, cand, med, tmp, B, P, (hipStream_t)stream);
    return hook_finish(nullptr, nullptr, (hipStream_t)stream);
}
int vistaf_ftp_test_hole_zin(float *tmp_zin, const float *fill, int B, int P, void *stream)
{
    if (!tmp_zin || !fill || !frame_ok(B, 1, P)) return fail(VISTAF_E_INVALID, "bad argument");
    launch_hole_zin(tmp_zin, fill, B, P, (hipStream_t)stream);
    return hook_finish(nullptr, nullptr, (hipStream_t)stream);
}
int vistaf_ftp_test_hole_merge(float *hmap_inout, const uint8_t *reliable, const uint8_t *cand, const float *zin, uint8_t *out_rel, int B, int P,
                               void *stream)
{
    if (!hmap_inout || !reliable || !cand || !zin || !out_rel || !frame_ok(B, 1, P)) return fail(VISTAF_E_INVALID, "bad argument");
    launch_hole_merge(hmap_inout, reliable, cand, zin, out_rel, B, P, (hipStream_t)stream);
    return hook_finish(nullptr, nullptr, (hipStream_t)stream);
}

int vistaf_ftp_test_height_finish(const float *hmap, const uint8_t *reliable, const uint8_t *roi, const float *dist_in, const float *dist_out,
                                  const float *roi_den, float band, int use_band, double sigma_unrel, int curve_type, double curve_a, double curve_b,
                                  double curve_c, int use_neg, float *unitless, float *depth, uint8_t *cand, float *gmax, int B, int h, int w, int variant,
                                  void *stream)
{
    if (!hmap || !reliable || !roi || !dist_in || !dist_out || !roi_den || !unitless || !depth || !cand || !gmax || !frame_ok(B, h, w) ||
        !sigma_ok(sigma_unrel) || (use_band != 0 && use_band != 1) || (use_band && !(band > 0.f)) || !curve_ok(curve_type, curve_a, curve_b, curve_c))
        return fail(VISTAF_E_INVALID, "bad argument");
    if (variant < 0 || variant > 2) return fail(VISTAF_E_INVALID, "variant must be 0, 1 or 2");
    const std::vector<float> f = sigma_unrel > 0 ? gauss_taps(sigma_unrel) : std::vector<float>();
    const int k = (int)f.size(), P = h * w;
    const bool tile_ok = k > 0 && k <= GF_MAXK;
    if (variant == 2 && !tile_ok) return fail(VISTAF_E_INVALID, "variant 2: the tile kernel takes 1..15 taps");
    hipStream_t st = (hipStream_t)stream;
    const Curve curve{curve_type, curve_a, curve_b, curve_c};
    const float taper_band = use_band ? band : 1.0f;
    HookBufs bufs;
    float *taps = nullptr;
    if (!upload_taps(bufs, f, &taps)) return bufs.no_memory();
    if (variant == 2 || (variant == 0 && Tiers().fused_chains && tile_ok)) {
        launch_compose_finalize_mm(hmap, reliable, roi, dist_in, taper_band, roi_den, dist_out, band, use_band, curve, use_neg != 0, unitless, depth, cand,
                                   (unsigned int *)gmax, taps, k, B, h, w, st);
        return bufs.finish(st, 2);
    }
    const size_t n = (size_t)B * P;
    float *z0f = nullptr, *snum = nullptr, *tmp = nullptr;
    if (!bufs.get(&z0f, n) || (k && (!bufs.get(&snum, n) || !bufs.get(&tmp, n)))) return bufs.no_memory();
    launch_frontier_compose(hmap, reliable, roi, dist_in, taper_band, z0f, B, P, st);
    if (k) launch_gauss_blur(z0f, tmp, snum, taps, k, B, h, w, st, Tiers().gauss_strip != 0);
    launch_finalize_unitless(z0f, k ? snum : nullptr, roi_den, reliable, roi, dist_out, band, use_band, unitless, B, P, st);
    launch_to_mm(unitless, roi, curve, use_neg != 0, depth, cand, (unsigned int *)gmax, B, P, st);
    return bufs.finish(st, 1);
}

int vistaf_ftp_test_to_mm(const float *unitless, const uint8_t *roi, int curve_type, double curve_a, double curve_b, double curve_c, int use_neg, float *depth,
                          uint8_t *cand, float *gmax, int B, int P, void *stream)
{
    if (!unitless || !roi || !depth || !cand || !gmax || !frame_ok(B, 1, P) || !curve_ok(curve_type, curve_a, curve_b, curve_c))
        return fail(VISTAF_E_INVALID, "bad argument");
    launch_to_mm(unitless, roi, Curve{curve_type, curve_a, curve_b, curve_c}, use_neg != 0, depth, cand, (unsigned int *)gmax, B, P, (hipStream_t)stream);
    return hook_finish(nullptr, nullptr, (hipStream_t)stream);
}

int vistaf_ftp_test_tail(const float *height, const uint8_t *roi_frame, const float *unitless, const uint8_t *roi_static, double mm_per_px,
                         double depth_eps_mm, double period_px, int force_type, double force_a, double force_b, double force_c, double *scalars, int nscal,
                         double *out3, int B, int P, int variant, void *stream)
{
    if (!height || (!scalars && !out3) || (scalars && (!roi_static || nscal < 9)) || !frame_ok(B, 1, P) ||
        !curve_ok(force_type, force_a, force_b, force_c))
        return fail(VISTAF_E_INVALID, "bad argument");
    if (variant < 0 || variant > 2) return fail(VISTAF_E_INVALID, "variant must be 0, 1 or 2");
    hipStream_t st = (hipStream_t)stream;
    HookBufs bufs;
    unsigned long long *scratch = nullptr;
    size_t bytes = 0;
    if (!tail_hook_scratch(bufs, B, P, variant == 2 || (variant == 0 && large_frame((size_t)P)), &scratch, &bytes)) return bufs.no_memory();
    const int force = variant == 0 ? 0 : variant == 1 ? TAIL_FRAME : TAIL_BLOCKS;
    const int tier = tail_tier(B, P, scratch != nullptr, bytes, force);
    launch_tail(height, roi_frame, unitless, roi_static, hook_post_params(mm_per_px, depth_eps_mm, period_px, Curve{force_type, force_a, force_b, force_c}),
                scalars, nscal, out3, B, P, st, scratch, bytes, force);
    return bufs.finish(st, tier);
}

int vistaf_ftp_test_backend_fits(int h, int w)
{
    if (h < 1 || w < 1 || (size_t)h * w > 0x7fffffffull) return fail(VISTAF_E_INVALID, "bad argument");
    return backend_fused_fits(h, w) ? 1 : 0;
}

int vistaf_ftp_test_backend(float *depth_inout, const uint8_t *cand, const float *gmax, const float *unitless, const uint8_t *roi_static,
                            const uint8_t *reliable, const int32_t *status, double min_peak_mm, double rel_frac, double mm_per_px, double depth_eps_mm,
                            double period_px, int force_type, double force_a, double force_b, double force_c, int32_t *labels, uint32_t *peak_bits,
                            uint8_t *kept, double *scalars, int nscal, float *out_h, uint8_t *out_r, int B, int h, int w, int variant, void *stream)
{
    if (!depth_inout || !cand || !gmax || !roi_static || !reliable || !status || !labels || !peak_bits || !scalars || nscal < 9 || !frame_ok(B, h, w) ||
        !curve_ok(force_type, force_a, force_b, force_c))
        return fail(VISTAF_E_INVALID, "bad argument");
    if (variant < 0 || variant > 2) return fail(VISTAF_E_INVALID, "variant must be 0, 1 or 2");
    const bool fits = backend_fused_fits(h, w);
    if (variant == 2 && !fits) return fail(VISTAF_E_INVALID, "variant 2: the fused back end does not take this frame size");
    hipStream_t st = (hipStream_t)stream;
    const int P = h * w;
    const PostParams pp = hook_post_params(mm_per_px, depth_eps_mm, period_px, Curve{force_type, force_a, force_b, force_c});
    HookBufs bufs;
    if (variant == 2 || (variant == 0 && Tiers().fused_backend && fits)) {
        launch_backend_fused(depth_inout, cand, (const unsigned int *)gmax, unitless, roi_static, reliable, status, min_peak_mm, rel_frac, pp, labels, peak_bits,
                             kept, scalars, nscal, out_h, out_r, B, h, w, st);
        return bufs.finish(st, 2);
    }
    unsigned long long *scratch = nullptr;
    size_t bytes = 0;
    if (!tail_hook_scratch(bufs, B, P, large_frame((size_t)P), &scratch, &bytes)) return bufs.no_memory();
    launch_cc_label(cand, labels, B, h, w, st);
    launch_blob_filter(depth_inout, cand, labels, peak_bits, (const unsigned int *)gmax, min_peak_mm, rel_frac, kept, B, P, st);
    launch_tail(depth_inout, nullptr, unitless, roi_static, pp, scalars, nscal, nullptr, B, P, st, scratch, bytes);
    launch_copy_out(depth_inout, reliable, status, out_h, out_r, B, P, st);
    return bufs.finish(st, 1);
}

int vistaf_ftp_test_frame_records(const int *rel_count, const int *flipped, const float *amp_thr, const float *contact_thr, const float *bg_med,
                                  const int *bad_count, double *scalars, int nscal, int32_t *status, int B, void *stream)
{
    if (!rel_count || (!scalars && !status) || (scalars && nscal < 16) || B < 1) return fail(VISTAF_E_INVALID, "bad argument");
    if (scalars) launch_fill_scalars(scalars, nscal, rel_count, flipped, amp_thr, contact_thr, bg_med, bad_count, B, (hipStream_t)stream);
    if (status) launch_mark_empty(rel_count, status, B, (hipStream_t)stream);
    return hook_finish(nullptr, nullptr, (hipStream_t)stream);
}

int vistaf_depth_map_to_volume(const float *d_height, const uint8_t *d_roi, int batch, int h, int w, double mm_per_px,
                               double depth_eps_mm, double *d_out, void *stream)
{
    if (!d_height || !d_out || batch < 1 || h < 1 || w < 1) return fail(VISTAF_E_INVALID, "bad argument");
    PostParams pp;
    pp.mm_per_px = mm_per_px; pp.depth_eps_mm = depth_eps_mm; pp.period_px = 0; pp.force_curve = Curve{0, 0, 0, 0};
    launch_tail(d_height, d_roi, nullptr, nullptr, pp, nullptr, 0, d_out, batch, h * w, (hipStream_t)stream);
    return launch_ok("launch");
}

int vistaf_predict_force_from_volume(const vistaf_curve *curve, double volume_cm3, double *force_out)
{
    if (!curve || !force_out) return fail(VISTAF_E_INVALID, "null argument");
    if (curve->type < 0 || curve->type > 5) return fail(VISTAF_E_INVALID, "Unknown model type in force calibration JSON");
    Curve cv{curve->type, curve->a, curve->b, curve->c};
    *force_out = curve_eval(cv, volume_cm3);
    return 0;
}

}  // extern "C"
