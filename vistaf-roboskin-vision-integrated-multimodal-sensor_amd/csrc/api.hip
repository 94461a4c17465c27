// C ABI of the MI355X-native VISTAF FTP path (see include/vistaf_ftp.h).  Host orchestration only:
// every image operation runs in a HIP kernel of this library; the host builds constant tables
// (Gaussian taps, Hann window, DFT twiddles, ROI / apodisation planes) in double precision.  This file is the predict path: the handle,
// create, reference, predict and pairs.  The stages that choose between kernel tiers are functions of stages.hpp, which the test hooks
// (api_hooks.hip) call too; vistaf_ftp_test_set, the one hook that reads the handle, is here.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "stages.hpp"
#include "mask_bits.hpp"       // mask_chain_fits

using namespace vf;
#include "test_hooks.h"        // vistaf_ftp_test_set
#ifdef VISTAF_DEBUG
namespace vf { void telea_debug_dump(); void telea_window_debug_dump(int B); void telea_window_mw_debug_dump(int B); void fit_debug_dump(); void unwrap_big_debug_dump(); void unwrap_batch_debug_dump(); }
#endif

static thread_local std::string g_err;
static int fail(int code, const std::string &msg) { g_err = msg; return code; }
namespace vf { int set_error(int code, const std::string &msg) { return fail(code, msg); } }   // for the other translation units of the ABI

namespace {

struct GKern { float *d = nullptr; int k = 0; };

// The tables of a demodulation as launch_dft_forward and launch_dft_inverse take them: the session's (one carrier: the batch shares tables and
// window, the patch is the reference's ph x pw) or pair mode's (per-frame tables and windows in slots of pmax x pmax, per-frame geometry)
struct CarrierTables {
    const double2 *Ex = nullptr, *Ey = nullptr, *Gx = nullptr, *Gy = nullptr;      // forward (E) and inverse (G) tables
    size_t stride_x = 0, stride_y = 0;                                             // their per-frame strides, 0: shared
    const float *win = nullptr;
    int win_stride = 0, patch_stride = 0, ph = 0, pw = 0;
    const CarrierGeom *geom = nullptr;                                             // per-frame geometry, or null
};

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
    int Hf = 0, Wf = 0, pmax = 0;
    double2 *Ex = nullptr, *Ey = nullptr, *Gx = nullptr, *Gy = nullptr, *cref = nullptr;
    float *win = nullptr, *amp_ref = nullptr;
    CarrierGeom *geom = nullptr;                      // [1] session carrier, device
    CarrierTables tabs;                               // the above as the demodulation takes them, with the reference's patch size (set_reference)
    // carrier search (full spectrum), allocated on first use for `search_cap` frames
    double2 *Exf = nullptr, *Eyf = nullptr, *search_tmp = nullptr;
    double *search_mag = nullptr, *search_peaks = nullptr;
    int search_cap = 0;
    // uncached-pair mode (vistaf_ftp_predict_pairs): per-frame carriers, tables and reference fields, allocated on first use
    CarrierGeom *pgeom = nullptr;
    double2 *pEx = nullptr, *pEy = nullptr, *pGx = nullptr, *pGy = nullptr, *pcref = nullptr;
    float *pamp_ref = nullptr, *pwin = nullptr, *hann_tab = nullptr;     // pwin: [maxB][pmax^2] per-sample windows; hann_tab: hann(M)[i] at [M * pmax + i]
    CarrierTables ptabs;                              // the pair tables as the demodulation takes them
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
    if (!gauss_fits(sigma)) return gauss_refused();
    const std::vector<float> f = gauss_taps(sigma);
    TRY(hd->allocs.upload(&g->d, f));
    g->k = (int)f.size();
    return 0;
}

void blur(vistaf_ftp_handle *hd, const float *src, float *dst, const GKern &g, int B, hipStream_t st)
{
    launch_gauss_blur(src, hd->tmpf, dst, g.d, g.k, B, hd->h, hd->w, st, hd->tiers.gauss_strip != 0);
}

// the two halves of a demodulation with the tables `t`: forward of the frames iw / mu into hd->patch, inverse of hd->patch into the planes given
void dft_forward(vistaf_ftp_handle *hd, const CarrierTables &t, const float *iw, const float *mu, int B, hipStream_t st)
{
    launch_dft_forward(iw, mu, t.Ex, t.Ey, t.stride_x, t.stride_y, t.win, hd->tmpT, hd->patch, t.patch_stride, B, hd->h, hd->w, t.ph, t.pw, st, t.win_stride,
                       hd->tiers.dft_staged != 0);
}
void dft_inverse(vistaf_ftp_handle *hd, const CarrierTables &t, double2 *field, float *amp, const double2 *cref, const float *amp_ref, size_t ref_stride,
                 float *prod, float *wrapped, int B, hipStream_t st)
{
    launch_dft_inverse(hd->patch, t.patch_stride, t.Gx, t.Gy, t.stride_x, t.stride_y, hd->tmpT, field, amp, cref, amp_ref, ref_stride, prod, wrapped, B,
                       hd->h, hd->w, t.ph, t.pw, st, t.geom, hd->tiers.dft_staged != 0);
}

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

InpaintBuffers inpaint_buffers(const vistaf_ftp_handle *hd) { return {hd->inpaint_scratch, hd->inpaint_cl_scratch, hd->inpaint_win_scratch, hd->big_only}; }

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
        inpaint_dispatch(hd->img, hd->bad1, inpaint_range(c.bad_inpaint_radius), hd->tiers, true, inpaint_buffers(hd), hd->status, B, h, w, st,
                         timed ? hd->ev[ST_INPAINT] : nullptr);
    } else if (timed) hipEventRecord(hd->ev[ST_INPAINT], st);
    if (timed) hipEventRecord(hd->ev[ST_PREPROC], st);
    blur(hd, hd->img, hd->blurA, hd->g_illum, B, st);
    if (fuses(hd->tiers, hd->g_pre.k)) launch_illum_pre_apod(hd->img, hd->blurA, hd->apo, hd->iw, hd->g_pre.d, hd->g_pre.k, B, h, w, st);
    else {
        launch_illum_norm(hd->img, hd->blurA, hd->inorm, B, P, st);
        const float *in = hd->inorm;
        if (hd->g_pre.k) { blur(hd, hd->inorm, hd->blurA, hd->g_pre, B, st); in = hd->blurA; }
        launch_mul_static(in, hd->apo, hd->iw, B, P, st);
    }
    select(hd, hd->iw, hd->valid, 0, nullptr, false, hd->req_med, 1, hd->mu, nullptr, B, st);
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
    hd->tabs = {hd->Ex, hd->Ey, hd->Gx, hd->Gy, 0, 0, hd->win, 0, hd->pmax * hd->pmax, g.ph, g.pw, nullptr};
    const CarrierTables &t = hd->tabs;
    {
        std::vector<float> win = hann_patch(g.ph, g.pw);
        HIPCHK(hipMemcpyAsync(hd->win, win.data(), win.size() * sizeof(float), hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));         // `win` is a host temporary
    }
    launch_build_tables(hd->geom, 0, hd->Ex, hd->Ey, hd->Gx, hd->Gy, 0, 0, 1, h, w, pad, Hf, Wf, hd->pmax, st);
    dft_forward(hd, t, hd->iw, hd->mu, 1, st);
    dft_inverse(hd, t, hd->cref, hd->amp_ref, nullptr, nullptr, 0, nullptr, nullptr, 1, st);
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
    smooth_stage(hd->detr, hd->bg_med, hd->reliable, hd->g_rel.d, hd->g_rel.k, SmoothScratch{hd->z0, hd->mplane, hd->num, hd->den, hd->tmpf}, hd->hmap,
                 hd->tiers.fused_chains != 0, hd->tiers.gauss_strip != 0, B, h, w, st);      // without taps NaN stays NaN: the hole stage below is live
    core_medians(hd->hmap, hd->reliable, hd->req_core_med, hd->req_core, hd->req_med, hd->core_thr, hd->core_med, chain_scratch(hd),
                 hd->tiers.select_resident != 0, B, P, st);
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
        inpaint_dispatch(hd->z0, hd->hole_cand, inpaint_range(c.inpaint_radius), hd->tiers, false, inpaint_buffers(hd), hd->status, B, h, w, st, nullptr);
        launch_hole_merge(hd->hmap, hd->reliable, hd->hole_cand, hd->z0, hd->out_rel, B, P, st);
        orel = hd->out_rel;
    }

    // ---- frontier taper, composition, unreliable-region smoothing, clamp (shape_ftp.py:1770-1841)
    if (timed) hipEventRecord(hd->ev[ST_COMPOSE], st);
    bool use_band = c.frontier_zero_band_px > 0;
    float band = (float)c.frontier_zero_band_px;
    // both distance transforms of the reliable mask (to its outside for the taper, to its inside for the final blend) in one launch; the
    // second one lands in a plane that is idle at this point (`area` is the integer temporary): `depth`, which to_mm writes below, or, when
    // the one-kernel compose runs, `snum`, which only the kernel sequence writes -- that kernel reads the distance and writes `depth` in one
    // pass, and with the two apart none of its pointers alias
    float *dist2 = fuses(hd->tiers, hd->g_unrel.k) ? hd->snum : hd->depth;      // (the predicate of height_finish_stage)
    if (use_band) launch_chamfer_pair(orel, hd->rowdist, hd->dist, hd->area, dist2, B, h, w, c.frontier_zero_band_px + 2, st, hd->tiers.chamfer_twopass != 0);
    else HIPCHK(hipMemsetAsync(hd->dist, 0x7f, (size_t)B * P * sizeof(float), st));   // huge distance: taper weight 1
    // ---- unitless -> mm (shape_ftp.py:1850-1873): the mm_blob stage starts at the mm curve
    height_finish_stage(hd->hmap, orel, hd->roi, hd->dist, use_band ? band : 1.0f, hd->roi_den, use_band ? dist2 : hd->dist, band, use_band ? 1 : 0,
                        hd->hcurve, hd->use_neg, hd->g_unrel.d, hd->g_unrel.k, HeightScratch{hd->z0f, hd->snum, hd->tmpf}, hd->unitless, hd->depth,
                        hd->cand, hd->gmax, hd->tiers.fused_chains != 0, hd->tiers.gauss_strip != 0, timed ? hd->ev[ST_MM_BLOB] : nullptr, B, h, w, st);

    // ---- blob filter, force tail (multimodal_sensor.py:388-419) + arg-extrema, the frame records, the caller's planes: the tail stage starts
    // at the tail (with the one-launch back end, which counts as mm_blob, it is left with k_fill_scalars and the two small copies)
    const FrameRecords rec = {hd->rel_count, hd->flipped, hd->amp_thr, hd->thr_used, hd->bg_med, bad_count};
    backend_stage(hd->depth, hd->cand, hd->gmax, hd->unitless, hd->roi, orel, hd->status, c.contact_blob_min_peak_mm, c.contact_blob_min_peak_rel_frac,
                  post_params(hd, pair_geom), hd->labels, hd->peak_bits, hd->kept, hd->scalars, VISTAF_NSCALARS, d_height_mm, d_reliable,
                  chain_scratch(hd), hd->big_scratch_bytes, hd->tiers.fused_backend != 0, &rec, timed ? hd->ev[ST_TAIL] : nullptr, B, h, w, st);
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
    bool timed = hd->timing;
    if (timed) ensure_events(hd);
    HIPCHK(hipMemsetAsync(hd->status, 0, sizeof(int32_t) * B, st));

    preprocess(hd, d_frames, format, B, st, timed);

    // ---- demodulation, carrier locked to the reference (shape_ftp.py:1643-1653, :1681-1689)
    if (timed) hipEventRecord(hd->ev[ST_DEMOD], st);
    dft_forward(hd, hd->tabs, hd->iw, hd->mu, B, st);
    dft_inverse(hd, hd->tabs, hd->keep_planes ? hd->field : nullptr, hd->amp, hd->cref, hd->amp_ref, 0, hd->prod, hd->wrapped, B, st);
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
        const std::vector<float> tab = hann_table(pm);
        HIPCHK(hipMemcpy(hd->hann_tab, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
        // every sample's patch in a pmax x pmax slot: its own ph x pw bins (fewer where the spectrum border clips it), zeros beyond
        hd->ptabs = {hd->pEx, hd->pEy, hd->pGx, hd->pGy, (size_t)w * pm, (size_t)h * pm, hd->pwin, pm * pm, pm * pm, pm, pm, hd->pgeom};
        hd->pairs_ready = true;
    }
    HIPCHK(hipMemsetAsync(hd->status, 0, sizeof(int32_t) * B, st));
    const CarrierTables &t = hd->ptabs;
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
    launch_build_tables(hd->pgeom, 1, hd->pEx, hd->pEy, hd->pGx, hd->pGy, t.stride_x, t.stride_y, B, h, w, pad, hd->Hf, hd->Wf, pm, st, hd->hann_tab, hd->pwin);
    dft_forward(hd, t, hd->iw, hd->mu, B, st);
    dft_inverse(hd, t, hd->pcref, hd->pamp_ref, nullptr, nullptr, 0, nullptr, nullptr, B, st);
    // ---- deformed frames, carrier locked to their own reference
    if (!together) preprocess(hd, d_defs, format, B, st, timed);
    if (timed) hipEventRecord(hd->ev[ST_DEMOD], st);
    dft_forward(hd, t, iw_def, mu_def, B, st);
    dft_inverse(hd, t, hd->keep_planes ? hd->field : nullptr, hd->amp, hd->pcref, hd->pamp_ref, (size_t)P, hd->prod, hd->wrapped, B, st);
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
