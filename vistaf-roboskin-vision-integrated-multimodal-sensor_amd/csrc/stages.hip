// The tier dispatch of the stages of a predict (stages.hpp): host orchestration only, every image operation is a launcher of kernels.hpp.
#include "stages.hpp"
#include "mask_rules.hpp"      // chamfer_ball
#include "mask_bits.hpp"       // mask_chain_fits

namespace vf {

int make_se(int k, RowSpanSE *se, bool force_odd)
{
    if (force_odd) k = std::max(3, k | 1);
    if (k > 33) return set_error(VISTAF_E_INVALID, "structuring element larger than 33");
    *se = ellipse_se(k);
    return 0;
}

// np.hanning(M) = 0.5 + 0.5*cos(pi*n/(M-1)), n = 1-M, 3-M, ...
std::vector<float> hann_patch(int ph, int pw)
{
    auto hann = [](int M, int i) -> float { return M == 1 ? 1.0f : (float)(0.5 + 0.5 * std::cos(3.14159265358979323846 * (double)(1 - M + 2 * i) / (double)(M - 1))); };
    std::vector<float> win((size_t)ph * pw);
    for (int a = 0; a < ph; a++)
        for (int c = 0; c < pw; c++) win[(size_t)a * pw + c] = hann(ph, a) * hann(pw, c);
    return win;
}

std::vector<float> hann_table(int pmax)
{
    std::vector<float> tab((size_t)(pmax + 1) * pmax, 0.0f);
    for (int M = 1; M <= pmax; M++) {
        const std::vector<float> row = hann_patch(1, M);
        std::copy(row.begin(), row.end(), tab.begin() + (size_t)M * pmax);
    }
    return tab;
}

int gauss_refused() { return set_error(VISTAF_E_INVALID, "gaussian sigma too large (ksize > 511)"); }
static_assert(GAUSS_MAX_TAPS == 511, "the text of gauss_refused names the limit");

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

int smooth_stage(const float *detr, const float *bg_med, const uint8_t *reliable, const float *taps, int k, const SmoothScratch &ws, float *hmap,
                 bool fused_chains, bool gauss_strip, int B, int h, int w, hipStream_t st)
{
    const int P = h * w;
    if (fuses(fused_chains, k)) {
        launch_smooth_reliable(detr, bg_med, reliable, hmap, taps, k, B, h, w, st);
        return 2;
    }
    if (k > 0) {
        launch_sub_scalar_mask(detr, bg_med, reliable, ws.z0, ws.mplane, B, P, st);
        launch_gauss_blur(ws.z0, ws.tmp, ws.num, taps, k, B, h, w, st, gauss_strip);
        launch_gauss_blur(ws.mplane, ws.tmp, ws.den, taps, k, B, h, w, st, gauss_strip);
        launch_div_planes(ws.num, ws.den, hmap, B, P, st);
        return 1;
    }
    launch_zeroed_keep_nan(detr, bg_med, reliable, hmap, B, P, st);      // NaN stays NaN: the hole stage of a session is live
    return 3;
}

int core_medians(const float *hmap, const uint8_t *reliable, const float *req_chain, const float *req_core, const float *req_med, float *core_thr,
                 float *core_med, void *chain, bool select_resident, int B, int P, hipStream_t st)
{
    float *const outs[2] = {core_thr, core_med};
    if (select_variant(B, P, 2, chain != nullptr, select_resident) >= SELV_RES16 &&
        launch_select_chained(hmap, reliable, (size_t)P, false, req_chain, 2, outs, nullptr, B, P, st) >= 0)
        return 2;
    launch_select(hmap, reliable, (size_t)P, nullptr, false, req_core, 1, core_thr, nullptr, B, P, st, chain, select_resident);
    launch_select(hmap, reliable, (size_t)P, core_thr, false, req_med, 1, core_med, nullptr, B, P, st, chain, select_resident);
    return 1;
}

int height_finish_stage(const float *hmap, const uint8_t *reliable, const uint8_t *roi, const float *dist_in, float taper_band, const float *roi_den,
                        const float *dist_out, float band, int use_band, const Curve &curve, int use_neg, const float *taps, int k,
                        const HeightScratch &ws, float *unitless, float *depth, uint8_t *cand, unsigned int *gmax_bits, bool fused_chains,
                        bool gauss_strip, hipEvent_t ev_mm, int B, int h, int w, hipStream_t st)
{
    const int P = h * w;
    if (fuses(fused_chains, k)) {      // the mm curve runs in the same kernel and counts as composition
        launch_compose_finalize_mm(hmap, reliable, roi, dist_in, taper_band, roi_den, dist_out, band, use_band, curve, use_neg, unitless, depth, cand,
                                   gmax_bits, taps, k, B, h, w, st);
        if (ev_mm) hipEventRecord(ev_mm, st);
        return 2;
    }
    launch_frontier_compose(hmap, reliable, roi, dist_in, taper_band, ws.z0f, B, P, st);
    if (k) launch_gauss_blur(ws.z0f, ws.tmp, ws.snum, taps, k, B, h, w, st, gauss_strip);
    launch_finalize_unitless(ws.z0f, k ? ws.snum : nullptr, roi_den, reliable, roi, dist_out, band, use_band, unitless, B, P, st);
    if (ev_mm) hipEventRecord(ev_mm, st);
    launch_to_mm(unitless, roi, curve, use_neg, depth, cand, gmax_bits, B, P, st);
    return 1;
}

int backend_stage(float *depth, const uint8_t *cand, const unsigned int *gmax_bits, const float *unitless, const uint8_t *roi_static,
                  const uint8_t *reliable, const int32_t *status, double min_peak_mm, double rel_frac, const PostParams &pp, int32_t *labels,
                  unsigned int *peak_bits, uint8_t *kept, double *scalars, int nscal, float *out_h, uint8_t *out_r, void *chain, size_t chain_bytes,
                  bool fused_backend, const FrameRecords *rec, hipEvent_t ev_tail, int B, int h, int w, hipStream_t st)
{
    const int P = h * w;
    const bool fused = fused_backend && backend_fused_fits(h, w);
    if (fused)
        launch_backend_fused(depth, cand, gmax_bits, unitless, roi_static, reliable, status, min_peak_mm, rel_frac, pp, labels, peak_bits, kept, scalars,
                             nscal, out_h, out_r, B, h, w, st);
    else {
        launch_cc_label(cand, labels, B, h, w, st);
        launch_blob_filter(depth, cand, labels, peak_bits, gmax_bits, min_peak_mm, rel_frac, kept, B, P, st);
    }
    if (ev_tail) hipEventRecord(ev_tail, st);
    if (!fused) launch_tail(depth, nullptr, unitless, roi_static, pp, scalars, nscal, nullptr, B, P, st, chain, chain_bytes);
    if (rec) launch_fill_scalars(scalars, nscal, rec->rel_count, rec->flipped, rec->amp_thr, rec->contact_thr, rec->bg_med, rec->bad_count, B, st);
    if (!fused) launch_copy_out(depth, reliable, status, out_h, out_r, B, P, st);
    return fused ? 2 : 1;
}

}  // namespace vf
