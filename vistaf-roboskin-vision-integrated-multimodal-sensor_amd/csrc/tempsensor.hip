// The temperature modality end to end (include/vistaf_tempsensor.h): Code/temperature_sensor.py:749-870 `main()` as one session.
//
// The host side only: every step is one of the library's existing stages (tempseg.hip, k_lab.hip, k_tempmodel.hip, k_tempmap.hip) launched on
// the session's own device buffers, so no intermediate plane leaves the device; the statistics are k_tempstats.hip.  The session owns one
// segmentation session (vistaf_tempseg_handle) whose workspaces are built here, and the smoothing taps, so that predict allocates nothing.
#include <hip/hip_runtime.h>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/vistaf_tempsensor.h"
#include "host_util.hpp"

using namespace vf;

struct vistaf_tstats {
    int H = 0, W = 0;
    uint8_t *scratch = nullptr, *big = nullptr;
    double *out = nullptr;                  // the results when the caller passes no device buffer
    DeviceAllocs allocs;
};

struct vistaf_tsensor {
    vistaf_tsensor_config cfg;
    int H = 0, W = 0;
    size_t P = 0;
    const vistaf_tmodel *models[2] = {nullptr, nullptr};
    vistaf_tempseg_handle *seg = nullptr;
    vistaf_tstats *stats = nullptr;
    DeviceAllocs allocs;
    float *planes = nullptr;                // L, a, b, gray
    float *raw = nullptr;                   // wide_raw, color_raw
    float *tmp = nullptr, *wide = nullptr, *color = nullptr, *fused = nullptr;
    uint8_t *masks = nullptr, *source = nullptr;
    float *kx = nullptr, *ky = nullptr;
    int nx = 0, ny = 0;
};

extern "C" {

int vistaf_tsensor_default_config(vistaf_tsensor_config *c)
{
    if (!c) return set_error(VISTAF_E_INVALID, "null config");
    memset(c, 0, sizeof(*c));
    vistaf_tempseg_default_config(&c->seg);
    c->fuse.color_t_min = 20.0; c->fuse.color_t_max = 33.0; c->fuse.color_guard_band = 0.5; c->fuse.switch_margin_c = 1.0;
    c->fuse.final_t_min = 20.0; c->fuse.final_t_max = 75.0;
    c->blur_ksize = 5; c->color_support_dilate = 3; c->wide_inpaint_radius = 7; c->color_inpaint_radius = 5;
    c->color_chroma_min = 10.0; c->color_clamp_pad = 5.0; c->smooth_sigma_across = 6.0; c->smooth_sigma_along = 1.0;
    return 0;
}

void vistaf_tsensor_stats_destroy(vistaf_tstats *s)
{
    if (!s) return;
    s->allocs.free_all();
    delete s;
}

int vistaf_tsensor_stats_create(int H, int W, vistaf_tstats **out)
{
    if (!out) return set_error(VISTAF_E_INVALID, "null argument");
    if (H < 1 || W < 1) return set_error(VISTAF_E_INVALID, "map sides must be >= 1");
    if ((long long)H * W > 0x7fffffffll) return set_error(VISTAF_E_INVALID, "map larger than 2^31 pixels");
    Created<vistaf_tstats> s(new vistaf_tstats(), vistaf_tsensor_stats_destroy);
    s->H = H; s->W = W;
    TRY(s->allocs.alloc(&s->scratch, tstats_scratch_bytes(H, W)));
    if (tstats_needs_big_scratch(H, W)) TRY(s->allocs.alloc(&s->big, big_scratch_bytes(1, H, W)));
    TRY(s->allocs.alloc(&s->out, VISTAF_TSENSOR_NSTATS));
    *out = s.release();
    return 0;
}

int vistaf_tsensor_map_statistics(vistaf_tstats *s, const float *d_map, const uint8_t *d_valid, double *d_stats, double *stats_host, void *stream)
{
    if (!s || !d_map) return set_error(VISTAF_E_INVALID, "null argument");
    if (!d_stats && !stats_host) return set_error(VISTAF_E_INVALID, "map_statistics: no output (d_stats and stats_host are both NULL)");
    hipStream_t st = (hipStream_t)stream;
    double *out = d_stats ? d_stats : s->out;
    launch_tstats(d_map, d_valid, s->H, s->W, s->scratch, s->big, out, st);
    int rc = launch_ok("map_statistics");
    if (rc) return rc;
    if (stats_host) {
        if (hipMemcpyAsync(stats_host, out, VISTAF_TSENSOR_NSTATS * sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return set_error(VISTAF_E_HIP, "map_statistics: host copy");
    }
    return 0;
}

void vistaf_tsensor_destroy(vistaf_tsensor *h)
{
    if (!h) return;
    h->allocs.free_all();
    vistaf_tempseg_destroy(h->seg);
    vistaf_tsensor_stats_destroy(h->stats);
    delete h;
}

int vistaf_tsensor_create(const vistaf_tsensor_config *cfg, int H, int W, const vistaf_tmodel *wide_model, const vistaf_tmodel *color_model,
                          vistaf_tsensor **out)
{
    if (!cfg || !out) return set_error(VISTAF_E_INVALID, "null argument");
    if (!wide_model || !color_model) return set_error(VISTAF_E_INVALID, "tsensor_create: both the wide and the colour model are required");
    if (H < 64 || W < 64 || H % 16)
        return set_error(VISTAF_E_INVALID, "tsensor_create: the segmentation needs a frame height that is a multiple of 16 and both sides >= 64, got " +
                                               std::to_string(H) + " x " + std::to_string(W));
    if (cfg->wide_inpaint_radius < 1 || cfg->wide_inpaint_radius > 100 || cfg->color_inpaint_radius < 1 || cfg->color_inpaint_radius > 100)
        return set_error(VISTAF_E_INVALID, "tsensor_create: inpaint radius out of range");
    const int kb = cfg->blur_ksize > 1 ? odd_up(cfg->blur_ksize) : 1;
    if (kb != 1 && kb != 5) return set_error(VISTAF_E_INVALID, "tsensor_create: blur_ksize must be 5 (BLUR_KSIZE as shipped) or <= 1 (no smoothing)");
    if (odd_up(cfg->color_support_dilate) > 33) return set_error(VISTAF_E_INVALID, "tsensor_create: colour support dilation taller than 33");
    Created<vistaf_tsensor> h(new vistaf_tsensor(), vistaf_tsensor_destroy);
    h->cfg = *cfg; h->H = H; h->W = W; h->P = (size_t)H * W;
    h->models[0] = wide_model; h->models[1] = color_model;
    const size_t P = h->P;
    TRY(vistaf_tempseg_create(&cfg->seg, H, W, &h->seg));
    TRY(tempseg_prepare(h->seg));
    TRY(vistaf_tsensor_stats_create(H, W, &h->stats));
    TRY(h->allocs.alloc(&h->planes, 4 * P)); TRY(h->allocs.alloc(&h->raw, 2 * P)); TRY(h->allocs.alloc(&h->tmp, P));
    TRY(h->allocs.alloc(&h->wide, P)); TRY(h->allocs.alloc(&h->color, P)); TRY(h->allocs.alloc(&h->fused, P));
    TRY(h->allocs.alloc(&h->masks, VISTAF_TSENSOR_NMASKS * P)); TRY(h->allocs.alloc(&h->source, P));
    TRY(h->allocs.alloc(&h->kx, 1024)); TRY(h->allocs.alloc(&h->ky, 1024));
    TRY(temp_blur_taps(cfg->smooth_sigma_across, cfg->smooth_sigma_along, h->kx, h->nx, h->ky, h->ny, nullptr));
    *out = h.release();
    return 0;
}

int vistaf_tsensor_predict(vistaf_tsensor *h, const uint8_t *d_bgr, const uint8_t *d_roi, float *d_final, uint8_t *d_source, float *d_wide,
                           float *d_color, uint8_t *d_masks, double *info_host, double *d_stats, double *stats_host, void *stream)
{
    if (!h || !d_bgr || !d_roi || !d_final) return set_error(VISTAF_E_INVALID, "null argument");
    hipStream_t st = (hipStream_t)stream;
    const vistaf_tsensor_config &c = h->cfg;
    const size_t P = h->P;
    uint8_t *M = d_masks ? d_masks : h->masks;
    uint8_t *roi_eff = M + VISTAF_TSENSOR_MASK_ROI_EFF * P, *sat = M + VISTAF_TSENSOR_MASK_SAT * P, *dark = M + VISTAF_TSENSOR_MASK_DARK * P,
            *light = M + VISTAF_TSENSOR_MASK_LIGHT * P, *support = M + VISTAF_TSENSOR_MASK_COLOR_SUPPORT * P;
    float *L = h->planes, *A = h->planes + P, *B = h->planes + 2 * P, *G = h->planes + 3 * P;
    float *wide_raw = h->raw, *color_raw = h->raw + P;
    float *wide = d_wide ? d_wide : h->wide, *color = d_color ? d_color : h->color;
    uint8_t *source = d_source ? d_source : h->source;
    double seg_info[VISTAF_TEMPSEG_NINFO];
    // 1-3: segmentation, feature planes, colour support (:770-799 on the full frame)
    TRY(vistaf_tempseg_segment(h->seg, d_bgr, d_roi, dark, light, roi_eff, sat, seg_info, stream));
    TRY(vistaf_temp_feature_planes(h->seg, d_bgr, c.blur_ksize, L, A, B, G, stream));
    TRY(vistaf_temp_color_support(h->seg, A, B, light, roi_eff, sat, c.color_chroma_min, c.color_support_dilate, nullptr, support, stream));
    // 4: both regressors in one pass: the wide model over roi_eff (inferred, see the header), the colour model over the colour support
    const uint8_t *mk[2] = {roi_eff, support};
    float *outs[2] = {wide_raw, color_raw};
    const float *pl[4] = {L, A, B, G};
    TRY(vistaf_tmodel_predict_maps(2, h->models, mk, outs, pl, h->H, h->W, stream));
    // 5-6: inpaint and clamp each map (:835-845)
    TRY(vistaf_temp_inpaint_map(h->seg, wide_raw, d_roi, c.wide_inpaint_radius, h->tmp, stream));
    TRY(vistaf_temp_clamp_map(h->seg, h->tmp, d_roi, c.fuse.final_t_min, c.fuse.final_t_max, wide, stream));
    TRY(vistaf_temp_inpaint_map(h->seg, color_raw, support, c.color_inpaint_radius, h->tmp, stream));
    TRY(vistaf_temp_clamp_map(h->seg, h->tmp, support, c.fuse.color_t_min - c.color_clamp_pad, c.fuse.color_t_max + c.color_clamp_pad, color, stream));
    // 7-8: per-pixel fusion, smoothing along the stripes (:850-865)
    int64_t counts[4] = {0, 0, 0, 0};
    TRY(vistaf_temp_fuse_maps(h->seg, d_roi, wide, color, &c.fuse, h->fused, source, info_host ? counts : nullptr, stream));
    TRY(temp_blur_apply(h->seg, h->fused, d_roi, seg_info[VISTAF_TS_CARRIER_ANGLE_RAD], h->kx, h->nx, h->ky, h->ny, d_final, st));
    // 9: statistics of the final map over its finite pixels
    if (d_stats || stats_host) TRY(vistaf_tsensor_map_statistics(h->stats, d_final, nullptr, d_stats, stats_host, stream));
    if (info_host) {
        for (int i = 0; i < VISTAF_TEMPSEG_NINFO; i++) info_host[i] = seg_info[i];
        for (int i = 0; i < 4; i++) info_host[VISTAF_TEMPSEG_NINFO + i] = (double)counts[i];
    }
    return launch_ok("tsensor_predict");
}

}  // extern "C"
