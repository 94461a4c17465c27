// Stand-alone host check of the surface texture read-out's C ABI (include_ext/vistaf_texture.h): the argument checking of both functions and
// the workspace layout, for a run under the host sanitizers.  It includes the translation unit itself, so texture_scratch is the one the library
// carves with; every call here is refused before a launch, nothing needs a device.  Build and run (no GPU needed):
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -o texture_host_check tests/diag/texture_host_check.hip
//   ASAN_OPTIONS=detect_leaks=0 ./texture_host_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "../../vistaf-roboskin-vision-integrated-multimodal-sensor_amd/csrc/k_texture.hip"

static std::string g_last;
namespace vf {
int set_error(int code, const std::string &msg) { g_last = msg; return code; }
}  // namespace vf

#define EXPECT(c)                                                                 \
    do {                                                                          \
        if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } \
    } while (0)

static bool says(const char *word) { return g_last.find(word) != std::string::npos; }

int main()
{
    size_t bytes = 1;
    EXPECT(vistaf_texture_workspace_bytes(8, 8, 1, 8, 8, nullptr) == VISTAF_E_INVALID && says("bytes"));
    const struct { int h, w, b, k, l; const char *word; } bad[] = {
        {0, 8, 1, 8, 8, "h "}, {8, 0, 1, 8, 8, "w "}, {65536, 65536, 1, 8, 8, "h * w"}, {8, 8, 0, 8, 8, "max_batch"}, {8, 8, -1, 8, 8, "max_batch"},
        {8, 8, (1 << 19) + 1, 8, 8, "max_batch"}, {8, 8, 1, 0, 8, "max_contacts"}, {8, 8, 1, 65, 8, "max_contacts"}, {8, 8, 1, 8, 1, "max_lag"},
        {8, 8, 1, 8, 32, "max_lag"}, {8, 8, 1, 8, -4, "max_lag"}};
    for (const auto &a : bad) {
        bytes = 1;
        EXPECT(vistaf_texture_workspace_bytes(a.h, a.w, a.b, a.k, a.l, &bytes) == VISTAF_E_INVALID && bytes == 0 && says(a.word));
    }

    // the layout: sized with a null base, carved from a buffer of exactly that size; both regions are written to their last element, and a
    // smaller batch ends inside the buffer of a larger one
    const struct { int B, K, L; } shapes[] = {{1, 1, 2}, {3, 8, 8}, {2, 4, 31}, {5, 64, 16}, {256, 8, 8}};
    for (const auto &sh : shapes) {
        ScratchRec rec;
        EXPECT(vistaf_texture_workspace_bytes(37, 53, sh.B, sh.K, sh.L, &bytes) == 0);
        EXPECT(bytes == texture_scratch_bytes(sh.B, sh.K, sh.L, &rec) && rec.size() == 2);
        uint8_t *base = (uint8_t *)std::aligned_alloc(256, (bytes + 255) & ~(size_t)255);
        EXPECT(base);
        ScratchLayout carve(base);
        const TextureBufs bf = texture_scratch(carve, sh.B, sh.K, sh.L);
        EXPECT(carve.bytes() == bytes && rec.back().offset + rec.back().bytes == bytes);
        EXPECT(rec[0].offset == 0 && rec[1].offset % 256 == 0 && rec[0].bytes <= rec[1].offset);
        const size_t n = (size_t)sh.B * sh.K * (sh.L + 1) * (2 * sh.L + 1);
        EXPECT((uint8_t *)bf.C == base && rec[0].bytes == n * 8 && (uint8_t *)bf.N == base + rec[1].offset && rec[1].bytes == n * 4);
        std::memset(bf.C, 0x5a, n * 8);
        std::memset(bf.N, 0x5a, n * 4);
        // the last entry the kernels write: row B*K - 1, dy = L, lane 2L
        const size_t last = (((size_t)sh.B * sh.K - 1) * (sh.L + 1) + sh.L) * (2 * sh.L + 1) + 2 * sh.L;
        EXPECT(last == n - 1);
        bf.C[last] = 1.0;
        bf.N[last] = 1;
        for (int b = 1; b < sh.B; b += 7) EXPECT(texture_scratch_bytes(b, sh.K, sh.L, nullptr) <= bytes);
        std::free(base);
    }

    // measure: every refusal comes before any HIP call and names its argument
    alignas(256) static uint8_t ws[4096];
    alignas(8) static double tab[8 * 16], mpp[1], out[8 * 40], acf[8 * 17 * 17];
    alignas(4) static float depth[64], res[64];
    alignas(4) static int32_t cnt[1];
    static int8_t idx[64];
    EXPECT(vistaf_texture_workspace_bytes(8, 8, 1, 8, 8, &bytes) == 0 && bytes > sizeof ws);
    struct Args {
        const float *depth; const int8_t *idx; const double *tab; const int32_t *cnt; const double *mpp; float eps; double frac; int deg, L; double thr, pm;
        int h, w, B, K; double *out; float *res; double *acf; void *ws; size_t n;
    };
    const Args good{depth, idx, tab, cnt, mpp, 0.01f, 0.5, 2, 8, 0.2, 0.3, 8, 8, 1, 8, out, res, acf, ws, bytes};
    auto call = [](const Args &a) {
        return vistaf_texture_measure(a.depth, a.idx, a.tab, a.cnt, a.mpp, a.eps, a.frac, a.deg, a.L, a.thr, a.pm, a.h, a.w, a.B, a.K, a.out, a.res, a.acf,
                                      a.ws, a.n, nullptr);
    };
    const double nan = std::numeric_limits<double>::quiet_NaN();
    Args a = good;
    a.depth = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_depth_mm")); a = good;
    a.idx = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_contact_index")); a = good;
    a.tab = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_contacts")); a = good;
    a.cnt = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_count")); a = good;
    a.mpp = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_mm_per_px")); a = good;
    a.out = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_textures")); a = good;
    a.res = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_residual_mm")); a = good;
    a.acf = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_acf")); a = good;
    a.ws = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_workspace")); a = good;
    a.h = 0; EXPECT(call(a) == VISTAF_E_INVALID && says("h ")); a = good;
    a.w = -2; EXPECT(call(a) == VISTAF_E_INVALID && says("w ")); a = good;
    a.h = a.w = 65536; EXPECT(call(a) == VISTAF_E_INVALID && says("h * w")); a = good;
    a.B = 0; EXPECT(call(a) == VISTAF_E_INVALID && says("batch")); a = good;
    a.K = 65; EXPECT(call(a) == VISTAF_E_INVALID && says("max_contacts")); a = good;
    a.L = 1; EXPECT(call(a) == VISTAF_E_INVALID && says("max_lag")); a = good;
    a.L = 32; EXPECT(call(a) == VISTAF_E_INVALID && says("max_lag")); a = good;
    a.eps = std::numeric_limits<float>::infinity(); EXPECT(call(a) == VISTAF_E_INVALID && says("depth_eps_mm")); a = good;
    a.frac = 1.0; EXPECT(call(a) == VISTAF_E_INVALID && says("eval_min_fraction")); a = good;
    a.frac = nan; EXPECT(call(a) == VISTAF_E_INVALID && says("eval_min_fraction")); a = good;
    a.deg = 3; EXPECT(call(a) == VISTAF_E_INVALID && says("form_degree")); a = good;
    a.deg = -1; EXPECT(call(a) == VISTAF_E_INVALID && says("form_degree")); a = good;
    a.thr = 0.0; EXPECT(call(a) == VISTAF_E_INVALID && says("acf_threshold")); a = good;
    a.thr = nan; EXPECT(call(a) == VISTAF_E_INVALID && says("acf_threshold")); a = good;
    a.pm = 1.0; EXPECT(call(a) == VISTAF_E_INVALID && says("peak_min")); a = good;
    a.tab = (const double *)((const char *)tab + 4); EXPECT(call(a) == VISTAF_E_INVALID && says("aligned") && says("d_contacts")); a = good;
    a.res = (float *)((char *)res + 2); EXPECT(call(a) == VISTAF_E_INVALID && says("aligned") && says("d_residual_mm")); a = good;
    a.ws = ws + 64; EXPECT(call(a) == VISTAF_E_INVALID && says("d_workspace") && says("aligned")); a = good;
    a.n = bytes - 1; EXPECT(call(a) == VISTAF_E_INVALID && says("workspace_bytes")); a = good;
    a.n = 0; EXPECT(call(a) == VISTAF_E_INVALID && says("workspace_bytes")); a = good;
    a.B = 2; EXPECT(call(a) == VISTAF_E_INVALID && says("workspace_bytes"));      // sized for one frame
    std::printf("texture host check ok\n");
    return 0;
}
