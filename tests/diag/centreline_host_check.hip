// Stand-alone host check of the centreline read-out's C ABI (include_ext/vistaf_centreline.h): the argument checking of both functions, the tier
// rule and the workspace layout, for a run under the host sanitizers.  It includes the translation unit itself, so centreline_scratch is the one
// the library carves with; every call here is refused before a launch, nothing needs a device.  Build and run (no GPU needed):
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -o centreline_host_check tests/diag/centreline_host_check.hip
//   ASAN_OPTIONS=detect_leaks=0 ./centreline_host_check
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../vistaf-roboskin-vision-integrated-multimodal-sensor_amd/csrc/k_centreline.hip"

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
    EXPECT(vistaf_centreline_workspace_bytes(8, 8, 1, 8, nullptr) == VISTAF_E_INVALID && says("bytes"));
    const struct { int h, w, b, k; const char *word; } bad[] = {
        {0, 8, 1, 8, "h "}, {32768, 8, 1, 8, "h "}, {8, 0, 1, 8, "w "}, {8, 32768, 1, 8, "w "}, {32767, 32767, 1, 8, "h * w"}, {8, 8, 0, 8, "batch"},
        {8, 8, -1, 8, "batch"}, {8, 8, (1 << 24) + 1, 8, "batch"}, {8, 8, 1, 0, "max_contacts"}, {8, 8, 1, 65, "max_contacts"}};
    for (const auto &a : bad) {
        bytes = 1;
        EXPECT(vistaf_centreline_workspace_bytes(a.h, a.w, a.b, a.k, &bytes) == VISTAF_E_INVALID && bytes == 0 && says(a.word));
    }

    // the tier rule: monotone in both sizes, a whole 224 x 224 frame in LDS, the launch's LDS never above the budget
    EXPECT(vistaf_ftp_test_centreline_tier(0, 8) == VISTAF_E_INVALID && says("bw") && vistaf_ftp_test_centreline_tier(8, 32768) == VISTAF_E_INVALID && says("bh"));
    EXPECT(vistaf_ftp_test_centreline_tier(224, 224) == 1 && vistaf_ftp_test_centreline_tier(1, 1) == 1 && vistaf_ftp_test_centreline_tier(32767, 32767) == 0);
    for (int n = 1; n < 700; n++) {
        EXPECT(!cl_box_in_lds(n, n) || (cl_box_in_lds(n - 1 > 0 ? n - 1 : 1, n) && cl_box_in_lds(n, n - 1 > 0 ? n - 1 : 1)));
        EXPECT(cl_launch_lds(n, n) <= (size_t)CL_LDS_BUDGET && (!cl_box_in_lds(n, n) || cl_launch_lds(n, n) == cl_planes_bytes(n, n)));
        EXPECT(cl_planes_bytes(n, n) == (size_t)(n + 2) * ((n + 63) / 64) * 8 * CL_PLANES);
    }

    // the layout: sized with a null base, carved from a buffer of exactly that size; every region is written to its last element; the row
    // planes are there exactly when a box of the whole frame leaves LDS, and the last row's seven planes end with the region
    const struct { int B, h, w, K; } shapes[] = {{1, 1, 1, 1}, {3, 24, 32, 8}, {2, 37, 53, 8}, {5, 7, 201, 64}, {2, 224, 224, 8}, {2, 263, 263, 3}, {1, 9, 4000, 2}};
    for (const auto &sh : shapes) {
        ScratchRec rec;
        EXPECT(vistaf_centreline_workspace_bytes(sh.h, sh.w, sh.B, sh.K, &bytes) == 0);
        EXPECT(bytes == centreline_scratch_bytes(sh.B, sh.h, sh.w, sh.K, &rec) && rec.size() == 3);
        uint8_t *base = (uint8_t *)std::aligned_alloc(256, (bytes + 255) & ~(size_t)255);
        EXPECT(base);
        ScratchLayout carve(base);
        const CentrelineBufs bf = centreline_scratch(carve, sh.B, sh.h, sh.w, sh.K);
        EXPECT(carve.bytes() == bytes && rec.back().offset + rec.back().bytes == bytes);
        for (size_t i = 0; i + 1 < rec.size(); i++) EXPECT(rec[i].offset % 256 == 0 && rec[i].offset + rec[i].bytes <= rec[i + 1].offset);
        const size_t P = (size_t)sh.h * sh.w, rows = (size_t)sh.B * sh.K;
        EXPECT((bf.row_words == 0) == cl_box_in_lds(sh.w, sh.h) && (bf.row_words == 0 || bf.row_words == cl_plane_words(sh.w, sh.h) * CL_PLANES));
        const struct { void *p; size_t n; } regions[] = {{bf.stn, sh.B * P * 4}, {bf.d2, sh.B * P * 4}, {bf.planes, rows * bf.row_words * 8}};
        for (size_t i = 0; i < 3; i++) {
            EXPECT((uint8_t *)regions[i].p == base + rec[i].offset && regions[i].n == rec[i].bytes);
            std::memset(regions[i].p, 0x5a, regions[i].n);
        }
        if (bf.row_words) {
            u64 *last = bf.planes + (rows - 1) * bf.row_words;                      // as k_centreline_rows cuts it
            EXPECT((uint8_t *)(last + CL_PLANES * cl_plane_words(sh.w, sh.h)) == base + bytes);
        }
        std::free(base);
    }

    // measure: every refusal comes before any HIP call and names its argument
    alignas(256) static uint8_t ws[4096];
    alignas(8) static double tab[8 * 16], mpp[1], out[8 * 40];
    alignas(4) static int32_t cnt[1], st[64], sd[32], offs[9];
    alignas(4) static float dep[64];
    static int8_t idx[64], sk[64];
    EXPECT(vistaf_centreline_workspace_bytes(8, 8, 1, 8, &bytes) == 0 && bytes > 0 && bytes <= sizeof ws);
    struct Args { const int8_t *idx; const double *tab; const int32_t *cnt; const double *mpp; const float *dep; int B, h, w, K, span, V; double *out; int32_t *st, *sd, *offs; int8_t *sk; void *ws; size_t n; };
    const Args good{idx, tab, cnt, mpp, dep, 1, 8, 8, 8, 8, 32, out, st, sd, offs, sk, ws, bytes};
    auto call = [](const Args &a) {
        return vistaf_centreline_measure(a.idx, a.tab, a.cnt, a.mpp, a.dep, a.B, a.h, a.w, a.K, a.span, a.V, a.out, a.st, a.sd, a.offs, a.sk, a.ws, a.n, nullptr);
    };
    Args a = good;
    a.idx = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_contact_index")); a = good;
    a.tab = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_contacts")); a = good;
    a.cnt = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_count")); a = good;
    a.mpp = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_mm_per_px")); a = good;
    a.out = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_centrelines")); a = good;
    a.ws = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_workspace")); a = good;
    a.st = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_stations") && says("d_offsets")); a = good;
    a.st = nullptr; a.offs = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_stations") && says("d_station_d2")); a = good;
    a.offs = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_offsets") && says("d_stations")); a = good;
    a.h = 0; EXPECT(call(a) == VISTAF_E_INVALID && says("h ")); a = good;
    a.w = 40000; EXPECT(call(a) == VISTAF_E_INVALID && says("w ")); a = good;
    a.B = 0; EXPECT(call(a) == VISTAF_E_INVALID && says("batch")); a = good;
    a.K = 65; EXPECT(call(a) == VISTAF_E_INVALID && says("max_contacts")); a = good;
    a.span = 0; EXPECT(call(a) == VISTAF_E_INVALID && says("tangent_span")); a = good;
    a.span = 1025; EXPECT(call(a) == VISTAF_E_INVALID && says("tangent_span")); a = good;
    a.V = -1; EXPECT(call(a) == VISTAF_E_INVALID && says("max_stations")); a = good;
    a.tab = (const double *)((const char *)tab + 4); EXPECT(call(a) == VISTAF_E_INVALID && says("aligned") && says("d_contacts")); a = good;
    a.offs = (int32_t *)((char *)offs + 2); EXPECT(call(a) == VISTAF_E_INVALID && says("aligned") && says("d_offsets")); a = good;
    a.dep = (const float *)((const char *)dep + 1); EXPECT(call(a) == VISTAF_E_INVALID && says("aligned") && says("d_depth_mm")); a = good;
    a.ws = ws + 64; EXPECT(call(a) == VISTAF_E_INVALID && says("d_workspace") && says("aligned")); a = good;
    a.n = bytes - 1; EXPECT(call(a) == VISTAF_E_INVALID && says("workspace_bytes")); a = good;
    a.n = 0; EXPECT(call(a) == VISTAF_E_INVALID && says("workspace_bytes"));
    std::printf("centreline host check ok\n");
    return 0;
}
