// Stand-alone host check of the lobe read-out's C ABI (include_ext/vistaf_lobes.h): the argument checking of both functions, the tier rule and
// the workspace layout, for a run under the host sanitizers.  It includes the translation unit itself, so lobes_scratch is the one the library
// carves with; every call here is refused before a launch, nothing needs a device.  Build and run (no GPU needed):
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -o lobes_host_check tests/diag/lobes_host_check.hip
//   ASAN_OPTIONS=detect_leaks=0 ./lobes_host_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../vistaf-roboskin-vision-integrated-multimodal-sensor_amd/csrc/k_lobes.hip"

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
    EXPECT(vistaf_lobes_workspace_bytes(8, 8, 1, 8, nullptr) == VISTAF_E_INVALID && says("bytes"));
    const struct { int h, w, b, k; const char *word; } bad[] = {
        {0, 8, 1, 8, "h "}, {32768, 8, 1, 8, "h "}, {8, 0, 1, 8, "w "}, {8, 32768, 1, 8, "w "}, {32767, 32767, 1, 8, "h * w"}, {8, 8, 0, 8, "batch"},
        {8, 8, -1, 8, "batch"}, {8, 8, (1 << 24) + 1, 8, "batch"}, {8, 8, 1, 0, "max_contacts"}, {8, 8, 1, 65, "max_contacts"}};
    for (const auto &a : bad) {
        bytes = 1;
        EXPECT(vistaf_lobes_workspace_bytes(a.h, a.w, a.b, a.k, &bytes) == VISTAF_E_INVALID && bytes == 0 && says(a.word));
    }

    // the tier rule: monotone in both sizes, the launch's LDS never above the budget, the row's tables as the header of the hook counts them
    EXPECT(vistaf_ftp_test_lobes_tier(0, 8) == VISTAF_E_INVALID && says("bw") && vistaf_ftp_test_lobes_tier(8, 32768) == VISTAF_E_INVALID && says("bh"));
    EXPECT(vistaf_ftp_test_lobes_tier(48, 48) == 1 && vistaf_ftp_test_lobes_tier(1, 1) == 1 && vistaf_ftp_test_lobes_tier(32767, 32767) == 0);
    for (int n = 1; n < 400; n++) {
        EXPECT(!lb_box_in_lds(n, n) || (lb_box_in_lds(n - 1 > 0 ? n - 1 : 1, n) && lb_box_in_lds(n, n - 1 > 0 ? n - 1 : 1)));
        EXPECT(lb_launch_lds(n, n) <= (size_t)LB_LDS_BUDGET && (!lb_box_in_lds(n, n) || lb_launch_lds(n, n) == lb_row_bytes(n, n)));
        const size_t mc = (size_t)((n + 1) / 2) * ((n + 1) / 2);
        EXPECT(lb_max_cap(n, n) == mc && lb_pow2(mc) >= mc && lb_pow2(mc) < 2 * mc && (lb_pow2(mc) & (lb_pow2(mc) - 1)) == 0);
        EXPECT(lb_row_bytes(n, n) == 12 * (size_t)n * n + 32 * mc + 8 * lb_pow2(mc) && lb_row_bytes(n, n) % 4 == 0);
    }

    // the layout: sized with a null base, carved from a buffer of exactly that size; every region is written to its last element; the row
    // tables are there exactly when a box of the whole frame leaves LDS, and the last row's tables end inside the region
    const struct { int B, h, w, K; } shapes[] = {{1, 1, 1, 1}, {3, 24, 32, 8}, {2, 37, 53, 8}, {5, 7, 201, 64}, {2, 224, 224, 8}, {2, 263, 263, 3}, {1, 9, 4000, 2}};
    for (const auto &sh : shapes) {
        ScratchRec rec;
        EXPECT(vistaf_lobes_workspace_bytes(sh.h, sh.w, sh.B, sh.K, &bytes) == 0);
        EXPECT(bytes == lobes_scratch_bytes(sh.B, sh.h, sh.w, sh.K, &rec) && rec.size() == 4);
        uint8_t *base = (uint8_t *)std::aligned_alloc(256, (bytes + 255) & ~(size_t)255);
        EXPECT(base);
        ScratchLayout carve(base);
        const LobesBufs bf = lobes_scratch(carve, sh.B, sh.h, sh.w, sh.K);
        EXPECT(carve.bytes() == bytes && rec.back().offset + rec.back().bytes == bytes);
        for (size_t i = 0; i + 1 < rec.size(); i++) EXPECT(rec[i].offset % 256 == 0 && rec[i].offset + rec[i].bytes <= rec[i + 1].offset);
        const size_t P = (size_t)sh.h * sh.w, rows = (size_t)sh.B * sh.K;
        EXPECT((bf.row_stride == 0) == lb_box_in_lds(sh.w, sh.h) && bf.row_stride % 256 == 0 && (bf.row_stride == 0 || bf.row_stride >= lb_row_bytes(sh.w, sh.h)));
        const struct { void *p; size_t n; } regions[] = {{bf.aux, rows * LB_MAXL * LB_AUX * 8}, {bf.rank, rows * LB_MAXL * 4}, {bf.plane, sh.B * P},
                                                         {bf.rows, rows * bf.row_stride}};
        for (size_t i = 0; i < 4; i++) {
            EXPECT((uint8_t *)regions[i].p == base + rec[i].offset && regions[i].n == rec[i].bytes);
            std::memset(regions[i].p, 0x5a, regions[i].n);
        }
        if (bf.row_stride) {
            uint8_t *last = bf.rows + (rows - 1) * bf.row_stride;                      // as k_lobes_rows cuts it
            EXPECT(last + lb_row_bytes(sh.w, sh.h) <= base + bytes);
        }
        std::free(base);
    }

    // measure: every refusal comes before any HIP call and names its argument
    alignas(256) static uint8_t ws[32768];
    alignas(8) static double tab[8 * 16], mpp[1], lobes[8 * 4 * 16], rows[8 * 12], split[8 * 16];
    alignas(4) static int32_t cnt[1], scount[1], parent[16];
    alignas(4) static float dep[64];
    static int8_t idx[64], lidx[64], sidx[64];
    EXPECT(vistaf_lobes_workspace_bytes(8, 8, 1, 8, &bytes) == 0 && bytes > 0 && bytes <= sizeof ws);
    struct Args { const int8_t *idx; const double *tab; const int32_t *cnt; const double *mpp; const float *dep; int B, h, w, K, L; double pmm, pfrac, eps;
                  double *lobes, *rows; int8_t *lidx; double *split; int32_t *scount; int8_t *sidx; int32_t *parent; void *ws; size_t n; };
    const Args good{idx, tab, cnt, mpp, dep, 1, 8, 8, 8, 4, 0.02, 0.1, 0.01, lobes, rows, lidx, split, scount, sidx, parent, ws, bytes};
    auto call = [](const Args &a) {
        return vistaf_lobes_measure(a.idx, a.tab, a.cnt, a.mpp, a.dep, a.B, a.h, a.w, a.K, a.L, a.pmm, a.pfrac, a.eps, a.lobes, a.rows, a.lidx, a.split,
                                    a.scount, a.sidx, a.parent, a.ws, a.n, nullptr);
    };
    Args a = good;
    a.idx = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_contact_index")); a = good;
    a.tab = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_contacts")); a = good;
    a.cnt = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_count")); a = good;
    a.mpp = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_mm_per_px")); a = good;
    a.dep = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_depth_mm")); a = good;
    a.lobes = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_lobes")); a = good;
    a.rows = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_rows")); a = good;
    a.ws = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_workspace")); a = good;
    a.split = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_split_contacts") && says("all")); a = good;
    a.scount = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_split_count")); a = good;
    a.sidx = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_split_index")); a = good;
    a.parent = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_split_parent")); a = good;
    a.split = nullptr; a.scount = nullptr; a.sidx = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_split_parent")); a = good;
    a.h = 0; EXPECT(call(a) == VISTAF_E_INVALID && says("h ")); a = good;
    a.w = 40000; EXPECT(call(a) == VISTAF_E_INVALID && says("w ")); a = good;
    a.B = 0; EXPECT(call(a) == VISTAF_E_INVALID && says("batch")); a = good;
    a.K = 65; EXPECT(call(a) == VISTAF_E_INVALID && says("max_contacts")); a = good;
    a.L = 0; EXPECT(call(a) == VISTAF_E_INVALID && says("max_lobes")); a = good;
    a.L = 65; EXPECT(call(a) == VISTAF_E_INVALID && says("max_lobes")); a = good;
    a.pmm = -0.1; EXPECT(call(a) == VISTAF_E_INVALID && says("min_prominence_mm")); a = good;
    a.pmm = NAN; EXPECT(call(a) == VISTAF_E_INVALID && says("min_prominence_mm")); a = good;
    a.pfrac = INFINITY; EXPECT(call(a) == VISTAF_E_INVALID && says("min_prominence_frac")); a = good;
    a.pfrac = -1.0; EXPECT(call(a) == VISTAF_E_INVALID && says("min_prominence_frac")); a = good;
    a.eps = NAN; EXPECT(call(a) == VISTAF_E_INVALID && says("depth_eps_mm")); a = good;
    a.eps = -1e-9; EXPECT(call(a) == VISTAF_E_INVALID && says("depth_eps_mm")); a = good;
    a.tab = (const double *)((const char *)tab + 4); EXPECT(call(a) == VISTAF_E_INVALID && says("aligned") && says("d_contacts")); a = good;
    a.rows = (double *)((char *)rows + 4); EXPECT(call(a) == VISTAF_E_INVALID && says("aligned") && says("d_rows")); a = good;
    a.parent = (int32_t *)((char *)parent + 2); EXPECT(call(a) == VISTAF_E_INVALID && says("aligned") && says("d_split_parent")); a = good;
    a.dep = (const float *)((const char *)dep + 1); EXPECT(call(a) == VISTAF_E_INVALID && says("aligned") && says("d_depth_mm")); a = good;
    a.ws = ws + 64; EXPECT(call(a) == VISTAF_E_INVALID && says("d_workspace") && says("aligned")); a = good;
    a.n = bytes - 1; EXPECT(call(a) == VISTAF_E_INVALID && says("workspace_bytes")); a = good;
    a.n = 0; EXPECT(call(a) == VISTAF_E_INVALID && says("workspace_bytes"));
    std::printf("lobes host check ok\n");
    return 0;
}
