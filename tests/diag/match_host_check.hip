// Stand-alone host check of the indenter match read-out's C ABI (include_ext/vistaf_match.h): every refusal of its four functions, the host bank
// builder -- which indexes arrays -- on a 3-template bank, and the workspace layout, for a run under the host sanitizers.  It includes the
// translation unit itself, so bank_layout and match_scratch are the ones the library uses; every measure call here is refused before a launch,
// nothing needs a device.  Build and run (no GPU needed):
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -o match_host_check tests/diag/match_host_check.hip
//   ASAN_OPTIONS=detect_leaks=0 ./match_host_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "../../vistaf-roboskin-vision-integrated-multimodal-sensor_amd/csrc/k_match.hip"

static std::string g_last;
namespace vf {
int set_error(int code, const std::string &msg) { g_last = msg; return code; }
}  // namespace vf

#define EXPECT(c)                                                                 \
    do {                                                                          \
        if (!(c)) { std::printf("FAILED line %d: %s (%s)\n", __LINE__, #c, g_last.c_str()); return 1; } \
    } while (0)

static bool says(const char *word) { return g_last.find(word) != std::string::npos; }

int main()
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    // ---- vistaf_match_bank_bytes
    size_t bytes = 1;
    const int32_t sym[3] = {0, 2, 1};
    EXPECT(vistaf_match_bank_bytes(3, 9, 12, sym, nullptr) == VISTAF_E_INVALID && says("bytes"));
    EXPECT(vistaf_match_bank_bytes(3, 9, 12, nullptr, &bytes) == VISTAF_E_INVALID && bytes == 0 && says("symmetry"));
    const struct { int T, P, R; int32_t s[3]; const char *word; } bad[] = {
        {0, 9, 12, {0, 2, 1}, "T "}, {65, 9, 12, {0, 2, 1}, "T "}, {3, 8, 12, {0, 2, 1}, "P "}, {3, 3, 12, {0, 2, 1}, "P "}, {3, 35, 12, {0, 2, 1}, "P "},
        {3, 9, 0, {0, 2, 1}, "R "}, {3, 9, 65, {0, 2, 1}, "R "}, {3, 9, 12, {0, 5, 1}, "R % symmetry"}, {3, 9, 12, {0, 9, 1}, "symmetry"},
        {3, 9, 12, {0, 2, -1}, "symmetry"}};
    for (const auto &a : bad) {
        bytes = 1;
        EXPECT(vistaf_match_bank_bytes(a.T, a.P, a.R, a.s, &bytes) == VISTAF_E_INVALID && bytes == 0 && says(a.word));
    }
    {
        int32_t many[64];
        for (int &v : many) v = 1;
        EXPECT(vistaf_match_bank_bytes(64, 9, 64, many, &bytes) == VISTAF_E_INVALID && says("2048"));
        for (int &v : many) v = 2;
        EXPECT(vistaf_match_bank_bytes(64, 33, 64, many, &bytes) == 0 && bytes == bank_layout(64, 33, 64, 2048, disc_count(33)).bytes);
    }
    EXPECT(disc_count(5) == 13 && disc_count(9) == 49 && disc_count(17) == 197);

    // ---- vistaf_match_build_bank on a 3-template bank: a cone, a ramp bar and an L, P = 9, R = 12 (M = 1 + 6 + 12 = 19, D = 49, Dp = 52)
    const int T = 3, P = 9, R = 12, M = 19, D = 49;
    float tp[3 * 9 * 9];
    for (int y = 0; y < P; y++)
        for (int x = 0; x < P; x++) {
            const double u = x - 4, v = y - 4;
            tp[y * P + x] = (float)std::max(0.0, 0.5 - 0.1 * std::sqrt(u * u + v * v));
            tp[81 + y * P + x] = std::fabs(v) <= 1 ? (float)(0.4 - 0.02 * u * u) : 0.0f;
            tp[162 + y * P + x] = (std::fabs(u) <= 1 && v <= 3) || (v >= 2 && v <= 3 && u >= 0) ? 0.4f : 0.0f;
        }
    const int32_t kl[3] = {0, 1, 2};
    EXPECT(vistaf_match_bank_bytes(T, P, R, sym, &bytes) == 0);
    const BankLayout L = bank_layout(T, P, R, M, D);
    EXPECT(bytes == L.bytes && L.Dp == 52 && L.cossin == 64 && L.rows % 256 == 0 && L.disc % 8 == 0 && L.mu % 8 == 0);
    // exactly the bytes, on the heap: a write past the end is the sanitizer's to see
    uint8_t *bank = (uint8_t *)std::aligned_alloc(256, (bytes + 255) & ~(size_t)255);
    EXPECT(bank);
    std::memset(bank, 0x5a, bytes);
    EXPECT(vistaf_match_build_bank(nullptr, kl, sym, T, P, R, 0.1, bank, bytes) == VISTAF_E_INVALID && says("templates"));
    EXPECT(vistaf_match_build_bank(tp, nullptr, sym, T, P, R, 0.1, bank, bytes) == VISTAF_E_INVALID && says("klass"));
    EXPECT(vistaf_match_build_bank(tp, kl, nullptr, T, P, R, 0.1, bank, bytes) == VISTAF_E_INVALID && says("symmetry"));
    EXPECT(vistaf_match_build_bank(tp, kl, sym, T, P, R, 0.1, nullptr, bytes) == VISTAF_E_INVALID && says("h_bank"));
    EXPECT(vistaf_match_build_bank(tp, kl, sym, T, 10, R, 0.1, bank, bytes) == VISTAF_E_INVALID && says("P "));
    EXPECT(vistaf_match_build_bank(tp, kl, sym, T, P, 11, 0.1, bank, bytes) == VISTAF_E_INVALID && says("R % symmetry"));
    EXPECT(vistaf_match_build_bank(tp, kl, sym, 0, P, R, 0.1, bank, bytes) == VISTAF_E_INVALID && says("T "));
    {
        const int32_t neg[3] = {0, 1, -4};
        EXPECT(vistaf_match_build_bank(tp, neg, sym, T, P, R, 0.1, bank, bytes) == VISTAF_E_INVALID && says("klass[2]"));
    }
    EXPECT(vistaf_match_build_bank(tp, kl, sym, T, P, R, 0.0, bank, bytes) == VISTAF_E_INVALID && says("template_mm_per_px"));
    EXPECT(vistaf_match_build_bank(tp, kl, sym, T, P, R, nan, bank, bytes) == VISTAF_E_INVALID && says("template_mm_per_px"));
    EXPECT(vistaf_match_build_bank(tp, kl, sym, T, P, R, inf, bank, bytes) == VISTAF_E_INVALID && says("template_mm_per_px"));
    EXPECT(vistaf_match_build_bank(tp, kl, sym, T, P, R, 0.1, bank + 4, bytes) == VISTAF_E_INVALID && says("aligned"));
    EXPECT(vistaf_match_build_bank(tp, kl, sym, T, P, R, 0.1, bank, bytes - 8) == VISTAF_E_INVALID && says("bank_bytes"));
    EXPECT(vistaf_match_build_bank(tp, kl, sym, T, P, R, 0.1, bank, bytes + 8) == VISTAF_E_INVALID && says("bank_bytes"));
    {
        float flat[3 * 81];
        std::memcpy(flat, tp, sizeof flat);
        for (int i = 0; i < 81; i++) flat[81 + i] = 0.25f;
        EXPECT(vistaf_match_build_bank(flat, kl, sym, T, P, R, 0.1, bank, bytes) == VISTAF_E_INVALID && says("templates[1]") && says("flat"));
        std::memcpy(flat, tp, sizeof flat);
        flat[162 + 40] = std::numeric_limits<float>::infinity();
        EXPECT(vistaf_match_build_bank(flat, kl, sym, T, P, R, 0.1, bank, bytes) == VISTAF_E_INVALID && says("templates[2]") && says("finite"));
    }
    EXPECT(vistaf_match_build_bank(tp, kl, sym, T, P, R, 0.1, bank, bytes) == 0);
    const int32_t *hdr = (const int32_t *)bank;
    EXPECT(hdr[0] == VISTAF_MATCH_MAGIC && hdr[1] == T && hdr[2] == P && hdr[3] == R && hdr[4] == M && hdr[5] == D && hdr[6] == 52 && hdr[7] == 0);
    double tmpp;
    std::memcpy(&tmpp, hdr + 8, 8);
    EXPECT(tmpp == 0.1);
    const BankView bv = bank_view(bank, L, tmpp);
    EXPECT(bv.cossin[0] == 1.0 && bv.cossin[1] == 0.0 && std::fabs(bv.cossin[2 * 3 + 1] - 1.0) < 1e-15);
    EXPECT(bv.rowtab[0] == 0 && bv.rowtab[1] == 0 && bv.rowtab[2] == 1 && bv.rowtab[2 * 6 + 1] == 5 && bv.rowtab[2 * 7] == 2 && bv.rowtab[2 * 18 + 1] == 11);
    EXPECT(bv.klass[2] == 2 && bv.symmetry[1] == 2 && bv.disc[0] == 0 && bv.disc[1] == -4 && bv.disc[2 * 48] == 0 && bv.disc[2 * 48 + 1] == 4);
    for (int row = 0; row < M; row++) {
        double s = 0.0, ss = 0.0;
        for (int j = 0; j < D; j++) { s += bv.rows[row * 52 + j]; ss += bv.rows[row * 52 + j] * bv.rows[row * 52 + j]; }
        EXPECT(std::fabs(s) < 1e-13 && std::fabs(ss - 1.0) < 1e-13 && bv.norm[row] > 0.0 && std::isfinite(bv.mu[row]));
        for (int j = D; j < 52; j++) EXPECT(bv.rows[row * 52 + j] == 0.0);
    }
    EXPECT((const uint8_t *)(bv.rows + (size_t)M * 52) == bank + bytes);

    // ---- vistaf_match_workspace_bytes and the layout
    size_t wsb = 1;
    EXPECT(vistaf_match_workspace_bytes(40, 48, 1, 2, 9, 2, 19, nullptr) == VISTAF_E_INVALID && says("bytes"));
    const struct { int h, w, b, k, p, m, rows; const char *word; } badw[] = {
        {0, 48, 1, 2, 9, 2, 19, "h "}, {40, 0, 1, 2, 9, 2, 19, "w "}, {65536, 65536, 1, 2, 9, 2, 19, "h * w"}, {40, 48, 0, 2, 9, 2, 19, "max_batch"},
        {40, 48, (1 << 19) + 1, 2, 9, 2, 19, "max_batch"}, {40, 48, 1, 0, 9, 2, 19, "max_contacts"}, {40, 48, 1, 65, 9, 2, 19, "max_contacts"},
        {40, 48, 1, 2, 8, 2, 19, "P "}, {40, 48, 1, 2, 35, 2, 19, "P "}, {40, 48, 1, 2, 9, -1, 19, "max_shift"}, {40, 48, 1, 2, 9, 9, 19, "max_shift"},
        {40, 48, 1, 2, 9, 2, 0, "M "}, {40, 48, 1, 2, 9, 2, 2049, "M "}};
    for (const auto &a : badw) {
        wsb = 1;
        EXPECT(vistaf_match_workspace_bytes(a.h, a.w, a.b, a.k, a.p, a.m, a.rows, &wsb) == VISTAF_E_INVALID && wsb == 0 && says(a.word));
    }
    const struct { int B, K, m, M; } shapes[] = {{1, 1, 0, 1}, {3, 8, 2, 19}, {2, 4, 8, 2048}, {5, 64, 3, 37}, {256, 4, 4, 256}};
    for (const auto &sh : shapes) {
        ScratchRec rec;
        EXPECT(vistaf_match_workspace_bytes(37, 53, sh.B, sh.K, 9, sh.m, sh.M, &wsb) == 0);
        EXPECT(wsb == match_scratch_bytes(sh.B, sh.K, sh.m, sh.M, &rec) && rec.size() == 7);
        uint8_t *base = (uint8_t *)std::aligned_alloc(256, (wsb + 255) & ~(size_t)255);
        EXPECT(base);
        ScratchLayout carve(base);
        const MatchBufs bf = match_scratch(carve, sh.B, sh.K, sh.m, sh.M);
        EXPECT(carve.bytes() == wsb && rec.back().offset + rec.back().bytes == wsb);
        for (size_t i = 0; i + 1 < rec.size(); i++) EXPECT(rec[i].offset % 256 == 0 && rec[i].offset + rec[i].bytes <= rec[i + 1].offset);
        const size_t n = (size_t)sh.B * sh.K, ns = (size_t)(2 * sh.m + 1) * (2 * sh.m + 1);
        // the last element the kernels write of every region
        bf.pre[n * MT_NPRE - 1] = 1.0; bf.s1[n * ns - 1] = 1.0; bf.var[n * ns - 1] = 1.0; bf.nz[n * ns - 1] = 1;
        bf.bscore[n * sh.M - 1] = 1.0; bf.bg[n * sh.M - 1] = 1.0; bf.bshift[n * sh.M - 1] = 1;
        EXPECT((uint8_t *)(bf.bshift + n * sh.M) == base + wsb);
        for (int b = 1; b < sh.B; b += 7) EXPECT(match_scratch_bytes(b, sh.K, sh.m, sh.M) <= wsb);
        std::free(base);
    }

    // ---- vistaf_match_measure: every refusal comes before any HIP call and names its argument
    EXPECT(vistaf_match_workspace_bytes(40, 48, 1, 2, 9, 2, 19, &wsb) == 0);
    uint8_t *ws = (uint8_t *)std::aligned_alloc(256, (wsb + 255) & ~(size_t)255);
    EXPECT(ws);
    alignas(8) static double tab[2 * 16], mpp[1], out[2 * 24], sc[2 * 3];
    alignas(4) static float depth[40 * 48], pat[2 * 13 * 13];
    alignas(4) static int32_t cnt[1];
    static int8_t idx[40 * 48];
    struct Args {
        const float *depth; const int8_t *idx; const double *tab; const int32_t *cnt; const double *mpp; const void *bank; size_t nb; const int32_t *hdr;
        float eps; int m, minpix; double acs, acm; int h, w, B, K; double *out, *sc; float *pat; void *ws; size_t n;
    };
    const Args good{depth, idx, tab, cnt, mpp, bank, bytes, hdr, 0.01f, 2, 6, 0.7, 0.05, 40, 48, 1, 2, out, sc, pat, ws, wsb};
    auto call = [](const Args &a) {
        return vistaf_match_measure(a.depth, a.idx, a.tab, a.cnt, a.mpp, a.bank, a.nb, a.hdr, a.eps, a.m, a.minpix, a.acs, a.acm, a.h, a.w, a.B, a.K, a.out,
                                    a.sc, a.pat, a.ws, a.n, nullptr);
    };
    Args a = good;
    a.depth = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_depth_mm")); a = good;
    a.idx = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_contact_index")); a = good;
    a.tab = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_contacts")); a = good;
    a.cnt = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_count")); a = good;
    a.mpp = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_mm_per_px")); a = good;
    a.bank = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_bank")); a = good;
    a.hdr = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("h_bank_header")); a = good;
    a.out = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_matches")); a = good;
    a.sc = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_scores")); a = good;
    a.pat = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_patches")); a = good;
    a.ws = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_workspace")); a = good;
    {
        int32_t h2[VISTAF_MATCH_HEADER_INTS];
        const struct { int at, value; const char *word; } edits[] = {{0, 7, "h_bank_header"}, {1, 0, "h_bank_header"}, {1, 65, "h_bank_header"}, {2, 10, "h_bank_header"},
                                                                    {3, 0, "h_bank_header"}, {4, 0, "h_bank_header"}, {4, 37, "h_bank_header"}, {5, 50, "h_bank_header"},
                                                                    {6, 49, "h_bank_header"}, {9, 0x7ff80000, "h_bank_header"}, {4, 20, "bank_bytes"}, {3, 24, "bank_bytes"}};
        for (const auto &e : edits) {
            std::memcpy(h2, hdr, sizeof h2);
            h2[e.at] = e.value;
            a.hdr = h2;
            EXPECT(call(a) == VISTAF_E_INVALID && says(e.word));
        }
        a = good;
    }
    a.nb = bytes - 8; EXPECT(call(a) == VISTAF_E_INVALID && says("bank_bytes")); a = good;
    a.h = 0; EXPECT(call(a) == VISTAF_E_INVALID && says("h ")); a = good;
    a.w = -2; EXPECT(call(a) == VISTAF_E_INVALID && says("w ")); a = good;
    a.h = a.w = 65536; EXPECT(call(a) == VISTAF_E_INVALID && says("h * w")); a = good;
    a.B = 0; EXPECT(call(a) == VISTAF_E_INVALID && says("batch")); a = good;
    a.K = 0; EXPECT(call(a) == VISTAF_E_INVALID && says("max_contacts")); a = good;
    a.K = 65; EXPECT(call(a) == VISTAF_E_INVALID && says("max_contacts")); a = good;
    a.m = -1; EXPECT(call(a) == VISTAF_E_INVALID && says("max_shift")); a = good;
    a.m = 9; EXPECT(call(a) == VISTAF_E_INVALID && says("max_shift")); a = good;
    a.eps = std::numeric_limits<float>::infinity(); EXPECT(call(a) == VISTAF_E_INVALID && says("depth_eps_mm")); a = good;
    a.eps = std::numeric_limits<float>::quiet_NaN(); EXPECT(call(a) == VISTAF_E_INVALID && says("depth_eps_mm")); a = good;
    a.minpix = 0; EXPECT(call(a) == VISTAF_E_INVALID && says("min_pixels")); a = good;
    a.acs = nan; EXPECT(call(a) == VISTAF_E_INVALID && says("accept_score")); a = good;
    a.acs = inf; EXPECT(call(a) == VISTAF_E_INVALID && says("accept_score")); a = good;
    a.acm = nan; EXPECT(call(a) == VISTAF_E_INVALID && says("accept_margin")); a = good;
    a.tab = (const double *)((const char *)tab + 4); EXPECT(call(a) == VISTAF_E_INVALID && says("aligned") && says("d_contacts")); a = good;
    a.bank = bank + 4; EXPECT(call(a) == VISTAF_E_INVALID && says("aligned") && says("d_bank")); a = good;
    a.pat = (float *)((char *)pat + 2); EXPECT(call(a) == VISTAF_E_INVALID && says("aligned") && says("d_patches")); a = good;
    a.ws = ws + 64; EXPECT(call(a) == VISTAF_E_INVALID && says("d_workspace") && says("aligned")); a = good;
    a.n = wsb - 1; EXPECT(call(a) == VISTAF_E_INVALID && says("workspace_bytes")); a = good;
    a.n = 0; EXPECT(call(a) == VISTAF_E_INVALID && says("workspace_bytes")); a = good;
    a.B = 2; EXPECT(call(a) == VISTAF_E_INVALID && says("workspace_bytes")); a = good;      // sized for one frame
    a.m = 3; EXPECT(call(a) == VISTAF_E_INVALID && says("workspace_bytes"));                // and for 25 shifts
    std::free(ws);
    std::free(bank);
    std::printf("match host check ok\n");
    return 0;
}
