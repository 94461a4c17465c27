// Stand-alone host check of the contact outline read-out's C ABI (include_ext/vistaf_outline.h): the argument checking of both functions and
// the workspace layout, for a run under the host sanitizers, and the capacity rule of the polylines (row_capacity, contact_rows.hpp: the one
// k_outline_poly and k_centreline_poly apply) against a direct restatement.  It includes the translation unit itself, so outline_scratch is the
// one the library carves with; every call here is refused before a launch, nothing needs a device.  Build and run (no GPU needed):
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -o outline_host_check tests/diag/outline_host_check.hip
//   ASAN_OPTIONS=detect_leaks=0 ./outline_host_check
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../vistaf-roboskin-vision-integrated-multimodal-sensor_amd/csrc/k_outline.hip"

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
    EXPECT(vistaf_outline_workspace_bytes(8, 8, 1, 8, nullptr) == VISTAF_E_INVALID && says("bytes"));
    const struct { int h, w, b, k; const char *word; } bad[] = {
        {0, 8, 1, 8, "h "}, {32768, 8, 1, 8, "h "}, {8, 0, 1, 8, "w "}, {8, 32768, 1, 8, "w "}, {32767, 32767, 1, 8, "h * w"}, {8, 8, 0, 8, "batch"},
        {8, 8, -1, 8, "batch"}, {8, 8, (1 << 24) + 1, 8, "batch"}, {8, 8, 1, 0, "max_contacts"}, {8, 8, 1, 65, "max_contacts"}};
    for (const auto &a : bad) {
        bytes = 1;
        EXPECT(vistaf_outline_workspace_bytes(a.h, a.w, a.b, a.k, &bytes) == VISTAF_E_INVALID && bytes == 0 && says(a.word));
    }

    // the layout: sized with a null base, carved from a buffer of exactly that size; every region is written to its last element and the
    // views a kernel takes of a frame's jump buffer stay inside it
    const struct { int B, h, w, K; } shapes[] = {{1, 1, 1, 1}, {3, 24, 32, 8}, {2, 33, 47, 8}, {5, 7, 201, 64}, {2, 224, 224, 8}};
    for (const auto &sh : shapes) {
        ScratchRec rec;
        EXPECT(vistaf_outline_workspace_bytes(sh.h, sh.w, sh.B, sh.K, &bytes) == 0);
        EXPECT(bytes == outline_scratch_bytes(sh.B, sh.h, sh.w, sh.K, &rec) && rec.size() == 10);
        uint8_t *base = (uint8_t *)std::aligned_alloc(256, (bytes + 255) & ~(size_t)255);
        EXPECT(base);
        ScratchLayout carve(base);
        const OutlineBufs bf = outline_scratch(carve, sh.B, sh.h, sh.w, sh.K);
        EXPECT(carve.bytes() == bytes && rec.back().offset + rec.back().bytes == bytes);
        for (size_t i = 0; i + 1 < rec.size(); i++) EXPECT(rec[i].offset % 256 == 0 && rec[i].offset + rec[i].bytes <= rec[i + 1].offset);
        const size_t rows = (size_t)sh.B * sh.K, P = (size_t)sh.h * sh.w;
        const struct { void *p; size_t n; } regions[] = {{bf.cnt, rows * 2 * 4}, {bf.tcnt, rows * 1024 * 4}, {bf.meta, rows * 4 * 4}, {bf.rowlo, rows * sh.h * 4}, {bf.rowhi, rows * sh.h * 4},
            {bf.off, sh.B * P * 4}, {bf.next, sh.B * P * 16}, {bf.vtx, sh.B * P * 16},
            {bf.jump[0], sh.B * P * 48}, {bf.jump[1], sh.B * P * 48}};
        for (size_t i = 0; i < 10; i++) {
            EXPECT((uint8_t *)regions[i].p == base + rec[i].offset && regions[i].n == rec[i].bytes);
            std::memset(regions[i].p, 0x5a, regions[i].n);
        }
        // a frame's jump planes, as OlJump cuts them: the last frame's distance plane ends with the region
        uint8_t *ahead = (uint8_t *)(bf.jump[1] + (size_t)(sh.B - 1) * P * 6);
        EXPECT(ahead + 12 * P * 4 == (uint8_t *)bf.jump[1] + rec[9].bytes);
        std::free(base);
    }

    // measure: every refusal comes before any HIP call and names its argument
    alignas(256) static uint8_t ws[4096];
    alignas(8) static double tab[8 * 16], mpp[1], out[8 * 24];
    alignas(4) static int32_t cnt[1], verts[64], offs[9];
    static int8_t idx[64];
    EXPECT(vistaf_outline_workspace_bytes(8, 8, 1, 8, &bytes) == 0 && bytes > sizeof ws);
    struct Args { const int8_t *idx; const double *tab; const int32_t *cnt; const double *mpp; int B, h, w, K, V; double *out; int32_t *verts, *offs; void *ws; size_t n; };
    const Args good{idx, tab, cnt, mpp, 1, 8, 8, 8, 32, out, verts, offs, ws, bytes};
    auto call = [](const Args &a) {
        return vistaf_outline_measure(a.idx, a.tab, a.cnt, a.mpp, a.B, a.h, a.w, a.K, a.V, a.out, a.verts, a.offs, a.ws, a.n, nullptr);
    };
    Args a = good;
    a.idx = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_contact_index")); a = good;
    a.tab = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_contacts")); a = good;
    a.cnt = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_count")); a = good;
    a.mpp = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_mm_per_px")); a = good;
    a.out = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_outlines")); a = good;
    a.ws = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_workspace")); a = good;
    a.verts = nullptr; EXPECT(call(a) == VISTAF_E_INVALID && says("d_vertices") && says("d_offsets")); a = good;
    a.h = 0; EXPECT(call(a) == VISTAF_E_INVALID && says("h ")); a = good;
    a.w = 40000; EXPECT(call(a) == VISTAF_E_INVALID && says("w ")); a = good;
    a.B = 0; EXPECT(call(a) == VISTAF_E_INVALID && says("batch")); a = good;
    a.K = 65; EXPECT(call(a) == VISTAF_E_INVALID && says("max_contacts")); a = good;
    a.V = -1; EXPECT(call(a) == VISTAF_E_INVALID && says("max_vertices")); a = good;
    a.tab = (const double *)((const char *)tab + 4); EXPECT(call(a) == VISTAF_E_INVALID && says("aligned") && says("d_contacts")); a = good;
    a.offs = (int32_t *)((char *)offs + 2); EXPECT(call(a) == VISTAF_E_INVALID && says("aligned") && says("d_offsets")); a = good;
    a.ws = ws + 64; EXPECT(call(a) == VISTAF_E_INVALID && says("d_workspace") && says("aligned")); a = good;
    a.n = bytes - 1; EXPECT(call(a) == VISTAF_E_INVALID && says("workspace_bytes")); a = good;
    a.n = 0; EXPECT(call(a) == VISTAF_E_INVALID && says("workspace_bytes"));

    // the capacity rule, exhaustively: every count vector of K <= 4 rows with entries 0..3, every number of rows in use, every capacity 0..12.
    // The restatement walks the rows once: a row in use is written while no row before it was left out and it still fits.  Frame 1 of a
    // table of two, so that the frame stride counts; frame 0 holds counts that would overflow everything.
    for (int K = 1; K <= 4; K++) {
        int total = 1;
        for (int j = 0; j < K; j++) total *= 4;
        for (int code = 0; code < total; code++) {
            double table[2 * 4 * VISTAF_NOUTLINE];
            for (double &v : table) v = 1000.0;
            int c[4] = {0, 0, 0, 0};
            for (int j = 0, q = code; j < K; j++, q /= 4) {
                c[j] = q % 4;
                table[(size_t)(K + j) * VISTAF_NOUTLINE + VISTAF_OUTLINE_CORNERS] = (double)c[j];
            }
            for (int kk = 0; kk <= K; kk++)
                for (int cap = 0; cap <= 12; cap++) {
                    int run = 0, end = 0;
                    bool open = true;
                    for (int k = 0; k < K; k++) {
                        const bool fits = k < kk && open && run + c[k] <= cap;
                        if (k < kk && !fits) open = false;                    // the first row left out: nothing behind it is written
                        const RowCapacity got = row_capacity(table, VISTAF_NOUTLINE, VISTAF_OUTLINE_CORNERS, 1, K, k, kk, cap);
                        EXPECT(got.before == run && got.written == (fits ? c[k] : 0));
                        EXPECT(got.before == end && got.before + got.written <= cap);      // offsets[k] .. offsets[k + 1]: monotone, within V
                        EXPECT(open || got.written == 0);
                        end = got.before + got.written;
                        run += got.written;
                    }
                }
        }
    }
    std::printf("outline host check ok\n");
    return 0;
}
