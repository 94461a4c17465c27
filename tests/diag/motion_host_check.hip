// Stand-alone host check of the motion read-out's C ABI (include/vistaf_motion.h): the argument checking of create / update / reset and the
// scratch layout, for a run under the host sanitizers.  It includes the translation unit itself, so the anonymous namespace's motion_scratch
// is the one the library carves with; nothing here launches a kernel or needs a device.  Build and run (no GPU needed):
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -o motion_host_check tests/diag/motion_host_check.hip
//   ASAN_OPTIONS=detect_leaks=0 ./motion_host_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "../../vistaf-roboskin-vision-integrated-multimodal-sensor_amd/csrc/k_motion.hip"

static std::string g_last;
namespace vf {
int set_error(int code, const std::string &msg) { g_last = msg; return code; }
}  // namespace vf

#define EXPECT(c)                                                                 \
    do {                                                                          \
        if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } \
    } while (0)

int main()
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    vistaf_motion_handle *mo = nullptr;
    EXPECT(vistaf_motion_create(8, 8, 1, 8, 8, 1e-3, 16, 1, nullptr) == VISTAF_E_INVALID);
    const struct { int h, w, b, k, it; double tol; int mp, ic; } bad[] = {
        {0, 8, 1, 8, 8, 1e-3, 16, 1}, {8, 0, 1, 8, 8, 1e-3, 16, 1}, {8, 8, 0, 8, 8, 1e-3, 16, 1}, {8, 8, 1, 0, 8, 1e-3, 16, 1}, {8, 8, 1, 65, 8, 1e-3, 16, 1},
        {8, 8, 1, 8, 0, 1e-3, 16, 1}, {8, 8, 1, 8, 17, 1e-3, 16, 1}, {8, 8, 1, 8, 8, -1.0, 16, 1}, {8, 8, 1, 8, 8, nan, 16, 1}, {8, 8, 1, 8, 8, inf, 16, 1},
        {8, 8, 1, 8, 8, 1e-3, 0, 1}, {8, 8, 1, 8, 8, 1e-3, 16, 2}, {65536, 65536, 1, 8, 8, 1e-3, 16, 1}, {8, 8, 65536, 8, 8, 1e-3, 16, 1}};
    for (const auto &a : bad) {
        EXPECT(vistaf_motion_create(a.h, a.w, a.b, a.k, a.it, a.tol, a.mp, a.ic, &mo) == VISTAF_E_INVALID);
        EXPECT(mo == nullptr && !g_last.empty());
    }
    EXPECT(vistaf_motion_create(5, 7, 2, 3, 8, 1e-3, 16, 1, &mo) == 0 && mo);
    alignas(8) static double buf[64];
    alignas(8) static float f32[16];
    static int8_t i8[16];
    static int32_t cnt[2];
    const void *good[10] = {f32, i8, buf, cnt, buf, buf, nullptr, nullptr, buf, buf};
    auto call = [&](const void **a, float eps, int B) {
        return vistaf_motion_update(mo, (const float *)a[0], (const int8_t *)a[1], (const double *)a[2], (const int32_t *)a[3], (const double *)a[4],
                                    (const double *)a[5], eps, B, (double *)a[8], (double *)a[9], nullptr);
    };
    EXPECT(vistaf_motion_update(nullptr, f32, i8, buf, cnt, buf, buf, 0.01f, 1, buf, buf, nullptr) == VISTAF_E_INVALID);
    for (int i : {0, 1, 2, 3, 4, 5, 8, 9}) {
        const void *a[10];
        std::memcpy(a, good, sizeof a);
        a[i] = nullptr;
        EXPECT(call(a, 0.01f, 1) == VISTAF_E_INVALID && g_last.find("null") != std::string::npos);
    }
    for (int B : {0, 3, -1}) EXPECT(call(good, 0.01f, B) == VISTAF_E_INVALID && g_last.find("batch") != std::string::npos);
    for (float eps : {(float)nan, (float)inf, -(float)inf}) EXPECT(call(good, eps, 1) == VISTAF_E_INVALID && g_last.find("depth_eps_mm") != std::string::npos);
    for (int i : {2, 4, 5, 8, 9}) {
        const void *a[10];
        std::memcpy(a, good, sizeof a);
        a[i] = (const char *)buf + 4;
        EXPECT(call(a, 0.01f, 1) == VISTAF_E_INVALID && g_last.find("aligned") != std::string::npos);
    }
    {
        const void *a[10];
        std::memcpy(a, good, sizeof a);
        a[0] = (const char *)f32 + 2;
        EXPECT(call(a, 0.01f, 1) == VISTAF_E_INVALID);
    }
    EXPECT(mo->buf == nullptr && !mo->have_carry);          // a refused update allocates nothing and carries nothing
    EXPECT(vistaf_motion_reset(nullptr) == VISTAF_E_INVALID && vistaf_motion_reset(mo) == 0);
    vistaf_motion_destroy(mo);
    vistaf_motion_destroy(nullptr);

    // the layout: sized with a null base, carved from a buffer of exactly that size; every region is written to its last byte
    const struct { size_t P; int K; } shapes[] = {{1, 1}, {35, 3}, {37 * 53, 4}, {224 * 224, 8}, {1182 * 1182, 64}};
    for (const auto &sh : shapes) {
        ScratchRec rec;
        ScratchLayout size(nullptr, &rec);
        const MoBufs none = motion_scratch(size, sh.P, sh.K);
        EXPECT(!none.depth && !none.index && !none.table && !none.count && rec.size() == 4);
        const size_t bytes = size.bytes();
        void *base = std::aligned_alloc(256, (bytes + 255) & ~(size_t)255);
        EXPECT(base);
        ScratchLayout carve(base);
        const MoBufs bf = motion_scratch(carve, sh.P, sh.K);
        EXPECT(carve.bytes() == bytes);
        size_t end = 0;
        for (const auto &r : rec) {
            EXPECT(r.offset >= end && r.offset % r.align == 0 && r.offset + r.bytes <= bytes);
            end = r.offset + r.bytes;
        }
        EXPECT((uint8_t *)bf.depth == (uint8_t *)base + rec[0].offset && (uint8_t *)bf.index == (uint8_t *)base + rec[1].offset &&
               (uint8_t *)bf.table == (uint8_t *)base + rec[2].offset && (uint8_t *)bf.count == (uint8_t *)base + rec[3].offset);
        EXPECT(rec[0].bytes == sh.P * 4 && rec[1].bytes == sh.P && rec[2].bytes == (size_t)sh.K * VISTAF_NCONTACT * 8 && rec[3].bytes == 4);
        for (size_t i = 0; i < sh.P; i++) { bf.depth[i] = 1.0f; bf.index[i] = 1; }
        for (int i = 0; i < sh.K * VISTAF_NCONTACT; i++) bf.table[i] = 1.0;
        bf.count[0] = 1;
        std::free(base);
    }
    std::printf("motion host check ok\n");
    return 0;
}
