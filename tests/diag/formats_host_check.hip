// Stand-alone host check of the input frame layouts (include/vistaf_ftp.h, VISTAF_FMT_*): frame_layout of csrc/host_util.hpp -- the one
// function api.hip refuses by and launch_to_gray strides by -- against the header's table, every format over every size 2..260, plus the
// codes and sizes it has to refuse, for a run under the host sanitizers.  Nothing here launches a kernel or needs a device.  Build and run:
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -o formats_host_check tests/diag/formats_host_check.hip
//   ASAN_OPTIONS=detect_leaks=0 ./formats_host_check
#include <cstdio>
#include <cstring>

#include "../../vistaf-roboskin-vision-integrated-multimodal-sensor_amd/csrc/host_util.hpp"

#define EXPECT(c)                                                                                                        \
    do {                                                                                                                 \
        if (!(c)) { std::printf("FAILED line %d: %s (format %d, %d x %d)\n", __LINE__, #c, f, h, w); return 1; }       \
    } while (0)

int main()
{
    // the header's table, restated: bytes of one pixel's share (numerator / denominator), alignment, which of h and w must be even
    const struct { int code, num, den, align, even_h, even_w; const char *name; } table[] = {
        {VISTAF_FMT_GRAY_U8, 1, 1, 1, 0, 0, nullptr},     {VISTAF_FMT_BGR_U8, 3, 1, 1, 0, 0, nullptr},       {VISTAF_FMT_GRAY_F16, 2, 1, 2, 0, 0, nullptr},
        {VISTAF_FMT_BGR_F16, 6, 1, 2, 0, 0, nullptr},     {VISTAF_FMT_RGB_U8, 3, 1, 1, 0, 0, nullptr},       {VISTAF_FMT_BGRA_U8, 4, 1, 4, 0, 0, nullptr},
        {VISTAF_FMT_RGBA_U8, 4, 1, 4, 0, 0, nullptr},     {VISTAF_FMT_YUYV_U8, 2, 1, 4, 0, 1, "YUYV"},       {VISTAF_FMT_UYVY_U8, 2, 1, 4, 0, 1, "UYVY"},
        {VISTAF_FMT_NV12_U8, 3, 2, 1, 1, 1, "NV12"},      {VISTAF_FMT_BAYER_RGGB_U8, 1, 1, 1, 0, 0, nullptr}, {VISTAF_FMT_BAYER_GRBG_U8, 1, 1, 1, 0, 0, nullptr},
        {VISTAF_FMT_BAYER_GBRG_U8, 1, 1, 1, 0, 0, nullptr}, {VISTAF_FMT_BAYER_BGGR_U8, 1, 1, 1, 0, 0, nullptr}};
    int f = 0, h = 0, w = 0, n = 0;
    for (const auto &t : table) {
        f = t.code;
        EXPECT(f == n++);                                                           // the codes are 0..13 without a gap
        for (h = 2; h <= 260; h++)
            for (w = 2; w <= 260; w++) {
                const vf::FrameLayout fl = vf::frame_layout(f, h, w);
                if ((t.even_h && h % 2) || (t.even_w && w % 2)) {
                    EXPECT(fl.refusal && fl.bytes == 0 && fl.align == 0 && std::strstr(fl.refusal, t.name));      // the refusal names the format
                    continue;
                }
                EXPECT(!fl.refusal && fl.align == t.align);
                EXPECT(fl.bytes * t.den == (size_t)h * w * t.num);
                EXPECT(fl.bytes % fl.align == 0);                                   // so every frame of a batch keeps the first one's alignment
            }
    }
    EXPECT(n == 14);
    // the two strides the kernels must not assume more about
    f = VISTAF_FMT_NV12_U8, h = 150, w = 202;
    EXPECT(vf::frame_layout(f, h, w).bytes == 45450 && 45450 % 4 == 2);
    f = VISTAF_FMT_YUYV_U8, h = 151, w = 202;
    EXPECT(vf::frame_layout(f, h, w).bytes == 61004 && 61004 % 8 == 4);
    // what is refused: codes outside 0..13, sizes below 1 x 1, mosaics below 2 x 2
    h = w = 64;
    for (int code : {-1, 14, 15, 255, -2147483647 - 1, 2147483647}) {
        f = code;
        EXPECT(vf::frame_layout(f, h, w).refusal && std::strstr(vf::frame_layout(f, h, w).refusal, "format"));
    }
    for (f = 0; f < 14; f++)
        for (const auto &z : {std::pair<int, int>{0, 8}, {8, 0}, {-2, 8}, {8, -2}}) {
            h = z.first, w = z.second;
            EXPECT(vf::frame_layout(f, h, w).refusal);
        }
    for (f = VISTAF_FMT_BAYER_RGGB_U8; f <= VISTAF_FMT_BAYER_BGGR_U8; f++) {
        h = 1, w = 8;
        EXPECT(vf::frame_layout(f, h, w).refusal && std::strstr(vf::frame_layout(f, h, w).refusal, "Bayer"));
        h = 8, w = 1;
        EXPECT(vf::frame_layout(f, h, w).refusal);
    }
    f = VISTAF_FMT_GRAY_U8, h = 1, w = 1;
    EXPECT(!vf::frame_layout(f, h, w).refusal && vf::frame_layout(f, h, w).bytes == 1);
    // the largest frame create accepts in either direction does not wrap the byte count
    f = VISTAF_FMT_BGR_F16, h = 46340, w = 46340;
    EXPECT(vf::frame_layout(f, h, w).bytes == (size_t)6 * 46340 * 46340);
    std::printf("formats host check ok\n");
    return 0;
}
