// Stand-alone host check of what the phase-unwrap kernels share through csrc/unwrap.hpp and no GPU test states on its own: the wrap rule
// against a literal restatement, the multiply-high row index over whole padded frames and the boundary of its exactness, the padded index
// round trip, the neighbour slots, the rank plane's stride and the tiers at their thresholds, for a run under the host sanitizers.  Nothing
// here launches a kernel or needs a device.  Build and run:
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -o unwrap_host_check tests/diag/unwrap_host_check.hip
//   ASAN_OPTIONS=detect_leaks=0 ./unwrap_host_check
#include <cstdio>
#include <vector>

#include "../../vistaf-roboskin-vision-integrated-multimodal-sensor_amd/csrc/unwrap.hpp"

using namespace vf;

#define EXPECT(c)                                                                 \
    do {                                                                          \
        if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } \
    } while (0)

// the rule as the kernels' header comments state it, without wrap_count's rint: the integer k with d + 2 pi k in (-pi, pi], searched
static int wrap_literal(double d)
{
    const double twopi = 6.283185307179586476925286766559, pi_d = 3.14159265358979323846;
    for (int k = -4; k <= 4; k++) {
        const double dd = d + twopi * (double)k;
        if (dd > -pi_d && dd <= pi_d) return k;
    }
    return 99;
}

int main()
{
    // ---- wrap_count on [-4 pi, 4 pi]: a grid, and the points where the count changes or float32 meets float64, with their float64 neighbours
    {
        const double pi_d = 3.14159265358979323846, pi_f = (double)3.14159274f;
        std::vector<double> ds;
        for (int i = -4000; i <= 4000; i++) ds.push_back(4.0 * pi_d * (double)i / 4000.0);
        for (double c : {pi_d, -pi_d, pi_f, -pi_f, 3.0 * pi_d, -3.0 * pi_d, 0.0}) {
            ds.push_back(c);
            ds.push_back(std::nextafter(c, 1e300));
            ds.push_back(std::nextafter(c, -1e300));
        }
        for (double d : ds) {
            const int k = wrap_count(d);
            EXPECT(k == wrap_literal(d));
            const double dd = d + UW_TWOPI * (double)k;
            EXPECT(dd >= -UW_PI && dd <= UW_PI);
        }
        // the half-open ends
        EXPECT(wrap_count(pi_d) == 0 && wrap_count(-pi_d) == 1);
        EXPECT(wrap_count(std::nextafter(pi_d, 4.0)) == -1 && wrap_count(std::nextafter(-pi_d, 0.0)) == 0);
        EXPECT(wrap_count(pi_f) == -1 && wrap_count(-pi_f) == 1 && wrap_count(0.0) == 0);
        EXPECT(unwrap_value(1.5f, 0) == 1.5f && unwrap_value(1.5f, -2) == (float)(1.5 - 2.0 * UW_TWOPI));
    }

    // ---- the row of a padded index, every index of the frame: the direct tests' shapes and the native crop
    {
        const int shapes[][2] = {{64, 64}, {151, 203}, {921, 69}, {215, 300}, {254, 254}, {6000, 24}, {224, 224}, {1182, 1182}, {1623, 1623}};
        for (const auto &s : shapes) {
            const int h = s[0], w = s[1], W2 = w + 2;
            const long EN = padded_pixels(h, w);
            const uint32_t magic = padded_magic(h, w);
            EXPECT(magic != 0u);
            for (long idx = 0; idx < EN; idx++) EXPECT(padded_row((int)idx, magic, W2) == (int)(idx / W2));
        }
        // magic == 0 exactly where EN * W2 >= 2^32: square frames, 1625^3 < 2^32 <= 1626^3
        EXPECT(1625ull * 1625 * 1625 < 0x100000000ull && 1626ull * 1626 * 1626 >= 0x100000000ull);
        EXPECT(padded_magic(1623, 1623) != 0u && padded_magic(1624, 1624) == 0u);
        // and at one width: 1624 columns, 1628 | 1629 padded rows
        EXPECT(1628ull * 1624 * 1624 < 0x100000000ull && 1629ull * 1624 * 1624 >= 0x100000000ull);
        EXPECT(padded_magic(1626, 1622) != 0u && padded_magic(1627, 1622) == 0u);
        EXPECT(padded_row(1624 * 1000 + 7, 0u, 1624) == 1000);                 // without a magic: the division
        // every frame of the uint16 rank range has one (k_unwrap_flood_batch and k_unwrap_replay assume it): the widest, 1 x 21842
        EXPECT(unwrap_ranked_supported(1, 21842) && !unwrap_ranked_supported(1, 21843) && padded_magic(1, 21842) != 0u);
    }

    // ---- pad / unpad round trip and the distance test over a small frame, with and without a magic
    {
        const int h = 9, w = 13, W2 = w + 2;
        for (uint32_t magic : {padded_magic(h, w), 0u})
            for (int y = 0; y < h; y++)
                for (int x = 0; x < w; x++) {
                    const int idx = pad_index(y, x, W2);
                    EXPECT(idx == (y + 1) * W2 + x + 1 && idx < padded_pixels(h, w));
                    EXPECT(unpad_index(idx, magic, W2) == y * w + x);
                    for (int y1 = 0; y1 < h; y1++)
                        for (int x1 = 0; x1 < w; x1++)
                            EXPECT(within_two(idx, pad_index(y1, x1, W2), magic, W2) == (std::abs(y - y1) <= 2 && std::abs(x - x1) <= 2));
                }
    }

    // ---- the eight neighbour slots: the 3 x 3 block without its centre, lexicographic (dy, dx)
    {
        int n = 0;
        for (int dy = -1; dy <= 1; dy++)
            for (int dx = -1; dx <= 1; dx++) {
                if (dy == 0 && dx == 0) continue;
                int sy = 9, sx = 9;
                neighbour_slot(n, sy, sx);
                EXPECT(sy == dy && sx == dx && neighbour_offset(n, 302) == dy * 302 + dx);
                n++;
            }
        EXPECT(n == 8);
    }

    // ---- the rank plane: B frames at the stride the kernels index with stay inside the B * EN + 8 B elements the layout used to state
    {
        const int shapes[][2] = {{8, 8}, {64, 64}, {224, 224}, {253, 254}, {253, 255}, {512, 512}, {1182, 1182}, {8200, 8200}};
        for (const auto &s : shapes)
            for (long B : {1L, 3L, 8L, 64L}) {
                const long EN = padded_pixels(s[0], s[1]);
                EXPECT(code_stride(EN) >= EN && code_stride(EN) % 8 == 0 && B * code_stride(EN) <= B * EN + 8 * B);
            }
    }

    // ---- the tiers at their thresholds
    EXPECT(padded_pixels(921, 69) == 65533 && unwrap_tier_of(921, 69, false) == UWT_RANK16 && unwrap_tier_of(921, 69, true) == UWT_RANK16);
    EXPECT(padded_pixels(215, 300) == 65534 && unwrap_tier_of(215, 300, false) == UWT_BITMAP && unwrap_tier_of(215, 300, true) == UWT_GENERIC);
    EXPECT(padded_pixels(8189, 8191) == (1L << 26) - 1 && unwrap_tier_of(8189, 8191, false) == UWT_BITMAP);
    EXPECT(padded_pixels(8190, 8190) == (1L << 26) && unwrap_tier_of(8190, 8190, false) == UWT_GENERIC);

    std::printf("unwrap host check ok\n");
    return 0;
}
