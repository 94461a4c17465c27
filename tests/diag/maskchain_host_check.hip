// Stand-alone host check of the pure rules of the fused mask chains (csrc/mask_bits.hpp): the bit accessor's index arithmetic against plain
// division and a byte plane, the plane sizes, cc_row_contacts read through the accessor against the byte plane, and mask_chain_fits at its
// limits, for a run under the host sanitizers.  Nothing here launches a kernel or needs a device.  Build and run:
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -o maskchain_host_check tests/diag/maskchain_host_check.hip
//   ASAN_OPTIONS=detect_leaks=0 ./maskchain_host_check
#include <cstdio>
#include <cstdlib>
#include <random>
#include <utility>
#include <vector>

#include "../../vistaf-roboskin-vision-integrated-multimodal-sensor_amd/csrc/host_util.hpp"
#include "../../vistaf-roboskin-vision-integrated-multimodal-sensor_amd/csrc/mask_bits.hpp"

using namespace vf;

#define EXPECT(c)                                                                 \
    do {                                                                          \
        if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } \
    } while (0)

int main()
{
    // ---- row_of: the multiply-high division, every pixel index of every width the uint16 forest can meet
    for (int w = 1; w <= 65535; w++) {
        const BitMask m(nullptr, w);
        EXPECT(m.W64 == (w + 63) / 64);
        // every p for small and for a spread of widths, the ends of every row otherwise
        if (w <= 300 || w % 997 == 0 || w >= 65500) {
            for (int p = 0; p <= 65535; p++) EXPECT(m.row_of(p) == p / w);
        } else {
            for (int y = 0; y * w <= 65535; y++) {
                EXPECT(m.row_of(y * w) == y);
                if (y * w + w - 1 <= 65535) EXPECT(m.row_of(y * w + w - 1) == y);
                if (y > 0) EXPECT(m.row_of(y * w - 1) == y - 1);
            }
            EXPECT(m.row_of(65535) == 65535 / w);
        }
    }

    // ---- the accessor against the byte plane it stands for, and cc_row_contacts through either
    std::mt19937 rng(7);
    const int shapes[][2] = {{1, 1}, {9, 40}, {64, 64}, {33, 65}, {96, 80}, {5, 129}, {224, 224}, {255, 257}, {1, 65535}, {65535, 1}, {3, 200}};
    for (const auto &s : shapes) {
        const int h = s[0], w = s[1], P = h * w, W64 = mb_w64(w);
        EXPECT(mb_plane_bytes(h, w) == (size_t)h * W64 * 8);
        EXPECT(mb_last_valid(w) == ((w % 64) ? (1ull << (w % 64)) - 1ull : ~0ull));
        std::vector<uint8_t> bytes(P);
        std::vector<unsigned long long> words((size_t)h * W64, 0ull);
        for (int p = 0; p < P; p++) {
            bytes[p] = (rng() % 100) < 45 ? (uint8_t)(1 + rng() % 255) : (uint8_t)0;
            if (bytes[p]) words[(size_t)(p / w) * W64 + (p % w) / 64] |= 1ull << ((p % w) % 64);
        }
        const BitMask m(words.data(), w);
        for (int p = 0; p < P; p++) {
            int bit;
            const int i = m.word_of(p, bit);
            EXPECT(i == (p / w) * W64 + (p % w) / 64 && bit == (p % w) % 64);
            EXPECT(m[p] == (bytes[p] != 0));
        }
        for (int p = 0; p < P; p++) {
            if (!bytes[p]) continue;
            const int y = p / w, x = p % w;
            std::vector<std::pair<int, int>> ua, ub;
            cc_row_contacts(bytes.data(), p, x, y, w, x > 0 && bytes[p - 1], [&](int a, int b) { ua.push_back({a, b}); });
            cc_row_contacts(m, p, x, y, w, x > 0 && m[p - 1], [&](int a, int b) { ub.push_back({a, b}); });
            EXPECT(ua == ub);
        }
    }

    // ---- mask_chain_fits
    const RowSpanSE e3 = ellipse_se(3), e7 = ellipse_se(7), e15 = ellipse_se(15), e33 = ellipse_se(33), e4 = ellipse_se(4);
    for (int chain : {MCH_BAD, MCH_RELIABLE, MCH_CONTACT}) {
        EXPECT(mask_chain_fits(chain, 224, 224, e7, 2, 6.f) && mask_chain_fits(chain, 9, 40, e3, 0));
        EXPECT(mask_chain_fits(chain, 64, 64, e15, 4, 1.f) && !mask_chain_fits(chain, 64, 64, e15, 5, 1.f) && !mask_chain_fits(chain, 64, 64, e15, -1));
        EXPECT(!mask_chain_fits(chain, 0, 64, e3, 1) && !mask_chain_fits(chain, 64, 0, e3, 1));
        EXPECT(mask_chain_fits(chain, 64, 64, e33, 1) && !mask_chain_fits(chain, 64, 64, e4, 1) && mask_chain_fits(chain, 64, 64, e4, 0));
        EXPECT(!mask_chain_fits(chain, 1182, 1182, e7, 2));
    }
    EXPECT(!mask_chain_fits(0, 64, 64, e3, 1) && !mask_chain_fits(3, 64, 64, e3, 1) && !mask_chain_fits(8, 64, 64, e3, 1));
    // the forest: 65535 pixels at most, forest + three planes within LDS_DYN_HEADROOM
    EXPECT(!mask_chain_fits(MCH_RELIABLE, 256, 256, e7, 2, 6.f) && mask_chain_fits(MCH_BAD, 256, 256, e7, 2) && mask_chain_fits(MCH_CONTACT, 256, 256, e7, 2));
    EXPECT(!mask_chain_fits(MCH_RELIABLE, 255, 257, e7, 2, 6.f) && mask_chain_lds(MCH_RELIABLE, 255, 257) == 131088 + 3 * 10200);
    EXPECT(mask_chain_fits(MCH_RELIABLE, 240, 240, e7, 2, 6.f) && mask_chain_lds(MCH_RELIABLE, 240, 240) == 115216 + 3 * 7680);
    EXPECT(mask_chain_lds(MCH_RELIABLE, 224, 224) == 100368 + 3 * 7168 && mask_chain_lds(MCH_BAD, 224, 224) == 2 * 7168 &&
           mask_chain_lds(MCH_CONTACT, 224, 224) == 3 * 7168);
    // the chamfer ball: margins up to 16 have one (33 rows), none beyond; margin <= 0 asks for none
    EXPECT(mask_chain_fits(MCH_RELIABLE, 64, 64, e7, 2, 16.f) && !mask_chain_fits(MCH_RELIABLE, 64, 64, e7, 2, 17.f) && mask_chain_fits(MCH_RELIABLE, 64, 64, e7, 2, 0.f));
    EXPECT(mask_chain_fits(MCH_BAD, 64, 64, e7, 2, 40.f));           // the margin concerns the reliable chain only
    // whatever fits never asks for more LDS than the headroom, and never for an element the word-shift step refuses
    for (int h = 1; h <= 1200; h += 7)
        for (int w = 1; w <= 1200; w += 5)
            for (int chain : {MCH_BAD, MCH_RELIABLE, MCH_CONTACT})
                if (mask_chain_fits(chain, h, w, e15, 2, 6.f)) {
                    EXPECT(mask_chain_lds(chain, h, w) <= (size_t)LDS_DYN_HEADROOM && morph_bits_ok(e15, h, w));
                    EXPECT(chain != MCH_RELIABLE || h * w <= 65535);
                }
    std::printf("maskchain_host_check ok\n");
    return 0;
}
