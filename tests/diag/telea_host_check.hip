// Stand-alone host check of the rules the Telea inpaint kernels share through csrc/telea_common.hpp and that are plain arithmetic: the magic
// row division and where its exactness ends, the window of a hole box and its cell-to-pixel mapping, the window build's taps and
// classification against a plain dilation, the state switch over all 256 flag bytes, the disc enumeration, and the distance rule of the
// four-pop outside pass, for a run under the host sanitizers.  Nothing here launches a kernel or needs a device.  Build and run:
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -o telea_host_check tests/diag/telea_host_check.hip
//   ASAN_OPTIONS=detect_leaks=0 ./telea_host_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../vistaf-roboskin-vision-integrated-multimodal-sensor_amd/csrc/telea_common.hpp"

using namespace vf;

#define EXPECT(c)                                                                 \
    do {                                                                          \
        if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } \
    } while (0)

static uint32_t mulhi(uint32_t a, uint32_t b) { return (uint32_t)(((unsigned long long)a * b) >> 32); }

int main()
{
    std::mt19937 rng(12345);

    // ---- telea_magic_ww: cell / ww for the pitches the tiers use (LDS windows from 9 cells wide up to the widest that fits 14464 cells in 9
    // rows, padded planes of the big-cluster march), at both ends of the plane and either side of every multiple of the pitch
    {
        std::vector<int> pitches;
        for (int ww = 9; ww <= 1607; ww++) pitches.push_back(ww);
        for (int ww : {1190, 1631, 4104, 16383}) pitches.push_back(ww);
        for (int ww : pitches) {
            const uint32_t magic = telea_magic_ww(ww);
            const unsigned long long limit = 0x100000000ull / (unsigned)ww;          // cells with cell * ww < 2^32
            const uint32_t rows = (uint32_t)(limit / (unsigned)ww);
            EXPECT(rows >= 1);
            std::vector<uint32_t> rr;                                                   // the first and last rows, and rows in between
            for (uint32_t r = 0; r <= 48 && r <= rows; r++) { rr.push_back(r); rr.push_back(rows - r); }
            for (int k = 0; k < 64; k++) rr.push_back((uint32_t)(rng() % (rows + 1)));
            for (uint32_t r : rr)
                for (long long cell : {(long long)r * ww - 1, (long long)r * ww, (long long)r * ww + 1}) {
                    if (cell < 0 || (unsigned long long)cell >= limit) continue;
                    EXPECT(mulhi((uint32_t)cell, magic) == (uint32_t)cell / (uint32_t)ww);
                }
            EXPECT(mulhi((uint32_t)(limit - 1), magic) == (uint32_t)(limit - 1) / (uint32_t)ww);
        }
        // the plane-size test and the multiplier agree on where exactness ends: every cell of a 16383 x 16 plane splits exactly, and the
        // 16384 x 16 plane is refused although its multiplier would still be right -- the test is sufficient, never optimistic
        EXPECT(16383ull * 16383 * 16 < 0x100000000ull && 16384ull * 16384 * 16 >= 0x100000000ull);
        EXPECT(telea_magic_plane(16383, 16) == telea_magic_ww(16383) && telea_magic_plane(16383, 16) != 0u && telea_magic_plane(16384, 16) == 0u);
        for (uint32_t cell = 0; cell < 16383u * 16u; cell++) EXPECT(mulhi(cell, telea_magic_plane(16383, 16)) == cell / 16383u);
        // a pitch where the multiplier really fails just beyond the limit: ww = 3, cell = 2^32 - 1 is never formed, but 3 * cell >= 2^32 from
        // cell = 1431655766 on, and a wrong row shows up within a few thousand cells of the uint32 range's end
        bool wrong = false;
        for (uint32_t cell = 0xFFFFFFFFu; cell > 0xFFFFFFFFu - 10000u; cell--) wrong = wrong || mulhi(cell, telea_magic_ww(3)) != cell / 3u;
        EXPECT(wrong && telea_magic_plane(3, 477218589) == 0u && telea_magic_plane(3, 477218588) != 0u);
    }

    // ---- the window of a box: boxes touching each frame border; the mapping round-trips; every pixel within range + 1 of the box is inside
    {
        const int h = 23, w = 31;
        const int boxes[][4] = {{0, 0, 0, 0}, {30, 22, 30, 22}, {0, 5, 3, 9}, {27, 5, 30, 9}, {4, 0, 9, 2}, {4, 20, 9, 22}, {0, 0, 30, 22}, {10, 10, 12, 11}};
        for (int range = 1; range <= 7; range++)
            for (const auto &bx : boxes) {
                const int xmin = bx[0], ymin = bx[1], xmax = bx[2], ymax = bx[3], M = range + 1;
                const TeleaBoxWin bw = telea_window_of_box(xmin, ymin, xmax, ymax, range);
                EXPECT(bw.wh == ymax - ymin + 1 + 2 * M && bw.ww == xmax - xmin + 1 + 2 * M && bw.cells() == bw.wh * bw.ww);
                std::vector<int> seen((size_t)h * w, 0);
                int inside = 0;
                for (int r = 0; r < bw.wh; r++)
                    for (int cc = 0; cc < bw.ww; cc++) {
                        const int y = ymin - M + r, x = xmin - M + cc, li = r * bw.ww + cc;       // the pixel this cell stands for
                        size_t gp = 99;
                        const bool in = bw.locate(li, bw.cells(), r, cc, h, w, gp);
                        EXPECT(in == (y >= 0 && y < h && x >= 0 && x < w));
                        EXPECT(gp == (in ? (size_t)y * w + x : 0));
                        if (in) { EXPECT(bw.pixel(r, cc, w) == gp); seen[gp]++; inside++; }
                        size_t g2 = 99;
                        EXPECT(!bw.locate(bw.cells(), bw.cells(), r, cc, h, w, g2) && g2 == 0);    // a cell index past the window is never inside
                    }
                for (int y = 0; y < h; y++)
                    for (int x = 0; x < w; x++) {
                        const bool near = y >= ymin - M && y <= ymax + M && x >= xmin - M && x <= xmax + M;
                        EXPECT(seen[(size_t)y * w + x] == (near ? 1 : 0));
                    }
                EXPECT(inside > 0);
            }
    }

    // ---- the window build (row taps, column taps, 4-neighbour test, classification) on the unclipped window of small random masks, and the
    // prep kernels' per-pixel classification, against a plain dilation; ranges 1..7 lie on both sides of the unroll bound
    {
        EXPECT(TELEA_RING_U == 6);
        for (int range = 1; range <= 7; range++)
            for (int trial = 0; trial < 12; trial++) {
                const int h = 9 + (int)(rng() % 12), w = 9 + (int)(rng() % 14);
                std::vector<uint8_t> bad((size_t)h * w, 0);
                const int nh = 1 + (int)(rng() % 6);
                int xmin = w, ymin = h, xmax = -1, ymax = -1;
                for (int k = 0; k < nh; k++) {
                    const int y = (int)(rng() % h), x = (int)(rng() % w);
                    bad[(size_t)y * w + x] = (uint8_t)(1 + rng() % 255);
                    xmin = std::min(xmin, x); xmax = std::max(xmax, x); ymin = std::min(ymin, y); ymax = std::max(ymax, y);
                }
                if (trial == 0) { bad[0] = 1; xmin = ymin = 0; }                               // a hole in the frame's corner
                auto hole = [&](int y, int x) -> bool { return y >= 0 && y < h && x >= 0 && x < w && bad[(size_t)y * w + x] != 0; };
                auto want_kind = [&](int y, int x) -> int {                                     // of a pixel inside the image
                    if (hole(y, x)) return TC_NONE;
                    if (hole(y, x - 1) || hole(y, x + 1) || hole(y - 1, x) || hole(y + 1, x)) return TC_BAND;
                    for (int a = -range; a <= range; a++)
                        for (int c = -range; c <= range; c++)
                            if (hole(y + a, x + c)) return TC_RING;
                    return TC_NONE;
                };
                const TeleaBoxWin bw = telea_window_of_box(xmin, ymin, xmax, ymax, range);
                const int cells = bw.cells(), wh = bw.wh, ww = bw.ww;
                std::vector<uint8_t> f((size_t)cells);
                for (int li = 0; li < cells; li++) {
                    size_t gp;
                    const bool in = bw.locate(li, cells, li / ww, li % ww, h, w, gp);
                    f[li] = !in ? W_BORDER : bad[gp] ? W_HOLE : (uint8_t)0;
                }
                std::vector<uint8_t> row(f);
                for (int li = 0; li < cells; li++)
                    if (telea_ring_row_tap(f.data(), li, li / ww, li % ww, ww, range) & W_HOLE) row[li] |= W_ROW;
                for (int li = 0; li < cells; li++) {
                    const int r = li / ww, cc = li % ww, y = ymin - (range + 1) + r, x = xmin - (range + 1) + cc;
                    const int kind = telea_cell_kind(row[li], telea_nb4_tap(row.data(), li, r, cc, wh, ww), telea_ring_col_tap(row.data(), li, r, cc, wh, ww, range));
                    const bool in = y >= 0 && y < h && x >= 0 && x < w;
                    EXPECT(kind == (in ? want_kind(y, x) : (int)TC_NONE));
                    if (in && !hole(y, x)) {
                        auto hole1 = [&](int yy, int xx) -> bool { return hole(yy - 1, xx - 1); };       // the whole-frame kernel's coordinates: padded by one
                        EXPECT(telea_known_pixel_kind(hole, y, x, range) == kind && telea_known_pixel_kind(hole1, y + 1, x + 1, range) == kind);
                    }
                }
                // outside the window no pixel is band or ring: the window holds everything the outside pass touches
                for (int y = 0; y < h; y++)
                    for (int x = 0; x < w; x++)
                        if (y < ymin - range - 1 || y > ymax + range + 1 || x < xmin - range - 1 || x > xmax + range + 1) EXPECT(want_kind(y, x) == TC_NONE);
            }
    }

    // ---- the state switch, all 256 flag bytes
    for (int v = 0; v < 256; v++) {
        bool neg = false;
        const uint8_t m = telea_to_march_state((uint8_t)v, neg);
        EXPECT(neg == ((v & 3) == 3));                                                  // CHANGE: the outside pass ran here
        EXPECT((m & 3) == ((v & 0x40) ? 2 : 0));                                        // hole = INSIDE, everything else KNOWN
        EXPECT((m & 0xD0) == (v & 0xD0) && (m & 0x2C) == 0);                            // SEED, HOLE, BORDER kept; the scratch bit and bits 2-3 cleared
    }
    EXPECT(W_KNOWN == 0 && W_BAND == 1 && W_INSIDE == 2 && W_CHANGE == 3 && W_BORDER == 0x10 && W_ROW == 0x20 && W_HOLE == 0x40 && W_SEED == 0x80);

    // ---- the disc enumeration
    {
        const int want[5] = {0, 5, 13, 29, 49};
        for (int range = 1; range <= 4; range++) {
            std::vector<std::pair<int, int>> disc;                                      // row-major
            for (int dk = -range; dk <= range; dk++)
                for (int dl = -range; dl <= range; dl++)
                    if (dk * dk + dl * dl <= range * range) disc.push_back({dk, dl});
            EXPECT((int)disc.size() == want[range]);
            for (int lane = 0; lane < 64; lane++) {
                const TeleaDisc d = telea_disc(lane, range);
                EXPECT(d.ndisc == want[range] && d.nn == want[range] && !d.on[1]);
                EXPECT(d.on[0] == (lane < want[range]));
                if (d.on[0]) EXPECT(d.dk[0] == disc[lane].first && d.dl[0] == disc[lane].second);
            }
        }
        for (int range : {5, 6, 7, 12}) {
            const int side = 2 * range + 1;
            int nd = 0;
            for (int i = 0; i < side * side; i++) nd += (i / side - range) * (i / side - range) + (i % side - range) * (i % side - range) <= range * range;
            for (int lane = 0; lane < 64; lane++) {
                const TeleaDisc d = telea_disc(lane, range);
                EXPECT(d.ndisc == nd && nd > 64 && d.nn == side * side);
                for (int c2 = 0; c2 < 2; c2++) {
                    const int i = c2 * 64 + lane, dk = i / side - range, dl = i % side - range;
                    EXPECT(d.dk[c2] == dk && d.dl[c2] == dl && d.on[c2] == (i < side * side && dk * dk + dl * dl <= range * range));
                }
            }
        }
    }

    // ---- the prefix rule of the four-pop outside pass: the longest prefix whose members are pairwise at Manhattan distance >= 4; from cells
    // through the multiplier; 1 with the multiplier off
    for (int trial = 0; trial < 200000; trial++) {
        int r[4], c[4];
        const int spread = 2 + (int)(rng() % 9);
        for (int i = 0; i < 4; i++) { r[i] = (int)(rng() % spread); c[i] = (int)(rng() % spread); }
        const int n = 1 + (int)(rng() % 4);
        int m = 1;
        for (; m < n; m++) {
            bool clash = false;
            for (int i = 0; i < m; i++) clash = clash || std::abs(r[i] - r[m]) + std::abs(c[i] - c[m]) < 4;
            if (clash) break;
        }
        EXPECT(telea_prefix_by_distance(r, c, n) == m);
        const int ww = 16 + (int)(rng() % 4000), r0 = (int)(rng() % 1000);
        const int cells[4] = {(r0 + r[0]) * ww + c[0], (r0 + r[1]) * ww + c[1], (r0 + r[2]) * ww + c[2], (r0 + r[3]) * ww + c[3]};
        EXPECT(telea_outside_prefix(cells, n, ww, telea_magic_ww(ww)) == m && telea_outside_prefix(cells, n, ww, 0u) == 1);
    }

    std::printf("telea host check ok\n");
    return 0;
}
