// Stand-alone host check of the two rules csrc/select.hpp's block_select2_each ends a level and a selection with, run with the host's own loops in
// place of the workgroup:
//   1. the finish by counting (sel_rank_vote): for candidate lists of every length 1 .. 1024, padded to whole waves with SEL_PAD as the kernel
//      pads them, the maximum of the votes equals the sorted list's entry at every rank -- random keys, lists heavy in duplicates, lists of one
//      key, lists whose keys reach up to the key below the pad;
//   2. the self-cleaning histogram as a host model: a host array stands in for SelShared::hist, a level counts into it and the bucket search,
//      walked thread by thread over the kernel's own index ranges (NBT = SEL_NB / NT buckets from NBT * tid, four at a time, for NT = 256, 512
//      and 1024), zeroes what it reads; over sequences of selections that end in every way a level can end (one key left, shift 0, few enough
//      candidates, plans that are done before a level starts) the array is all zeros after every level, and the rank found is
//      std::nth_element's.  This checks the index ranges and the level rules, not the device code: what guards the kernels against a dirty
//      histogram is tests/test_select_finish.py, four requests per launch and the chained launch.
// Nothing here launches a kernel or needs a device.  Build and run (the sanitizers are optional):
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -o select_finish_host_check tests/diag/select_finish_host_check.hip
//   ASAN_OPTIONS=detect_leaks=0 ./select_finish_host_check
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../vistaf-roboskin-vision-integrated-multimodal-sensor_amd/csrc/select.hpp"

using namespace vf;

#define EXPECT(c)                                                                 \
    do {                                                                          \
        if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } \
    } while (0)

// the kernel's finish on the host: list[0 .. m) padded to a multiple of 64, every entry of the padded list counts and votes
static int check_finish(std::vector<uint32_t> list)
{
    const uint32_t m = (uint32_t)list.size();
    std::vector<uint32_t> sorted = list;
    std::sort(sorted.begin(), sorted.end());
    while (list.size() % 64) list.push_back(SEL_PAD);
    std::vector<uint32_t> less(list.size());
    for (size_t t = 0; t < list.size(); t++) {
        uint32_t c = 0;
        for (size_t i = 0; i < list.size(); i++) c += list[i] < list[t];
        less[t] = c;
    }
    for (uint32_t want = 0; want < m; want++) {
        uint32_t a = 0, b = 0;
        for (size_t t = 0; t < list.size(); t++) {
            a = std::max(a, sel_rank_vote(list[t], less[t], want));
            b = std::max(b, sel_rank_vote(list[t], less[t], want + 1));
        }
        if (a != sorted[want]) { std::printf("m %u rank %u: got %08x expected %08x\n", m, want, a, sorted[want]); return 1; }
        if (want + 1 < m && b != sorted[want + 1]) { std::printf("m %u rank %u + 1: got %08x expected %08x\n", m, want, b, sorted[want + 1]); return 1; }
    }
    return 0;
}

// block_select2_each's level loop for rank k over `keys`, the histogram in `hist` (all zeros on entry and, checked here, after every level).
// Returns the key of rank k; how: 0 one key left, 1 shift 0, 2 candidates (finished by the rule above), counted in ends[]
static int select_host(const std::vector<uint32_t> &keys, uint32_t k, uint32_t kmin, uint32_t kmax, std::vector<uint32_t> &hist, uint32_t &got, int *ends, int NT)
{
    const auto clean = [&]() { return std::all_of(hist.begin(), hist.end(), [](uint32_t v) { return v == 0; }); };
    uint32_t lo = kmin, hi = kmax, below = 0;
    for (int level = 0;; level++) {
        EXPECT(level < 4);
        if (hi == lo) { got = lo; ends[0]++; EXPECT(clean()); return 0; }
        const int shift = sel_shift(lo, hi, SEL_BITS);
        for (uint32_t key : keys)
            if (key >= lo && key <= hi) hist[(key - lo) >> shift]++;
        // the search: thread by thread, SEL_NB / SEL_T buckets each, read and zeroed
        const uint32_t want = k - below;
        uint32_t run = 0, bsel = 0, before = 0, cnt = 0;
        bool found = false;
        const int NBT = SEL_NB / NT;
        for (int tid = 0; tid < NT; tid++) {
            uint32_t cb[32];                                         // NBT <= 32
            for (int j = 0; j < NBT / 4; j++)                        // the kernel's uint4 reads, then its uint4 stores
                for (int e = 0; e < 4; e++) cb[4 * j + e] = hist[NBT * tid + 4 * j + e];
            for (int j = 0; j < NBT / 4; j++)
                for (int e = 0; e < 4; e++) hist[NBT * tid + 4 * j + e] = 0;
            for (int j = 0; j < NBT; j++) {
                if (want >= run && want < run + cb[j]) { bsel = (uint32_t)(NBT * tid + j); before = run; cnt = cb[j]; found = true; }
                run += cb[j];
            }
        }
        EXPECT(found && clean());
        below += before;
        const SelSpan nx = sel_narrow(lo, hi, bsel, (uint32_t)shift);
        lo = nx.lo; hi = nx.hi;
        if (shift == 0) { got = lo; ends[1]++; return 0; }
        if (cnt <= (uint32_t)SEL_CAND) {
            std::vector<uint32_t> cand;
            for (uint32_t key : keys)
                if (key >= lo && key <= hi) cand.push_back(key);
            EXPECT(cand.size() == cnt);
            const uint32_t m = cnt, want2 = k - below;
            while (cand.size() % 64) cand.push_back(SEL_PAD);
            uint32_t a = 0;
            for (uint32_t x : cand) {
                uint32_t less = 0;
                for (uint32_t y : cand) less += y < x;
                a = std::max(a, sel_rank_vote(x, less, want2));
            }
            EXPECT(want2 < m);
            got = a; ends[2]++;
            return 0;
        }
    }
}

int main()
{
    std::mt19937 rng(20240917u);
    // ---- 1. the finish, every length, every rank
    for (uint32_t m = 1; m <= (uint32_t)SEL_CAND; m++) {
        const int kind = (int)(m % 5);
        std::vector<uint32_t> v(m);
        const uint32_t base = rng();
        for (uint32_t i = 0; i < m; i++) {
            switch (kind) {
            case 0: v[i] = rng(); break;                                           // spread over all keys
            case 1: v[i] = base / 2 + rng() % 7u; break;                           // heavy in duplicates
            case 2: v[i] = base; break;                                            // one key
            case 3: v[i] = 0xFFFFFFFEu - rng() % (m < 4 ? 1u : m / 4u); break;     // ends just below the padding key, duplicates
            default: v[i] = (rng() & 1u) ? f2key(0.0f) : f2key(-0.0f); break;      // the two zeros: neighbouring keys
            }
            if (v[i] == SEL_PAD) v[i]--;
        }
        if (check_finish(v)) return 1;
    }
    EXPECT(f2key(-0.0f) + 1u == f2key(0.0f));
    // ---- 2. the self-cleaning histogram over sequences of selections
    std::vector<uint32_t> hist(SEL_NB, 0u);
    int ends[3] = {0, 0, 0}, skipped = 0;
    for (int seq = 0; seq < 60; seq++) {
        const uint32_t n = seq % 7 == 0 ? (uint32_t)(seq % 3) : 1u + rng() % 6000u;       // 0, 1, 2 elements among them
        std::vector<uint32_t> keys(n);
        const int kind = seq % 6;
        const uint32_t base = rng();
        for (auto &x : keys) {
            x = kind == 0 ? rng() : kind == 1 ? base : kind == 2 ? base / 2 + rng() % 3u : kind == 3 ? (base & 0xFFF00000u) + rng() % 40000u
                : kind == 4 ? f2key((float)(int)(rng() % 2001u - 1000u) * 1e-3f) : (rng() % 4u ? base / 2 : rng());
            if (x == SEL_PAD) x--;
        }
        const uint32_t kmin = n ? *std::min_element(keys.begin(), keys.end()) : 0u, kmax = n ? *std::max_element(keys.begin(), keys.end()) : 0u;
        const float reqs[] = {-1.f, 0.08f, 0.5f, 0.92f, 1.0f};
        for (float q : reqs) {
            const SelPlan p = sel_plan(n, q, kmin, kmax);
            if (p.done) { skipped++; EXPECT(std::all_of(hist.begin(), hist.end(), [](uint32_t v) { return v == 0; })); continue; }
            uint32_t got = 0;
            if (select_host(keys, p.k, kmin, kmax, hist, got, ends, 256 << (seq % 3))) return 1;
            std::vector<uint32_t> s = keys;
            std::nth_element(s.begin(), s.begin() + p.k, s.end());
            EXPECT(got == s[p.k]);
        }
    }
    EXPECT(ends[0] > 0 && ends[1] > 0 && ends[2] > 0 && skipped > 0);
    std::printf("select finish host check: ok (ends: one key %d, shift 0 %d, candidates %d; plans done before a level %d)\n", ends[0], ends[1], ends[2], skipped);
    return 0;
}
