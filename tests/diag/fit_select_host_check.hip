// Stand-alone host check of the rules the selection and fit kernels share through csrc/select.hpp and csrc/fit_rules.hpp and that are plain
// arithmetic: the plan and result of a request against NumPy's linear method written out in float32, the level rules as a host loop against
// std::nth_element, the monomial index and the assembled normal equations, the key ranges of the two medians, the normalised coordinate,
// and the two dispatch functions at their boundaries, for a run under the host sanitizers.  Nothing here launches a kernel or needs a
// device.  Build and run:
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -o fit_select_host_check tests/diag/fit_select_host_check.hip
//   ASAN_OPTIONS=detect_leaks=0 ./fit_select_host_check
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../vistaf-roboskin-vision-integrated-multimodal-sensor_amd/csrc/k_select.hip"
#include "../../vistaf-roboskin-vision-integrated-multimodal-sensor_amd/csrc/k_fit.hip"
#include "../../vistaf-roboskin-vision-integrated-multimodal-sensor_amd/csrc/k_big.hip"

using namespace vf;

#define EXPECT(c)                                                                 \
    do {                                                                          \
        if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } \
    } while (0)

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
// equal bits; two zeros count as equal (a float sort leaves the order of -0.0 and 0.0 open, the key order puts -0.0 first)
static bool same(float a, float b) { return bits(a) == bits(b) || (a == 0.f && b == 0.f); }

// np.percentile(s, method='linear') of the sorted float32 array s, numpy/lib/_function_base_impl.py (_quantile, _get_indexes, _lerp), float32
static float np_percentile_sorted(const std::vector<float> &s, float q)
{
    const int n = (int)s.size();
    const float vi = (float)(n - 1) * q;
    float prev = std::floor(vi);
    const float gamma = vi - prev;
    int p = (int)prev, nx = p + 1;
    if (vi >= (float)(n - 1)) p = nx = n - 1;          // indexes above the bounds: the last element twice
    if (p < 0) p = nx = 0;
    nx = std::min(nx, n - 1);
    const float a = s[p], b = s[nx], d = b - a;
    float r = a + d * gamma;
    if (gamma >= 0.5f) r = b - d * (1.0f - gamma);
    return r;
}
static float np_median_sorted(const std::vector<float> &s)
{
    const size_t n = s.size();
    return (n & 1) ? s[n / 2] : (s[n / 2 - 1] + s[n / 2]) / 2.0f;
}

static int check_plan(std::vector<float> v)
{
    std::vector<uint32_t> k(v.size());
    for (size_t i = 0; i < v.size(); i++) k[i] = f2key(v[i]);
    std::sort(k.begin(), k.end());
    for (size_t i = 0; i < v.size(); i++) { v[i] = key2f(k[i]); EXPECT(f2key(v[i]) == k[i]); }
    const uint32_t n = (uint32_t)v.size();
    const float pct[] = {0.f, 8.f, 25.f, 50.f, 92.f, 99.7f, 99.9f, 100.f, -100.f};          // the last one: the median request (q < 0)
    for (float pc : pct) {
        const float q = pc / 100.0f;
        const SelPlan p = sel_plan(n, q, k.front(), k.back());
        float got = p.result;
        if (!p.done) { EXPECT(p.k + 1 < n); got = sel_result(p, k[p.k], k[p.k + 1]); }
        const float exp = q < 0.f ? np_median_sorted(v) : np_percentile_sorted(v, q);
        if (!same(got, exp)) { std::printf("n %u q %g: got %08x expected %08x\n", n, q, bits(got), bits(exp)); return 1; }
    }
    return 0;
}

// the refinement of select.hpp as a host loop over `keys` for rank k, BITS digits per level; chain: the chain's next-width rule
static int check_levels(const std::vector<uint32_t> &keys, int BITS, bool chain)
{
    std::vector<uint32_t> sorted = keys;
    std::sort(sorted.begin(), sorted.end());
    const uint32_t n = (uint32_t)keys.size();
    std::vector<uint32_t> hist((size_t)1 << BITS);
    for (uint32_t k = 0; k < n; k++) {
        std::vector<uint32_t> nth = keys;
        std::nth_element(nth.begin(), nth.begin() + k, nth.end());
        const uint32_t want_key = nth[k];
        EXPECT(want_key == sorted[k]);
        uint32_t lo = sorted.front(), hi = sorted.back(), below = 0;
        uint32_t shift = (uint32_t)sel_shift(lo, hi, BITS);
        int levels = 0;
        for (;;) {
            if (!chain && hi == lo) break;                               // block_select2_each stops at a range of one key
            std::fill(hist.begin(), hist.end(), 0u);
            for (uint32_t key : keys)
                if (key >= lo && key <= hi) { EXPECT(((key - lo) >> shift) < hist.size()); hist[(key - lo) >> shift]++; }
            uint32_t bucket = 0, run = 0;
            while (run + hist[bucket] <= k - below) { run += hist[bucket]; bucket++; EXPECT(bucket < hist.size()); }
            below += run;
            const SelSpan s = sel_narrow(lo, hi, bucket, shift);
            EXPECT(s.lo >= lo && s.hi <= hi && s.lo <= s.hi);
            EXPECT(s.lo <= want_key && want_key <= s.hi);                // the narrowed range contains the wanted rank
            lo = s.lo; hi = s.hi;
            levels++;
            if (shift == 0) break;
            shift = chain ? sel_shift_chain_next(shift, BITS) : (uint32_t)sel_shift(lo, hi, BITS);
        }
        EXPECT(lo == want_key && hi == lo);                              // ends at a single key
        EXPECT(levels <= 3);
        // the next order statistic
        uint32_t cnt_le = 0, mg32 = 0xFFFFFFFFu;
        unsigned long long mg64 = ~0ull;
        for (uint32_t key : keys) { cnt_le += key <= lo; if (key > lo && key < mg32) mg32 = key; if (key > lo && key < mg64) mg64 = key; }
        const uint32_t next = k + 1 < n ? sorted[k + 1] : sorted[k];     // nothing above the largest key: a again
        EXPECT(sel_next(k, cnt_le, mg32, lo) == next);
        EXPECT(sel_next(k, cnt_le, mg64, lo) == next);
    }
    return 0;
}

template <int NC, int DEG>
static int check_assemble(std::mt19937 &rng)
{
    constexpr int NM = (DEG + 1) * (DEG + 2) / 2;
    std::uniform_real_distribution<double> U(0.1, 1.0), Z(-3.0, 3.0);
    double S[NM + 6] = {}, D[6][6] = {}, dr[6] = {};
    for (int y = 0; y < 5; y++)
        for (int x = 0; x < 7; x++) {
            const double xn = fit_coord(x, fit_centre(7)), yn = fit_coord(y, fit_centre(5)), w2 = U(rng), z = Z(rng);
            const double phi[6] = {xn, yn, 1.0, xn * xn, xn * yn, yn * yn};
            for (int b = 0; b <= DEG; b++)
                for (int a = 0; a + b <= DEG; a++) S[fit_mono(a, b, DEG)] += w2 * std::pow(xn, a) * std::pow(yn, b);
            for (int i = 0; i < NC; i++) {
                S[NM + i] += w2 * z * phi[i];
                dr[i] += w2 * z * phi[i];
                for (int j = 0; j < NC; j++) D[i][j] += w2 * phi[i] * phi[j];
            }
        }
    double A[6][6], rhs[6];
    fit_assemble<NC, DEG>(S, A, rhs);
    for (int i = 0; i < 6; i++) {
        for (int j = 0; j < 6; j++) {
            EXPECT(A[i][j] == A[j][i]);
            EXPECT(std::fabs(A[i][j] - D[i][j]) <= 1e-12 * std::max(1.0, std::fabs(D[i][j])));
        }
        EXPECT(rhs[i] == dr[i]);
    }
    return 0;
}

int main()
{
    std::mt19937 rng(2025);

    // ---- sel_plan + sel_result
    {
        const SelPlan p0 = sel_plan(0, 0.5f, 0xFFFFFFFFu, 0), m0 = sel_plan(0, -1.f, 0xFFFFFFFFu, 0);
        EXPECT(p0.done && m0.done && bits(p0.result) == 0x7fc00000u && bits(m0.result) == 0x7fc00000u);
        std::normal_distribution<float> N(0.f, 3.f);
        for (int n : {1, 2, 3, 4, 5, 100, 101}) {
            std::vector<float> plain(n), dup(n), zeros(n);
            for (int i = 0; i < n; i++) {
                plain[i] = N(rng);
                dup[i] = (float)((int)(rng() % 5) - 2) * 0.75f;                                  // five values, many copies
                zeros[i] = (rng() & 1) ? -0.0f : ((rng() & 1) ? 0.0f : (float)((int)(rng() % 3) - 1) * 1e-3f);
            }
            if (check_plan(plain) || check_plan(dup) || check_plan(zeros)) return 1;
            if (check_plan(std::vector<float>(n, -0.0f)) || check_plan(std::vector<float>(n, 1.25f))) return 1;
        }
        if (check_plan({-2.5f, 7.0f})) return 1;
    }

    // ---- level rules: BITS of select.hpp (13) and of the chain (11), either next-width rule
    {
        std::vector<std::vector<uint32_t>> sets;
        sets.push_back(std::vector<uint32_t>(5, 0x9ABCDEF0u));                                    // one value
        sets.push_back({7u, 7u, 0xC0000000u, 7u, 0xC0000000u});                                   // two distinct values
        sets.push_back({0u, 0xFFFFFFFEu, 0u, 0xFFFFFFFEu, 0xFFFFFFFEu});                          // the whole key span: the clipped last bucket
        sets.push_back({5u, 0xFFFFFFFEu, 6u, 0xFFF80005u, 0xFFFFFFFEu});                          // ... and the bucket that wraps past 2^32
        {
            std::vector<uint32_t> s;                                                              // a tight cluster plus far outliers
            for (int i = 0; i < 1500; i++) s.push_back(0xBF800000u + rng() % 300);
            for (uint32_t o : {1u, 2u, 0x10000000u, 0xF0000000u, 0xFFFFFFFEu}) s.push_back(o);
            sets.push_back(s);
        }
        {
            std::vector<uint32_t> s(2000);                                                        // the full 32-bit span
            for (auto &k : s) k = (uint32_t)rng() % 0xFFFFFFFFu;
            s[0] = 0; s[1] = 0xFFFFFFFEu; s[2] = s[3];
            sets.push_back(s);
        }
        for (const auto &s : sets)
            for (int BITS : {13, 11})
                for (bool chain : {false, true})
                    if (check_levels(s, BITS, chain)) return 1;
        EXPECT(sel_shift(0, 0, 13) == 0 && sel_shift(0, 0xFFFFFFFEu, 13) == 19 && sel_shift(0, 0xFFFFFFFEu, 11) == 21 && sel_shift(8, 8 + 8191, 13) == 0);
        EXPECT(sel_shift_chain_next(21, 11) == 10 && sel_shift_chain_next(10, 11) == 0);
    }

    // ---- monomial index against the tables it replaced
    {
        const int t4[5] = {0, 5, 9, 12, 14}, t2[3] = {0, 3, 5};
        for (int b = 0; b <= 4; b++)
            for (int a = 0; a + b <= 4; a++) EXPECT(fit_mono(a, b, 4) == t4[b] + a);
        for (int b = 0; b <= 2; b++)
            for (int a = 0; a + b <= 2; a++) EXPECT(fit_mono(a, b, 2) == t2[b] + a);
    }

    // ---- assembled normal equations against direct float64 sums of basis products
    if (check_assemble<6, 4>(rng) || check_assemble<3, 2>(rng) || check_assemble<3, 4>(rng)) return 1;

    // ---- key ranges of the two medians; csig
    for (int rep = 0; rep < 20; rep++) {
        std::uniform_real_distribution<float> C(-2.f, 2.f), Z(-5.f, 5.f);
        float coef[6];
        for (float &c : coef) c = C(rng);
        const int h = 9, w = 11;
        std::vector<float> z(h * w), r;
        for (float &v : z) v = Z(rng);
        const float zmin = *std::min_element(z.begin(), z.end()), zmax = *std::max_element(z.begin(), z.end());
        const FitKeys kr = fit_resid_range(coef, zmin, zmax);
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                const float xn = fit_coord(x, fit_centre(w)), yn = fit_coord(y, fit_centre(h)), zz = z[y * w + x];
                // eval_poly2d's order, and the generic kernel's chain
                const float chain = std::fma(coef[5], yn * yn, std::fma(coef[4], xn * yn, std::fma(coef[3], xn * xn, std::fma(coef[1], yn, coef[0] * xn) + coef[2])));
                for (float rr : {zz - fit_eval(coef, 2, xn, yn), zz - chain}) {
                    EXPECT(f2key(rr) >= kr.kmin && f2key(rr) <= kr.kmax);
                    r.push_back(rr);
                }
            }
        std::vector<float> sr = r;
        std::sort(sr.begin(), sr.end());
        const float med = np_median_sorted(sr);
        const FitKeys ka = fit_mad_range(kr, med);
        EXPECT(ka.kmin == f2key(0.f));
        for (float rr : r) { const float a = std::fabs(rr - med); EXPECT(f2key(a) >= ka.kmin && f2key(a) <= ka.kmax); }
        EXPECT(fit_csig(4.685f, 0.25f) == 4.685f * (1.4826f * (0.25f + 1e-6f)));
    }
    EXPECT(fit_gate(200, 0, 200, 0) && !fit_gate(199, 999, 200, 0) && !fit_gate(400, 499, 200, 500) && fit_gate(400, 500, 200, 500));

    // ---- normalised coordinate: exactly -1 and 1 at the ends; one pixel gives NaN (today's behaviour, see the (1, 150) degenerate test)
    for (int n : {2, 3, 224, 1182}) EXPECT(fit_coord(0, fit_centre(n)) == -1.0f && fit_coord(n - 1, fit_centre(n)) == 1.0f);
    EXPECT(std::isnan(fit_coord(0, fit_centre(1))));
    EXPECT(fit_coord(1, fit_centre(3)) == 0.0f);

    // ---- polyfit_variant (the values the function gave before the rules moved)
    {
        const struct { int h, w, v; } ladder[] = {{128, 128, FITV_COL16}, {160, 160, FITV_COL32}, {140, 300, FITV_COL48}, {165, 300, FITV_COL56},
                                                  {190, 300, FITV_COL64}, {151, 203, FITV_COL48_G4}, {224, 224, FITV_COL56_G4},
                                                  {256, 256, FITV_COL64_G4}, {320, 320, FITV_GENERIC}, {512, 512, FITV_BIG},
                                                  {1, 150, FITV_COL16}, {150, 1, FITV_COL16}};
        for (const auto &l : ladder) EXPECT(polyfit_variant(3, l.h, l.w, true, nullptr, nullptr) == l.v);
        int cp = 0, gr = 0;
        EXPECT(polyfit_variant(256, 224, 224, false, &cp, &gr) == FITV_COL56_G4 && cp == 256 && gr == 4);
        EXPECT(polyfit_variant(3, 1, 150, false, &cp, &gr) == FITV_COL16 && cp == 192 && gr == 1);
        EXPECT(polyfit_variant(3, 150, 1, false, &cp, &gr) == FITV_COL16 && cp == 64 && gr == 16);
        EXPECT(polyfit_variant(1, 1024, 2048, false, nullptr, nullptr) == FITV_GENERIC_DIV);
        EXPECT(polyfit_variant(3, 512, 512, false, nullptr, nullptr) == FITV_GENERIC);
        EXPECT(polyfit_variant(192, 512, 512, true, nullptr, nullptr) == FITV_BIG && polyfit_variant(193, 512, 512, true, nullptr, nullptr) == FITV_GENERIC);
    }

    // ---- select_variant
    {
        const struct { int P, v; } edge[] = {{16384, SELV_RES16}, {16385, SELV_RES32}, {32768, SELV_RES32}, {32769, SELV_RES49}, {50176, SELV_RES49},
                                             {50177, SELV_RES64}, {65536, SELV_RES64}, {65537, SELV_STREAM}, {262143, SELV_STREAM}};
        for (const auto &e : edge) {
            EXPECT(select_variant(3, e.P, 3, true, true) == e.v && select_variant(3, e.P, 3, false, true) == e.v);
            EXPECT(select_variant(3, e.P, 3, true, false) == SELV_STREAM);
        }
        EXPECT(select_variant(3, 262144, 4, true, true) == SELV_BIG && select_variant(3, 262144, 5, true, true) == SELV_STREAM);
        EXPECT(select_variant(3, 262144, 4, false, true) == SELV_STREAM && select_variant(193, 262144, 4, true, true) == SELV_STREAM);
    }

    std::printf("fit_select_host_check ok\n");
    return 0;
}
