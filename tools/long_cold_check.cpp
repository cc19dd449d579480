// long_cold_check.cpp -- host check of the lazy long detector's bound in its leading-edge form (sigtk_amd/csrc/
// tstat_math.h: sgk_lside_halves + sgk_long_cold; event_detect.h: LazyPass<.., LEAD>): the long window's estimates are
// formed from the f32 sums of its two halves.  Modelled on check #7 of oracle/verify_math.cpp, which covers the form
// that converts the long window's own f64 sums.
//   For W2 = 6 and 14: pairs of adjacent long windows (2 * W2 floats), sums formed exactly, estimates formed the NEW
//   way with tstat_math.h's own functions.  A VIOLATION is a pair that sgk_long_cold calls cold although
//   sgk_tstat_ref<W2> > 9 (exit status 1).  Also reported: the share of pairs called hot although the reference is <= 8
//   (what the bound's slack costs), next to the same share for the f64-sum form (sgk_lside).
//   Kinds of windows (k mod 8):
//     0 same sign, pA-like (level, jump between the windows, noise)      4 halves of every window of opposite sign:
//     1 ... with window B shifted so that the statistic lands near 9       m' ~ 0, |S1| + |S2| large; odd cases steered
//     2 mixed sign: a level near zero with noise across it               5 constant, or constant with one step
//     3 ... steered near 9                                               6 piecewise constant + noise, one step, steered
//                                                                        7 pA-like at both ends of the guard's range
// Build: g++ -O2 -std=c++17 -ffp-contract=off -pthread -o tools/long_cold_check tools/long_cold_check.cpp
// Run:   tools/long_cold_check [cases per window]    (default 10^9: a few minutes on 16 cores; the CPU test uses 4*10^6)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../sigtk_amd/csrc/tstat_math.h"

static inline uint64_t rng_next(uint64_t &s) {
    s += 0x9E3779B97F4A7C15ULL;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

constexpr int NKIND = 8;
constexpr int NSTREAM = 64;  // the case set does not depend on the thread count
struct Tally {
    uint64_t cases[NKIND] = {}, bad[NKIND] = {}, low[NKIND] = {}, fh_new[NKIND] = {}, fh_old[NKIND] = {}, near9[NKIND] = {};
    float first_bad_ref = 0.0f;
};

// 2 * W samples: window A = x[0 .. W), window B = x[W .. 2W)
template <int W>
static inline void make_samples(uint64_t &s, uint64_t k, float (&x)[2 * W]) {
    constexpr int H = W / 2;
    const float unit = 1402.882324f / 8192.0f;
    const uint64_t r = rng_next(s);
    const int kind = (int)(k % NKIND);
    const int jump = (int)((r >> 20) % 200) - 100, noise = 1 + (int)((r >> 40) % 12);
    const float off = (float)((r >> 52) % 20) + (((r >> 57) & 1) ? 0.25f : 0.0f);
    int base = 200 + (int)(r % 600);
    float scale = 1.0f;
    int wide = noise;
    const int j0 = 1 + (int)((r >> 30) % (uint64_t)(2 * W - 1));  // a step's position
    if (kind == 2 || kind == 3) { base = (int)(r % 121) - 60; wide = 1 + (int)((r >> 40) % 100); }
    if (kind == 4) base = 1 + (int)(r % 600);
    if (kind == 7) scale = ((r >> 58) & 1) ? ldexpf(1.0f, 12 - (int)((r >> 59) % 3)) : ldexpf(1.0f, -25 + (int)((r >> 59) % 3));
    for (int j = 0; j < 2 * W; ++j) {
        const uint64_t q = rng_next(s);
        const int nz = (int)(q % (uint64_t)(2 * wide + 1)) - wide;
        float v;
        switch (kind) {
            case 2: case 3: v = (float)(base + (j >= W ? jump : 0) + nz) - off; break;             // crosses zero
            case 4: v = ((j % W) < H ? 1.0f : -1.0f) * ((float)(base + nz) + off); break;          // +level | -level
            case 5: v = (float)(base + (((r >> 29) & 1) && j >= j0 ? jump : 0)) + off; break;      // constant (+ step)
            case 6: v = (float)(base + (j >= j0 ? jump : 0) + (nz % 3)) + off; break;              // step anywhere
            default: v = (float)(base + (j >= W ? jump : 0) + nz) + off;
        }
        x[j] = (v * unit) * scale;
    }
    const bool steer = kind == 1 || kind == 3 || kind == 6 || (kind == 4 && ((k / NKIND) & 1));
    if (steer) {
        // shift window B so that the statistic lands near 9: a shift moves the mean, not the variance
        double ma = 0, mb = 0, va = 0, vb = 0;
        for (int j = 0; j < W; ++j) { ma += x[j]; mb += x[W + j]; }
        ma /= W; mb /= W;
        for (int j = 0; j < W; ++j) { va += (x[j] - ma) * (x[j] - ma); vb += (x[W + j] - mb) * (x[W + j] - mb); }
        const double cv = (va + vb) / W;
        if (cv > 0.0) {
            const double target = 9.0 * (1.0 + ((double)(int64_t)(rng_next(s) % 2001) - 1000.0) * 1e-5);
            const double want = target * sqrt(cv / W) * ((r >> 28) & 1 ? 1.0 : -1.0);
            const float dq = (float)(ma + want - mb);
            for (int j = 0; j < W; ++j) x[W + j] = x[W + j] + dq;
        }
    }
}

template <int W>
static void run(uint64_t count, int t_lo, int t_hi, Tally *tl) {
    constexpr int H = W / 2;
    for (int t = t_lo; t < t_hi; ++t) {
        uint64_t s = 0x51ED27ULL * (uint64_t)(t + 13) + W;
        for (uint64_t k = 0; k < count / NSTREAM; ++k) {
            float x[2 * W];
            make_samples<W>(s, k, x);
            // exact sums of the four halves (doubles of at most 14 floats inside the guard's range)
            double S[4] = {0, 0, 0, 0}, Sq[4] = {0, 0, 0, 0};
            for (int j = 0; j < 2 * W; ++j) {
                const int h = j / H;
                S[h] += (double)x[j];
                Sq[h] += (double)(x[j] * x[j]);
            }
            const double A = S[0] + S[1], A2 = Sq[0] + Sq[1], B = S[2] + S[3], B2 = Sq[2] + Sq[3];
            const float ref = sgk_tstat_ref<W>(A, A2, B, B2);
            const SgkLSide la = sgk_lside_halves<W>((float)S[0], (float)Sq[0], (float)S[1], (float)Sq[1]);
            const SgkLSide lb = sgk_lside_halves<W>((float)S[2], (float)Sq[2], (float)S[3], (float)Sq[3]);
            const bool cold = sgk_long_cold<W>(la, lb);
            const bool cold_old = sgk_long_cold<W>(sgk_lside<W>(A, A2), sgk_lside<W>(B, B2));
            const int kind = (int)(k % NKIND);
            tl->cases[kind]++;
            if (ref > 8.5f && ref < 9.5f) tl->near9[kind]++;
            if (cold && !(ref <= 9.0f)) {
                if (!tl->bad[kind]) tl->first_bad_ref = ref;
                tl->bad[kind]++;
            }
            if (ref <= 8.0f) {
                tl->low[kind]++;
                if (!cold) tl->fh_new[kind]++;
                if (!cold_old) tl->fh_old[kind]++;
            }
        }
    }
}

template <int W>
static uint64_t check(uint64_t count, unsigned nt) {
    std::vector<Tally> tl(nt);
    std::vector<std::thread> th;
    for (unsigned k = 0; k < nt; ++k) th.emplace_back(run<W>, count, (int)(k * NSTREAM / nt), (int)((k + 1) * NSTREAM / nt), &tl[k]);
    Tally s;
    for (unsigned k = 0; k < nt; ++k) {
        th[k].join();
        for (int j = 0; j < NKIND; ++j) {
            s.cases[j] += tl[k].cases[j]; s.bad[j] += tl[k].bad[j]; s.low[j] += tl[k].low[j];
            s.fh_new[j] += tl[k].fh_new[j]; s.fh_old[j] += tl[k].fh_old[j]; s.near9[j] += tl[k].near9[j];
        }
        if (tl[k].first_bad_ref != 0.0f) s.first_bad_ref = tl[k].first_bad_ref;
    }
    uint64_t cases = 0, bad = 0, low = 0, fn = 0, fo = 0;
    for (int j = 0; j < NKIND; ++j) {
        printf("  W2 = %2d kind %d: %11llu cases, %10llu with the reference in (8.5, 9.5), %llu violations, hot although "
               "reference <= 8: %.6f %% (f64-sum form: %.6f %%)\n", W, j, (unsigned long long)s.cases[j],
               (unsigned long long)s.near9[j], (unsigned long long)s.bad[j],
               100.0 * (double)s.fh_new[j] / (double)(s.low[j] ? s.low[j] : 1),
               100.0 * (double)s.fh_old[j] / (double)(s.low[j] ? s.low[j] : 1));
        cases += s.cases[j]; bad += s.bad[j]; low += s.low[j]; fn += s.fh_new[j]; fo += s.fh_old[j];
    }
    printf("W2 = %d: %llu cases, %llu violations, hot although reference <= 8: %.6f %% (f64-sum form: %.6f %%)", W,
           (unsigned long long)cases, (unsigned long long)bad, 100.0 * (double)fn / (double)(low ? low : 1),
           100.0 * (double)fo / (double)(low ? low : 1));
    if (bad) printf(" (a violating reference value: %.9g)", s.first_bad_ref);
    printf("\n");
    return bad;
}

int main(int argc, char **argv) {
    const uint64_t count = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1000000000ull;
    if (count < NSTREAM) return 2;
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt == 0 ? 4 : (nt > 16 ? 16 : nt);
    uint64_t bad = 0;
    bad += check<6>(count, nt);
    bad += check<14>(count, nt);
    printf("%s\n", bad ? "FAILED" : "ok: no pair is called cold with a reference statistic above 9");
    return bad ? 1 : 0;
}
