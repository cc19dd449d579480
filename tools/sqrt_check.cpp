// sqrt_check.cpp -- host check of sgk_sqrt_cert (sigtk_amd/csrc/tstat_math.h) against sqrtf on every float bit pattern.
// The hardware's v_rsq_f32 is modelled as RN32((1 + eta) / sqrt(v)) with eta = 0, +-2^-23.3 (the largest error
// tools/rsq_check.hip measured on gfx950) and +-2^-22.3 (twice that).  For every model: no certified result may differ
// from sqrtf (exit status 1 otherwise); the certified share of the domain [2^-64, 2^41) is reported.
// Build: g++ -O2 -std=c++17 -ffp-contract=off -pthread -o tools/sqrt_check tools/sqrt_check.cpp
// Run:   tools/sqrt_check [stride]      (stride 1: all 2^32 patterns, about a minute on 8 cores; the CPU test uses 251)
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

static thread_local double g_eta = 0.0;
static inline float rsq_model(float v) { return (float)((1.0 + g_eta) / std::sqrt((double)v)); }
#define SGK_RSQ32(v) rsq_model(v)
#include "../sigtk_amd/csrc/tstat_math.h"

struct Tally {
    uint64_t certified = 0, in_domain = 0, mismatches = 0, certified_outside = 0;
    uint32_t first_bad = 0;
};

static void run(double eta, uint64_t lo, uint64_t hi, uint64_t stride, Tally *t) {
    g_eta = eta;
    for (uint64_t u = lo; u < hi; u += stride) {
        const uint32_t b = (uint32_t)u;
        float v;
        memcpy(&v, &b, 4);
        bool ok;
        const float s = sgk_sqrt_cert(v, ok);
        const bool dom = (b - SGK_SQRT_LO) < (SGK_SQRT_HI - SGK_SQRT_LO);
        t->in_domain += dom ? 1 : 0;
        if (!ok) continue;
        ++t->certified;
        if (!dom) ++t->certified_outside;
        const float r = sqrtf(v);
        if (memcmp(&s, &r, 4) != 0) {
            if (t->mismatches == 0) t->first_bad = b;
            ++t->mismatches;
        }
    }
}

int main(int argc, char **argv) {
    const uint64_t stride = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    if (stride == 0) return 2;
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt == 0 ? 4 : (nt > 16 ? 16 : nt);
    const double e1 = std::exp2(-23.3), e2 = std::exp2(-22.3);
    const double etas[5] = {0.0, e1, -e1, e2, -e2};
    uint64_t bad = 0;
    for (double eta : etas) {
        std::vector<Tally> tl(nt);
        std::vector<std::thread> th;
        const uint64_t span = (1ull << 32) / nt;
        for (unsigned k = 0; k < nt; ++k) {
            // every thread starts on a multiple of the stride, so that the union is the same set for any thread count
            const uint64_t a = k * span, b = k + 1 == nt ? (1ull << 32) : (k + 1) * span;
            const uint64_t a0 = (a + stride - 1) / stride * stride;
            th.emplace_back(run, eta, a0, b, stride, &tl[k]);
        }
        Tally s;
        for (unsigned k = 0; k < nt; ++k) {
            th[k].join();
            s.certified += tl[k].certified;
            s.in_domain += tl[k].in_domain;
            s.certified_outside += tl[k].certified_outside;
            if (tl[k].mismatches && !s.mismatches) s.first_bad = tl[k].first_bad;
            s.mismatches += tl[k].mismatches;
        }
        printf("rsq error %+.3e: %llu patterns in the domain, %llu certified (%.6f %%), %llu certified outside the domain, "
               "%llu mismatches with sqrtf", eta, (unsigned long long)s.in_domain, (unsigned long long)s.certified,
               s.in_domain ? 100.0 * (double)s.certified / (double)s.in_domain : 0.0, (unsigned long long)s.certified_outside,
               (unsigned long long)s.mismatches);
        if (s.mismatches) printf(" (first: 0x%08x)", s.first_bad);
        printf("\n");
        bad += s.mismatches + s.certified_outside;
    }
    printf("%s\n", bad ? "FAILED" : "ok: every certified result equals sqrtf");
    return bad ? 1 : 0;
}
