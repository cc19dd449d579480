/* sdtw_c.c -- the definition of sgk_sdtw_f32 (include/sigtk_gpu.h) restated in plain C, one thread, two rows of D and S:
 * context for profiles/sdtw.md, not product code.
 *     gcc -O2 -ffp-contract=off -o tools/sdtw_c tools/sdtw_c.c
 *     tools/sdtw_c [n_queries] [query_len] [n_targets] [target_len]      (default 20 250 2 30000)
 * prints one JSON line: the shape, the milliseconds of all pairs, cells per second and a checksum of the records. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <math.h>
#include <time.h>

typedef struct { float score; int32_t end, start; } rec_t;

static rec_t sdtw(const float *q, int m, const float *t, int n, float *D, int32_t *S) {
    float *d0 = D, *d1 = D + n;
    int32_t *s0 = S, *s1 = S + n;
    for (int j = 0; j < n; ++j) { d0[j] = fabsf(q[0] - t[j]); s0[j] = j; }
    for (int i = 1; i < m; ++i) {
        d1[0] = d0[0] + fabsf(q[i] - t[0]);
        s1[0] = s0[0];
        for (int j = 1; j < n; ++j) {
            float best = d0[j - 1];
            int32_t s = s0[j - 1];
            if (d0[j] < best) { best = d0[j]; s = s0[j]; }
            if (d1[j - 1] < best) { best = d1[j - 1]; s = s1[j - 1]; }
            d1[j] = fabsf(q[i] - t[j]) + best;
            s1[j] = s;
        }
        float *td = d0; d0 = d1; d1 = td;
        int32_t *ts = s0; s0 = s1; s1 = ts;
    }
    rec_t r = {d0[0], 0, s0[0]};
    for (int j = 1; j < n; ++j)
        if (d0[j] < r.score) { r.score = d0[j]; r.end = j; r.start = s0[j]; }
    return r;
}

static uint32_t rng_state = 12345u;
static float gauss_ish(void) {  /* a sum of four uniforms: the shape of the values does not matter to the time */
    float s = 0.0f;
    for (int k = 0; k < 4; ++k) {
        rng_state = rng_state * 1664525u + 1013904223u;
        s += (float)(rng_state >> 8) * (1.0f / 16777216.0f);
    }
    return (s - 2.0f) * 1.7320508f;
}

int main(int argc, char **argv) {
    const int nq = argc > 1 ? atoi(argv[1]) : 20, m = argc > 2 ? atoi(argv[2]) : 250;
    const int nt = argc > 3 ? atoi(argv[3]) : 2, n = argc > 4 ? atoi(argv[4]) : 30000;
    if (nq < 1 || m < 1 || nt < 1 || n < 1) return 2;
    float *q = malloc((size_t)nq * m * sizeof(float)), *t = malloc((size_t)nt * n * sizeof(float));
    float *D = malloc((size_t)2 * n * sizeof(float));
    int32_t *S = malloc((size_t)2 * n * sizeof(int32_t));
    if (!q || !t || !D || !S) return 1;
    for (size_t i = 0; i < (size_t)nq * m; ++i) q[i] = gauss_ish();
    for (size_t i = 0; i < (size_t)nt * n; ++i) t[i] = gauss_ish();
    struct timespec a, b;
    double sum = 0.0;
    clock_gettime(CLOCK_MONOTONIC, &a);
    for (int qi = 0; qi < nq; ++qi)
        for (int ti = 0; ti < nt; ++ti) {
            const rec_t r = sdtw(q + (size_t)qi * m, m, t + (size_t)ti * n, n, D, S);
            sum += r.score + r.end + r.start;
        }
    clock_gettime(CLOCK_MONOTONIC, &b);
    const double ms = (b.tv_sec - a.tv_sec) * 1e3 + (b.tv_nsec - a.tv_nsec) * 1e-6;
    const double cells = (double)nq * nt * m * n;
    printf("{\"c_one_thread\": {\"n_queries\": %d, \"query_len\": %d, \"n_targets\": %d, \"target_len\": %d, \"ms\": %.3f, "
           "\"cells_per_s\": %.4g, \"checksum\": %.6f}}\n", nq, m, nt, n, ms, cells / (ms * 1e-3), sum);
    return 0;
}
