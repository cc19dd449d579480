// median_literal.h -- the reference's selection (src/ksort.h:233-259, called from src/stat.h:56-73), restated step for
// step, for the medians whose VALUE does not settle them.
//
// A median is the element of rank n / 2, and for int16 samples any exact selection returns it.  For pA values it is the
// element the reference's own exchanges leave at position n / 2 of its copy, and that is more than a value: +0 and -0
// compare equal and print differently, and a NaN orders with nothing.  With a finite offset and a finite non-zero unit,
// pA values that compare equal have the same bits unless they are zeros (a product that underflows keeps the sign of
// raw + offset), so pA(raw order statistic) can differ from the reference's pick only when it == 0.0f or when the unit or
// the offset is not finite (median_is_a_pick).  Those medians are redone here, by ONE LANE, on a scratch copy.
//
// The steps, on the working range [lo, hi] around k:
//   - one element: done; two: put them in order, done;
//   - order a[mid], a[lo], a[hi] with three conditional exchanges (hi against mid, hi against lo, lo against mid), so
//     that a[lo] is the pivot, and park a[mid] at lo + 1;
//   - i walks up from lo + 1 past elements below the pivot, j down from hi past elements above it, both stepping
//     before they look; while they have not crossed, exchange a[i] and a[j];
//   - the pivot goes to j; the side(s) of j that hold k stay.
// a[hi] is never below the pivot and a[lo + 1] never above it, so i stops at hi and j at lo + 1 at the latest, whatever
// `lt` says about NaNs (it says false); the two range tests in the scans never decide anything and are there so that
// no comparator can walk a lane out of its scratch.
#pragma once
#include "sgk_common.h"

namespace sgk {

template <typename T, typename LT>
__device__ inline T literal_select(T *a, int64_t n, int64_t k, LT lt) {
    int64_t lo = 0, hi = n - 1;
    auto swap = [&](int64_t p, int64_t q) { const T t = a[p]; a[p] = a[q]; a[q] = t; };
    for (;;) {
        if (hi <= lo) return a[k];
        if (hi == lo + 1) {
            if (lt(a[hi], a[lo])) swap(lo, hi);
            return a[k];
        }
        const int64_t mid = lo + (hi - lo) / 2;
        if (lt(a[hi], a[mid])) swap(mid, hi);
        if (lt(a[hi], a[lo])) swap(lo, hi);
        if (lt(a[lo], a[mid])) swap(mid, lo);
        swap(mid, lo + 1);
        const T pivot = a[lo];
        int64_t i = lo + 1, j = hi;
        for (;;) {
            do ++i; while (i < hi && lt(a[i], pivot));
            do --j; while (j > lo && lt(pivot, a[j]));
            if (j < i) break;
            swap(i, j);
        }
        swap(lo, j);
        if (j <= k) lo = i;
        if (j >= k) hi = j - 1;
    }
}

// ---- the sign of a NaN.  The reference runs on x86 (SSE): an operation with a NaN operand returns THAT operand (the first
// one if both are), quieted, sign and all, and an invalid operation (inf - inf, 0 * inf, 0 / 0) returns the negative
// quiet NaN 0xffc00000 -- which is why the reference prints `-nan`.  The GPU's subtraction is an addition with a negated
// operand (the NaN's sign flips), its correctly rounded division and square root are instruction sequences, and the wave
// kernels' sums are oriented (seqsum.h): the value is a NaN either way, its sign bit is not the reference's.  Reads whose
// unit or offset is not finite -- only those can hold a NaN -- get their pA mean and deviation redone by one lane with
// every operation spelled the x86 way (k_median_literal, k_statf_literal); everywhere else the results are identical.
// (The FIRST NaN operand: that is the order in which the reference binary this project records its goldens from -- gcc -O2,
// oracle/Makefile -- hands the operands of `sum += x[i]`, `x[i] - m` and `d * d` to the instruction.  A compiler may swap the
// operands of an addition or a multiplication, so where both are NaNs of different signs -- float arrays with NaNs of both
// signs -- another build of the reference may print the other sign: that would be the build, not these kernels.)
__device__ __forceinline__ float x86_result(float r, float a, float b) {
    if (a != a) return __uint_as_float(__float_as_uint(a) | 0x00400000u);
    if (b != b) return __uint_as_float(__float_as_uint(b) | 0x00400000u);
    return r != r ? __uint_as_float(0xffc00000u) : r;
}
__device__ __forceinline__ float x86_add(float a, float b) { return x86_result(a + b, a, b); }
__device__ __forceinline__ float x86_sub(float a, float b) { return x86_result(a - b, a, b); }
__device__ __forceinline__ float x86_mul(float a, float b) { return x86_result(a * b, a, b); }
__device__ __forceinline__ float x86_div(float a, float b) { return x86_result(a / b, a, b); }
__device__ __forceinline__ float x86_sqrt(float a) { return x86_result(sqrtf(a), a, a); }
// signal_in_picoamps (src/misc.c:26-28)
__device__ __forceinline__ float x86_to_pa(int16_t raw, const Scale &s) { return x86_mul(x86_add((float)raw, s.offf), s.unit); }
// meanf and stdvf (src/stat.h:17-44) of x(0) .. x(n - 1), strictly in order
template <typename X>
__device__ inline void x86_mean_std(int64_t n, X x, float &mean, float &sd) {
    const float nf = (float)(int)n;
    float s = 0.0f;
    for (int64_t i = 0; i < n; ++i) s = x86_add(s, x(i));
    mean = x86_div(s, nf);
    float q = 0.0f;
    for (int64_t i = 0; i < n; ++i) {
        const float d = x86_sub(x(i), mean);
        q = x86_add(q, x86_mul(d, d));
    }
    sd = x86_sqrt(x86_div(q, nf));
}
__device__ __forceinline__ bool scale_is_finite(const Scale &sc) {
    const float inf = __builtin_inff();
    return fabsf(sc.unit) < inf && fabsf(sc.offf) < inf;
}

// can the reference's pick differ from pA(raw order statistic) = pm?
__device__ __forceinline__ bool median_is_a_pick(float pm, const Scale &sc) {
    return pm == 0.0f || !scale_is_finite(sc);
}

}  // namespace sgk
