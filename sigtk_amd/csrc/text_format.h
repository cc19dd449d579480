/* text_format.h -- the numbers of the TSV rows as characters, for the host and for HIP device code.
 *
 * The reference prints integers with "%ld" / "%d" and every float with printf("%f") (src/cfunc.c:19-56,
 * 90-96).  This header produces exactly those bytes, and their count alone (the measure pass of the
 * device-side writer, csrc/text_kernels.hip, needs counts before any byte has a place to go), from
 * plain C: the CLI's C99 build compiles it with gcc (`sigtk-amd _textcheck` compares it with glibc's
 * snprintf), the kernels compile the same lines for gfx950.
 *
 * Digits are written backwards from the end of their field, which is known from the count: no
 * temporary character array, so on the device nothing is indexed at run time but the destination.
 *
 * "%f" of a float (promoted to double, six decimals, the exact decimal expansion rounded half to even):
 *   |v| < 1e15   v = ip + frac, both exact; frac has at most 24 significant bits and 10^6 = 15625 * 2^6,
 *                so frac * 1e6 is exact in double and rint() of it is the correctly rounded fraction;
 *                a carry into ip when it reaches 10^6 (the argument of host/fmt.h, unchanged).
 *   |v| >= 1e15  the float is an integer m * 2^e below 2^128: four 32-bit limbs, divided by 10^9 five
 *                times (39 digits at most), then ".000000".
 *   inf / nan    "inf", "-inf", "nan", "-nan" (glibc prints the sign bit of a NaN).
 * No operation here can be contracted into an FMA (there is no multiply feeding an add); the library
 * is built with -ffp-contract=off all the same.
 */
#ifndef SGK_TEXT_FORMAT_H
#define SGK_TEXT_FORMAT_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define SGK_TF __host__ __device__ static inline
#else
#define SGK_TF static inline
#endif

#define SGK_TF_F32_MAX_BYTES 47 /* "-340282346638528859811704183484516925440.000000" */
#define SGK_TF_I64_MAX_BYTES 20 /* "-9223372036854775808" */

/* number of decimal digits of v (1 for 0) */
SGK_TF int sgk_tf_u32_len(uint32_t v) {
    return 1 + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) +
           (v >= 10000000u) + (v >= 100000000u) + (v >= 1000000000u);
}
SGK_TF int sgk_tf_u64_len(uint64_t v) {
    if (v <= 0xffffffffull) return sgk_tf_u32_len((uint32_t)v);
    const uint64_t hi = v / 1000000000ull; /* >= 4, < 1.9e10 */
    if (hi <= 0xffffffffull && (uint32_t)hi < 1000000000u) return 9 + sgk_tf_u32_len((uint32_t)hi);
    return 18 + sgk_tf_u32_len((uint32_t)(hi / 1000000000ull));
}
SGK_TF int sgk_tf_i64_len(int64_t v) {
    return v < 0 ? 1 + sgk_tf_u64_len((uint64_t)0 - (uint64_t)v) : sgk_tf_u64_len((uint64_t)v);
}

/* the n low decimal digits of v into p[0 .. n), most significant first (zero-padded on the left) */
SGK_TF void sgk_tf_digits(char *p, uint32_t v, int n) {
    while (n >= 2) {
        const uint32_t q = v / 100u, d = v - q * 100u, t = d / 10u;
        n -= 2;
        p[n] = (char)('0' + t);
        p[n + 1] = (char)('0' + (d - t * 10u));
        v = q;
    }
    if (n) p[0] = (char)('0' + v % 10u);
}

/* "%lu": writes sgk_tf_u64_len(v) bytes at p and returns that count */
SGK_TF int sgk_tf_u64(char *p, uint64_t v) {
    const int n = sgk_tf_u64_len(v);
    int k = n;
    while (v > 0xffffffffull) { /* at most twice */
        const uint64_t q = v / 1000000000ull;
        k -= 9;
        sgk_tf_digits(p + k, (uint32_t)(v - q * 1000000000ull), 9);
        v = q;
    }
    uint32_t w = (uint32_t)v;
    if (k > 9) { /* a 10-digit 32-bit value in front of nothing, or 10+ digits left of the 9-digit groups */
        const uint32_t q = w / 1000000000u;
        k -= 9;
        sgk_tf_digits(p + k, w - q * 1000000000u, 9);
        w = q;
    }
    sgk_tf_digits(p, w, k);
    return n;
}
/* "%ld" */
SGK_TF int sgk_tf_i64(char *p, int64_t v) {
    if (v < 0) {
        *p = '-';
        return 1 + sgk_tf_u64(p + 1, (uint64_t)0 - (uint64_t)v);
    }
    return sgk_tf_u64(p, (uint64_t)v);
}

/* "%d" of an int16 (the raw_signal column of a text SLOW5 record): 1 to 6 bytes */
#define SGK_TF_I16_MAX_BYTES 6 /* "-32768" */
SGK_TF int sgk_tf_i16_len(int16_t v) {
    const uint32_t a = v < 0 ? (uint32_t)(-(int32_t)v) : (uint32_t)v;
    return (v < 0) + 1 + (a >= 10u) + (a >= 100u) + (a >= 1000u) + (a >= 10000u);
}
/* writes sgk_tf_i16_len(v) bytes at p and returns that count */
SGK_TF int sgk_tf_i16(char *p, int16_t v) {
    const int neg = v < 0, n = sgk_tf_i16_len(v);
    if (neg) *p = '-';
    sgk_tf_digits(p + neg, neg ? (uint32_t)(-(int32_t)v) : (uint32_t)v, n - neg);
    return n;
}

SGK_TF uint32_t sgk_tf_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

/* |f| as a double; a denormal float is built from its integer mantissa, so that the result does not depend on
 * how the device's float -> double conversion treats denormals (m * 2^-149 is exact) */
SGK_TF double sgk_tf_abs(uint32_t bits, float f) {
    return (bits & 0x7f800000u) ? fabs((double)f) : (double)(bits & 0x7fffffu) * 0x1p-149;
}

/* |v| < 1e15: integer part and the six decimals as an integer below 10^6, rounded half to even */
SGK_TF void sgk_tf_split(double v, uint64_t *ip_out, uint32_t *fr_out) {
    uint64_t ip = (uint64_t)v;
    const double frac = v - (double)ip;
    uint32_t fr = (uint32_t)rint(frac * 1e6); /* exact product */
    if (fr >= 1000000u) {
        fr -= 1000000u;
        ip += 1;
    }
    *ip_out = ip;
    *fr_out = fr;
}

/* |v| >= 1e15 (finite): v = m * 2^e as four 32-bit limbs, then its five groups of nine decimal digits
 * g[0] (least significant) .. g[4]; returns the number of digits */
SGK_TF int sgk_tf_huge(uint32_t bits, uint32_t g[5]) {
    const uint32_t m = (bits & 0x7fffffu) | 0x800000u;
    const int e = (int)((bits >> 23) & 0xffu) - 150; /* 26 .. 104 */
    const int ws = e >> 5, bs = e & 31;
    const uint64_t sh = (uint64_t)m << bs; /* < 2^55 */
    const uint32_t lo = (uint32_t)sh, hi = (uint32_t)(sh >> 32);
    uint32_t l0 = 0, l1 = 0, l2 = 0, l3 = 0;
    if (ws == 0) { l0 = lo; l1 = hi; }
    else if (ws == 1) { l1 = lo; l2 = hi; }
    else if (ws == 2) { l2 = lo; l3 = hi; }
    else { l3 = lo; } /* ws == 3: e <= 104, so bs <= 8 and hi == 0 */
    for (int k = 0; k < 5; k++) {
        uint64_t r = l3;
        l3 = (uint32_t)(r / 1000000000u); r = ((r % 1000000000u) << 32) | l2;
        l2 = (uint32_t)(r / 1000000000u); r = ((r % 1000000000u) << 32) | l1;
        l1 = (uint32_t)(r / 1000000000u); r = ((r % 1000000000u) << 32) | l0;
        l0 = (uint32_t)(r / 1000000000u);
        g[k] = (uint32_t)(r % 1000000000u);
    }
    int top = 4;
    while (top > 0 && g[top] == 0) top--;
    return 9 * top + sgk_tf_u32_len(g[top]);
}

/* byte count of printf("%f", (double)f) */
SGK_TF int sgk_tf_f32_len(float f) {
    const uint32_t bits = sgk_tf_bits(f);
    const int neg = (int)(bits >> 31);
    if ((bits & 0x7f800000u) == 0x7f800000u) return 3 + neg;
    const double v = sgk_tf_abs(bits, f);
    if (v < 1e15) {
        uint64_t ip;
        uint32_t fr;
        sgk_tf_split(v, &ip, &fr);
        return neg + sgk_tf_u64_len(ip) + 7;
    }
    uint32_t g[5];
    return neg + sgk_tf_huge(bits, g) + 7;
}

/* printf("%f", (double)f): writes sgk_tf_f32_len(f) bytes (at most SGK_TF_F32_MAX_BYTES) at p, returns the count */
SGK_TF int sgk_tf_f32(char *p, float f) {
    const uint32_t bits = sgk_tf_bits(f);
    const int neg = (int)(bits >> 31);
    if (neg) *p++ = '-';
    if ((bits & 0x7f800000u) == 0x7f800000u) {
        const int nan = (bits & 0x7fffffu) != 0;
        p[0] = nan ? 'n' : 'i';
        p[1] = nan ? 'a' : 'n';
        p[2] = nan ? 'n' : 'f';
        return 3 + neg;
    }
    const double v = sgk_tf_abs(bits, f);
    int n;
    uint32_t fr = 0;
    if (v < 1e15) {
        uint64_t ip;
        sgk_tf_split(v, &ip, &fr);
        n = sgk_tf_u64(p, ip);
    } else {
        uint32_t g[5];
        n = sgk_tf_huge(bits, g);
        int k = n;
        for (int i = 0; i < 5; i++) { /* fixed trip count: g[] stays in registers once unrolled */
            if (k >= 9) {
                k -= 9;
                sgk_tf_digits(p + k, g[i], 9);
            } else if (k > 0) {
                sgk_tf_digits(p, g[i], k);
                k = 0;
            }
        }
    }
    p[n] = '.';
    sgk_tf_digits(p + n + 1, fr, 6);
    return neg + n + 7;
}

#endif
