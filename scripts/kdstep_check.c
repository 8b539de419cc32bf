/* Exactness check of the two short forms of one kd decision (csrc/traverse.hpp kd_step):
 *
 * 1. kd_below (device_math.hpp): the side of the split plane the ray starts on,
 *        below = (oa < split) || (oa == split && da <= 0)          (kdtree.cpp:267-268, 334-335)
 *    taken from the difference a = split - oa the step has already formed,
 *        below = -a < (da <= 0 ? 2^-149 : 0).
 *    Compared on every pair of a list of edge coordinates (zeros of both signs, the smallest and largest
 *    denormals and normals, neighbours of 1, values whose difference is denormal or overflows, NaN) crossed
 *    with every da of {-0, +0, +-2^-149, +-2^-126, +-2^-41 (an axis whose reciprocal is NaN), +-1, +-inf, NaN},
 *    and on 2^26 random pairs of nearby floats.  Infinite coordinates of equal sign are left out: oa == split
 *    holds for them while a is NaN (the kernels' coordinates are finite: queryroute.hpp sends any other
 *    query to the kernel that keeps the reference's expression).
 *
 * 2. div_by_rcp_wave_bounded (device_math.hpp): Markstein's correction from y = RN(1/b),
 *        q0 = RN(a*y);  r = fma(-q0, b, a);  q = fma(r, y, q0)   when |q0| >= 2^-60, else a / b,
 *    without the upper test |q0| <= 2^60 of div_by_rcp, claimed equal to RN(a/b) for 2^-40 <= |b| <= 2^40 and
 *    |a| <= 2^20 (where |q0| <= 2^60 follows).  The pairs are scripts/markstein_check.c's: every b significand
 *    (2^23) with per_b values of a, half of them random, half built so that a/b sits next to a rounding
 *    midpoint, exponents spread over the domain and up to its edges (|a| = 2^20, |b| = 2^-40 and 2^40 included).
 *    The default per_b of 2048 gives 1.7e10 pairs.
 *
 *   gcc -O2 -fopenmp -ffp-contract=off scripts/kdstep_check.c -o /tmp/kc -lm && /tmp/kc [per_b]
 * Prints the counts; exit status 1 on any difference.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static inline float fbits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static inline uint32_t ubits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline uint64_t mix64(uint64_t x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdULL; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL; x ^= x >> 33;
    return x;
}

/* the reference's expression and the kernel's (volatile: the difference is formed as a float, once) */
static int below_ref(float oa, float split, float da) { return (oa < split) || (oa == split && da <= 0); }
static int below_new(float oa, float split, float da) {
    volatile float a = split - oa;
    return -a < (da <= 0.f ? fbits(1u) : 0.f);
}
static float div_bounded(float a, float b, float y) {
    const float q0 = a * y;
    if (fabsf(q0) >= ldexpf(1.f, -60)) return fmaf(fmaf(-q0, b, a), y, q0);
    return a / b;
}

static long long check_below(void) {
    static const uint32_t cbits[] = {
        0x00000000u, 0x80000000u, 0x00000001u, 0x80000001u, 0x00000002u, 0x007fffffu, 0x807fffffu, 0x00800000u,
        0x80800000u, 0x00800001u, 0x00ffffffu, 0x01000000u, 0x33800000u, 0x3f7fffffu, 0x3f800000u, 0xbf800000u,
        0x3f800001u, 0xbf800001u, 0x40490fdbu, 0xc0490fdbu, 0x49742400u, 0x7f7fffffu, 0xff7fffffu, 0x7f7ffffeu,
        0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u};
    static const uint32_t dbits[] = {0x80000000u, 0x00000000u, 0x00000001u, 0x80000001u, 0x00800000u, 0x80800000u,
                                     0x2b000000u, 0xab000000u, 0x3f800000u, 0xbf800000u, 0x7f800000u, 0xff800000u,
                                     0x7fc00000u, 0xffc00000u};
    const int nc = (int)(sizeof cbits / sizeof cbits[0]), nd = (int)(sizeof dbits / sizeof dbits[0]);
    long long tested = 0, bad = 0, denormal_a = 0, equal = 0;
    for (int i = 0; i < nc; i++)
        for (int j = 0; j < nc; j++) {
            const float oa = fbits(cbits[i]), split = fbits(cbits[j]);
            if (isinf(oa) && isinf(split) && oa == split) continue;
            for (int k = 0; k < nd; k++) {
                const float da = fbits(dbits[k]);
                tested++;
                if (below_ref(oa, split, da) != below_new(oa, split, da)) {
                    if (bad++ < 10) fprintf(stderr, "BELOW oa=%a split=%a da=%a\n", oa, split, da);
                }
            }
        }
    /* random nearby pairs: split a few ulps from oa (equal included), over all exponents, so that the difference
       is exact, tiny, and often denormal */
#pragma omp parallel for reduction(+ : tested, bad, denormal_a, equal)
    for (uint32_t n = 0; n < (1u << 26); n++) {
        const uint64_t s = mix64(n + 12345u);
        const uint32_t e = (uint32_t)(s % 255u); /* 0: denormals and zero */
        const uint32_t ob = ((uint32_t)(s >> 8) & 1u) << 31 | e << 23 | ((uint32_t)(s >> 16) & 0x7fffffu);
        const int step = (int)((s >> 40) % 9u) - 4;
        uint32_t sb = ob;
        if ((ob & 0x7fffffffu) + 4u < 0x7f800000u && (ob & 0x7fffffffu) >= 4u) sb = (uint32_t)((int32_t)ob + step);
        const float oa = fbits(ob), split = fbits(sb);
        const float da = fbits(dbits[(s >> 48) % (uint64_t)nd]);
        const float a = split - oa;
        tested++;
        denormal_a += a != 0.f && fabsf(a) < ldexpf(1.f, -126);
        equal += oa == split;
        if (below_ref(oa, split, da) != below_new(oa, split, da)) {
            if (bad < 10)
#pragma omp critical
                fprintf(stderr, "BELOW oa=%a split=%a da=%a\n", oa, split, da);
            bad++;
        }
    }
    printf("below: tested %lld (denormal difference %lld, oa == split %lld) differing %lld\n", tested, denormal_a,
           equal, bad);
    if (!denormal_a || !equal) {
        fprintf(stderr, "below: the random pairs reached no denormal difference or no equality\n");
        return bad + 1;
    }
    return bad;
}

int main(int argc, char **argv) {
    const int per_b = argc > 1 ? atoi(argv[1]) : 2048;
    long long bad_below = check_below();
    const float hi_a = ldexpf(1.f, 20), hi_q = ldexpf(1.f, 60), lo_q = ldexpf(1.f, -60);
    long long tested = 0, skipped = 0, bad = 0, slow = 0, over = 0;
#pragma omp parallel for schedule(dynamic, 4096) reduction(+ : tested, skipped, bad, slow, over)
    for (uint32_t m = 0; m < (1u << 23); m++) {
        uint64_t s = mix64(m + 1);
        for (int k = 0; k < per_b; k++) {
            s = mix64(s + k);
            const int eb = (int)(s % 81) - 40;                       /* b exponent in [-40, 40] */
            const uint32_t sb = (uint32_t)(s >> 8) & 1u;
            /* |b| <= 2^40: at exponent 40 only the significand 1.0 */
            const float b = fbits((sb << 31) | ((uint32_t)(eb + 127) << 23) | (eb == 40 ? 0u : m));
            float a;
            if (k & 1) {
                /* a/b next to a midpoint: a random q, its midpoint with the next float, a = RN(mid * b) (double
                 * product rounded once to float), the exponent of q such that |a| stays inside 2^20 */
                const int top = 19 - eb < 50 ? 19 - eb : 50;
                const int eq = top - (int)((s >> 16) % 101);
                const float q = fbits(((uint32_t)(eq + 127) << 23) | ((uint32_t)(s >> 24) & 0x7fffffu));
                const double mid = ((double)q + (double)nextafterf(q, INFINITY)) * 0.5;
                a = (float)(mid * (double)b);
                if (s & (1ull << 60)) a = nextafterf(a, INFINITY);
                if (s & (1ull << 61)) a = nextafterf(a, -INFINITY);
            } else {
                /* a random a with its exponent within 50 of b's and at most 19; one in 64 is +-2^20 itself */
                const int top = eb + 50 < 19 ? eb + 50 : 19;
                const int ea = top - (int)((s >> 16) % 101);
                if (ea < -100) { skipped++; continue; }
                a = fbits(((uint32_t)(s >> 40) & 1u) << 31 | ((uint32_t)(ea + 127) << 23) |
                          ((uint32_t)(s >> 41) & 0x7fffffu));
                if (((s >> 2) & 63u) == 0u) a = copysignf(hi_a, a);
            }
            if (!(fabsf(a) <= hi_a)) { skipped++; continue; }
            const float y = 1.f / b;
            const float q0 = a * y;
            over += fabsf(q0) > hi_q;               /* the bound the dropped test stood for: never */
            slow += !(fabsf(q0) >= lo_q);
            const float q = div_bounded(a, b, y), ref = a / b;
            tested++;
            if (ubits(q) != ubits(ref)) {
                if (bad < 10)
#pragma omp critical
                    fprintf(stderr, "MISMATCH a=%a b=%a q=%a ref=%a\n", a, b, q, ref);
                bad++;
            }
        }
    }
    printf("division: tested %lld (full division %lld) skipped %lld, |q0| > 2^60 %lld, differing %lld\n", tested, slow,
           skipped, over, bad);
    return bad != 0 || over != 0 || bad_below != 0;
}
