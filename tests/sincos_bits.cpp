// Host program of tests/test_sincos_bits_cpu.py: sincos_precise of csrc/dpn_sincos.h (the quadrant's signs as bit arithmetic) against the form it
// replaced, kept here verbatim, bit for bit.  Compile with -ffp-contract=off (the polynomials are explicit fmaf calls: nothing may be fused beside them).
//   1. every 61st fp32 bit pattern (7.04e7 values: all exponents, both signs, NaNs and infinities among them);
//   2. +-0, the smallest and largest denormals and normals, +-inf, quiet and signalling NaNs of both signs;
//   3. 1e6 values around the multiples of pi/2 up to |theta| = 1e4: each multiple's fp32 neighbours within +-78 ulp, where k = rint(theta 2/pi) changes;
//   4. the quadrant alone on every residue of q, the int range's ends (the device's conversion saturates) and sp / cp patterns with NaNs of both signs.
// Prints the number of values compared and of mismatches per part; exit status 1 on any mismatch.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <cmath>
#include "dpn_sincos.h"

static void sincos_precise_old(float th, float& s, float& c) {
    const float k = rintf(th * 0.63661977236758134f);
    float r = fmaf(k, -1.5707963705062866f, th);               // float(pi/2); the fma keeps k*hi exact
    r = fmaf(k, 4.371138828673793e-08f, r);                     // pi/2 - float(pi/2)
    const float r2 = r * r;
    float sp = fmaf(r2, 2.7183114939898219064e-6f, -1.9839334836096632576e-4f);
    sp = fmaf(sp, r2, 8.3333293858894631756e-3f);
    sp = fmaf(sp, r2, -1.6666666641626524100e-1f);
    sp = fmaf(sp * r2, r, r);
    float cp = fmaf(r2, 2.4433157826443582e-5f, -1.3887316255057415e-3f);
    cp = fmaf(cp, r2, 4.1666645683529456e-2f);
    cp = fmaf(cp, r2, -0.5f);
    cp = fmaf(cp, r2, 1.0f);
    const int q = ((int)k) & 3;
    const float ss = (q & 1) ? cp : sp;
    const float cc = (q & 1) ? sp : cp;
    s = (q & 2) ? -ss : ss;
    c = ((q + 1) & 2) ? -cc : cc;
}
// the old quadrant on an integer that is given (part 4)
static void quadrant_old(int k, float sp, float cp, float& s, float& c) {
    const int q = k & 3;
    const float ss = (q & 1) ? cp : sp;
    const float cc = (q & 1) ? sp : cp;
    s = (q & 2) ? -ss : ss;
    c = ((q + 1) & 2) ? -cc : cc;
}

static uint32_t bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
static float fl(uint32_t u) { float x; memcpy(&x, &u, 4); return x; }

static long bad_total = 0;
// Beyond the int range (|theta| > 3.4e9, NaN, infinity) the quadrant is whatever the float -> int conversion returns -- one instruction on the host
// (0x80000000), a saturating one on the device -- and both forms read the same integer: part 4 covers the values the device's conversion names.
static void check(float th, long& n, long& bad) {
    float s0, c0, s1, c1;
    sincos_precise_old(th, s0, c0);
    sincos_precise(th, s1, c1);
    ++n;
    if (bits(s0) != bits(s1) || bits(c0) != bits(c1)) {
        if (bad < 5) printf("  MISMATCH theta %08x: old %08x %08x new %08x %08x\n", bits(th), bits(s0), bits(c0), bits(s1), bits(c1));
        ++bad;
    }
}

int main() {
    long n = 0, bad = 0;
    for (uint64_t u = 0; u <= 0xFFFFFFFFull; u += 61) check(fl((uint32_t)u), n, bad);
    printf("sweep: %ld values, %ld mismatches\n", n, bad);
    bad_total += bad;

    n = bad = 0;
    const uint32_t special[] = {0x00000000u, 0x80000000u, 0x00000001u, 0x80000001u, 0x007FFFFFu, 0x807FFFFFu, 0x00800000u, 0x80800000u, 0x7F7FFFFFu, 0xFF7FFFFFu,
                                0x7F800000u, 0xFF800000u, 0x7FC00000u, 0xFFC00000u, 0x7F800001u, 0xFF800001u, 0x7FFFFFFFu, 0xFFFFFFFFu, 0x4EFFFFFFu, 0xCEFFFFFFu};
    for (uint32_t u : special) check(fl(u), n, bad);
    printf("special: %ld values, %ld mismatches\n", n, bad);
    bad_total += bad;

    n = bad = 0;
    const int mmax = (int)(1.0e4 / 1.5707963267948966);            // 6366 multiples on either side
    for (int m = -mmax; m <= mmax; ++m) {
        const float centre = (float)((double)m * 1.5707963267948966);
        const uint32_t cb = bits(centre);
        for (int d = -78; d <= 78; ++d) {
            if (m == 0 && d < 0) { check(-fl((uint32_t)(-d)), n, bad); continue; }      // below zero: the negative denormals
            check(fl(cb + (uint32_t)((centre < 0.f) ? -d : d)), n, bad);
        }
    }
    printf("multiples of pi/2: %ld values, %ld mismatches\n", n, bad);
    if (n < 1000000) { printf("fewer than 1e6 values around the multiples\n"); bad_total += 1; }
    bad_total += bad;

    n = bad = 0;
    const int ks[] = {0, 1, 2, 3, 4, 5, 6, 7, -1, -2, -3, -4, -5, 2147483647, 2147483646, 2147483645, 2147483644, -2147483647 - 1, -2147483647, -2147483646, -2147483645};
    const uint32_t vals[] = {0x00000000u, 0x80000000u, 0x3F800000u, 0xBF800000u, 0x3F000000u, 0xBEAAAAABu, 0x00000001u, 0x80000001u, 0x7F800000u, 0xFF800000u,
                             0x7FC00000u, 0xFFC00000u, 0x7F800001u, 0xFFBFFFFFu};
    for (int k : ks)
        for (uint32_t a : vals)
            for (uint32_t b : vals) {
                float s0, c0, s1, c1;
                quadrant_old(k, fl(a), fl(b), s0, c0);
                sincos_quadrant((uint32_t)k, fl(a), fl(b), s1, c1);
                ++n;
                if (bits(s0) != bits(s1) || bits(c0) != bits(c1)) { ++bad; if (bad < 5) printf("  MISMATCH quadrant k %d sp %08x cp %08x\n", k, a, b); }
            }
    printf("quadrant: %ld values, %ld mismatches\n", n, bad);
    bad_total += bad;
    printf("total mismatches: %ld\n", bad_total);
    return bad_total ? 1 : 0;
}
