// sin and cos of the point kernels' hi+lo mode, usable from host code as well: tests/sincos_bits.cpp compares this form bit for bit with the one it
// replaced (same reduction, same polynomials, the quadrant's swap and signs as three compares and four selects) over the fp32 patterns.
#pragma once
#include <cstdint>
#include <cstring>
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DPN_SC_HD __host__ __device__ __forceinline__
#else
#define DPN_SC_HD static inline
#endif

DPN_SC_HD uint32_t dpn_sc_bits(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_bit_cast(uint32_t, x);
#else
    uint32_t u; memcpy(&u, &x, 4); return u;
#endif
}
DPN_SC_HD float dpn_sc_float(uint32_t u) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_bit_cast(float, u);
#else
    float x; memcpy(&x, &u, 4); return x;
#endif
}

// The quadrant q = k mod 4 of the reduced angle: s = sin, c = cos of r + q pi/2 from sp = sin r, cp = cos r.
//   odd q swaps the two; s is negated in quadrants 2, 3 (bit 1 of q), c in quadrants 1, 2 (bit 1 of q + 1 = bit 1 ^ bit 0 of q).
// A negation is a flip of bit 31, NaNs included, and adding 2^31 modulo 2^32 flips bit 31: both signs are shift-and-add on the bits (v_lshl_add_u32),
// no compare and no select beside the swap's.  Only bits 0 and 1 of q are read: k beyond the int range (the conversion saturates) gives what it gave.
DPN_SC_HD void sincos_quadrant(const uint32_t q, const float sp, const float cp, float& s, float& c) {
    const bool odd = (q & 1u) != 0u;
    const float ss = odd ? cp : sp;
    const float cc = odd ? sp : cp;
    const uint32_t m = q & 2u;
    const uint32_t sb = (m << 30) + dpn_sc_bits(ss);
    s = dpn_sc_float(sb);
    c = dpn_sc_float((q << 31) + ((m << 30) + dpn_sc_bits(cc)));
}

// Cody-Waite reduction by pi/2 + minimax polynomials, |err| ~1e-7 for |theta| up to a few hundred.
DPN_SC_HD void sincos_precise(float th, float& s, float& c) {
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
    sincos_quadrant((uint32_t)(int)k, sp, cp, s, c);
}
