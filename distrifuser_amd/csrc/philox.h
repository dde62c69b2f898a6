// Philox4x32-10 (Salmon et al., "Parallel Random Numbers: As Easy as 1, 2, 3";
// the Random123 constants) and the standard normals the stochastic scheduler
// steps add, as a pure function of (seed, draw, element index):
//
//   q       = i >> 2                       (i: flat element index, 64 bits)
//   counter = (lo32(q), hi32(q), draw, 0)
//   key     = (lo32(seed), hi32(seed))
//   r0..r3  = philox4x32_10(counter, key)
//
// and by Box-Muller in fp32, (ra, rb) = (r0, r1) for z0, z1 and (r2, r3) for
// z2, z3:
//
//   u1  = ((ra >> 8) + 1) * 2^-24          in (0, 1], exact
//   u2  = (rb >> 8) * 2^-24                in [0, 1), exact
//   rad = sqrtf(-2 * logf(u1))
//   (z_even, z_odd) = (rad * cosf(2pi * u2), rad * sinf(2pi * u2))
//
// Element i takes z[i & 3]; |z| <= sqrt(48 ln 2) ~ 5.77. The precise logf /
// sincosf, never the fast intrinsics: ops/eager.py holds the same rule in torch
// integer ops and the tests bound the two against each other. Nothing here
// depends on the element type, the vector width or the launch geometry, so a
// draw is the same bits on every path that asks for it.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

struct PhiloxKey {
    uint32_t k0, k1;  // lo32(seed), hi32(seed)
    uint32_t draw;
};

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                              uint32_t k0, uint32_t k1, uint32_t (&r)[4]) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
    constexpr uint32_t W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
        const uint32_t hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += W0;
        k1 += W1;
    }
    r[0] = c0;
    r[1] = c1;
    r[2] = c2;
    r[3] = c3;
}

__device__ __forceinline__ void box_muller(uint32_t ra, uint32_t rb, float& z_even,
                                           float& z_odd) {
#pragma clang fp contract(off)
    const float u1 = (float)((ra >> 8) + 1u) * 0x1p-24f;
    const float u2 = (float)(rb >> 8) * 0x1p-24f;
    const float rad = sqrtf(-2.f * logf(u1));
    float s, c;
    sincosf(6.28318530717958647692f * u2, &s, &c);
    z_even = rad * c;
    z_odd = rad * s;
}

// the four normals of block q: elements 4q .. 4q + 3
__device__ __forceinline__ void philox_normal4(const PhiloxKey& key, uint64_t q, float (&z)[4]) {
    uint32_t r[4];
    philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), key.draw, 0u, key.k0, key.k1, r);
    box_muller(r[0], r[1], z[0], z[1]);
    box_muller(r[2], r[3], z[2], z[3]);
}

// the normal of element i alone: its block, then its lane
__device__ __forceinline__ float philox_normal1(const PhiloxKey& key, uint64_t i) {
    uint32_t r[4];
    philox4x32_10((uint32_t)(i >> 2), (uint32_t)(i >> 34), key.draw, 0u, key.k0, key.k1, r);
    const bool hi = (i & 2) != 0;
    float ze, zo;
    box_muller(hi ? r[2] : r[0], hi ? r[3] : r[1], ze, zo);
    return (i & 1) ? zo : ze;
}
