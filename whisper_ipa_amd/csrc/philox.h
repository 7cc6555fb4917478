// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) and the Gumbel noise of the sampling tail.
// Counter-based: the four output words are a pure function of (counter, key), so a column's noise never depends on which thread,
// workgroup or batch row computes it.  Host and device compile the same text (the known answers are checked on the host).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WIPA_HD __host__ __device__ __forceinline__
#else
#define WIPA_HD inline
#endif

struct Philox4 {
    uint32_t w[4];
};

WIPA_HD uint32_t philox_mulhi(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(a, b);
#else
    return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32);
#endif
}

WIPA_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = philox_mulhi(M0, c0), lo0 = M0 * c0;
        const uint32_t hi1 = philox_mulhi(M1, c2), lo1 = M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += W0;  // the key schedule: bumped between rounds (the bump after the last round is unused)
        k1 += W1;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// u = ((word >> 9) + 0.5) * 2^-23 in (0, 1): 23 random bits and the half are exact in f32, so u is the same number everywhere.
// g = -log(-log(u)) in (-2.8, 16.7).  logf, not the fast intrinsic: the inner logarithm is taken next to 1 for the large draws,
// where an absolute error of the fast path is a large relative one.
WIPA_HD float gumbel_from_word(uint32_t word) {
    const float u = ((float)(word >> 9) + 0.5f) * 1.1920928955078125e-07f;
    return -logf(-logf(u));
}
