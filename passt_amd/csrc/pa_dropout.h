// The attention-dropout mask rule: a pure function of a 64-bit seed and the element's position, shared by the kernels of
// attention.hip and by the host entry pa_attention_dropout_mask (api of include/passt_amd.h, "attention dropout").
//
//   t = round(256 p), active for 1 <= t <= 255; element (site, s = b H + h, query q, key k) of the probabilities:
//     R    = philox4x32_10(counter = (k >> 2, q >> 2, s, site), key = (seed[0], seed[1]))
//     byte = (R[q & 3] >> (8 (k & 3))) & 0xff
//     kept <=> byte >= t
// One call covers a patch of 4 queries x 4 keys: word = query inside the patch, byte = key inside the patch.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PA_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define PA_HD inline
#endif

namespace pa {

struct Philox4 { uint32_t w[4]; };

PA_HD void philox_mulhilo(uint32_t a, uint32_t b, uint32_t& hi, uint32_t& lo) {
    const uint64_t p = (uint64_t)a * (uint64_t)b;               // device: v_mul_lo_u32 + v_mul_hi_u32
    lo = (uint32_t)p;
    hi = (uint32_t)(p >> 32);
}

// Philox4x32 with 10 rounds (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11), standard constants
PA_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        uint32_t hi0, lo0, hi1, lo1;
        philox_mulhilo(0xD2511F53u, c0, hi0, lo0);
        philox_mulhilo(0xCD9E8D57u, c2, hi1, lo1);
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    Philox4 o;
    o.w[0] = c0; o.w[1] = c1; o.w[2] = c2; o.w[3] = c3;
    return o;
}

// the four words of the patch that holds queries 4 qp .. 4 qp + 3 and keys 4 kp .. 4 kp + 3 of (site, s)
PA_HD Philox4 dropout_patch(uint32_t seed0, uint32_t seed1, uint32_t site, uint32_t s, uint32_t qp, uint32_t kp) {
    return philox4x32_10(kp, qp, s, site, seed0, seed1);
}
// byte j of a word against the threshold
PA_HD bool dropout_kept(uint32_t word, int j, uint32_t t) { return ((word >> (8 * j)) & 0xffu) >= t; }

// the rule for one element, as the text above states it
PA_HD bool dropout_keep(uint32_t seed0, uint32_t seed1, uint32_t site, uint32_t s, uint32_t q, uint32_t k, uint32_t t) {
    const Philox4 r = dropout_patch(seed0, seed1, site, s, q >> 2, k >> 2);
    return dropout_kept(r.w[q & 3], (int)(k & 3), t);
}

}  // namespace pa
