// The gadget bookkeeping of hint generation on resident buffers, the part the device kernel (kernel_rlwe.hpp:
// k_ct_ks_hint), its entry point (alch_ct_ks_hint) and the stand-alone host check (tests/sanitize/hints_harness.cpp) share.  Plain
// C++: it compiles with hipcc and with a host compiler alone.
//
// A gadget of D entries over L limbs: entry t belongs to limb i(t) and carries the scalar 2^d(t) on that limb, 0 on every other one.
//   TrivGad      D = L, i(t) = t, d(t) = 0
//   BaseBGad 2   D = sum_i ceil(log2 q_i), the digits of limb 0 first, least significant first (alch_hint_load, alch_decompose_base2)
// Both are one table first[0 .. L] of digit offsets (first[L] = D): i(t) is the limb with first[i] <= t < first[i + 1] and
// d(t) = t - first[i].  2^d(t) < q_i(t) always, so the scalar needs no table of its own.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define ALCH_GADGET_HD __host__ __device__ inline
#else
#define ALCH_GADGET_HD inline
#endif

namespace alch {
namespace hintgad {

constexpr int MAX_LIMBS = 8;                                     // MAXL of kernels_ntt.hpp

struct Layout {
    uint32_t first[MAX_LIMBS + 1];                               // first[i]: the first entry of limb i; first[L .. MAX_LIMBS] = D
    uint32_t L, D;
};

// ceil(log2 q) for q >= 1: the number of base-2 digits BaseBGad 2 gives a limb of modulus q (base2_layout in alchemy_hip.hip).
inline uint32_t digits_base2(uint64_t q) {
    uint32_t k = 0;
    for (uint64_t v = 1; v < q && k < 64; v <<= 1) ++k;          // q > 2^63: v wraps to 0 after 64 steps, k stops the loop
    return k;
}

// base2 = false: TrivGad.  L <= MAX_LIMBS.
inline Layout make_layout(const uint64_t* q, int L, bool base2) {
    Layout G;
    uint32_t D = 0;
    for (int i = 0; i <= MAX_LIMBS; ++i) {
        G.first[i] = D;
        if (i < L) D += base2 ? digits_base2(q[i]) : 1u;
    }
    G.L = (uint32_t)L;
    G.D = D;
    return G;
}

// Entry t < D -> (limb, exponent): a fixed scan, no division and no branch on the device.
ALCH_GADGET_HD void entry(const Layout& G, uint32_t t, uint32_t& limb, uint32_t& exponent) {
    uint32_t i = 0;
#pragma unroll
    for (int j = 1; j < MAX_LIMBS; ++j) i += ((uint32_t)j < G.L && G.first[j] <= t) ? 1u : 0u;
    limb = i;
    exponent = t - G.first[i];
}

// Counter of word (limb j, slot k) of the ODD element of pair `pair` in an array of L-limb, n-slot elements: the position
// alch_buf_fill_uniform gives that word, mod 2^64 (pair = ct0 + e of alch_ct_encrypt and alch_ct_ks_hint).
ALCH_GADGET_HD uint64_t odd_word_pos(uint64_t pair, uint32_t L, uint32_t j, uint32_t n, uint32_t k) {
    return ((2 * pair + 1) * (uint64_t)L + j) * (uint64_t)n + k;
}

}  // namespace hintgad
}  // namespace alch
