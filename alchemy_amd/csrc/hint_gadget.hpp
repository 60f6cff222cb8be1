// The gadget bookkeeping of hint generation on resident buffers, the part the device kernel (kernel_rlwe.hpp:
// k_ct_ks_hint), its entry point (alch_ct_ks_hint) and the stand-alone host check (tests/sanitize/hints_harness.cpp) share.  Plain
// C++: it compiles with hipcc and with a host compiler alone.
//
// A gadget of D entries over L limbs: entry t belongs to limb i(t) and carries the scalar 2^(w d(t)) on that limb, 0 on every other one.
//   TrivGad        D = L, i(t) = t, d(t) = 0 (w = 0)
//   BaseBGad 2     D = sum_i ceil(log2 q_i), the digits of limb 0 first, least significant first (alch_hint_load, alch_decompose_base2)
//   BaseBGad 2^w   D = sum_i ceil(ceil(log2 q_i) / w), same order (ALCH_GAD_BASEPOW2(w), 1 <= w <= 16; w = 1 is BaseBGad 2)
// All are one table first[0 .. L] of digit offsets (first[L] = D): i(t) is the limb with first[i] <= t < first[i + 1] and
// d(t) = t - first[i].  k_i is the smallest k with 2^(w k) >= q_i, so 2^(w d(t)) <= 2^(w (k_i - 1)) < q_i(t) always and the scalar
// needs no table of its own.
//
// The digits themselves (Lol's divModCent, oracle/model.py: decompose_baseb) also live here, in the closed form the digit loaders
// use: pow2_offset / pow2_digit below.
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
    uint32_t w;                                                  // log2 of the base: 0 TrivGad, 1 BaseBGad 2, up to MAX_WIDTH
};

constexpr uint32_t MAX_WIDTH = 16;                               // ALCH_GAD_BASEPOW2(w): 1 <= w <= 16

// Gadget code -> log2 of the base: 0 for TrivGad (code 0), w for BaseBGad 2^w (code 1, or 0x100 | w with 1 <= w <= 16), -1 for
// every other code.  The one predicate behind every entry point that takes a gadget.
inline int gadget_width(int gadget) {
    if (gadget == 0 || gadget == 1) return gadget;
    if ((gadget & ~0xff) == 0x100 && (gadget & 0xff) >= 1 && (gadget & 0xff) <= (int)MAX_WIDTH) return gadget & 0xff;
    return -1;
}

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
    G.w = base2 ? 1u : 0u;
    return G;
}

// ceil(ceil(log2 q) / w): the number of base-2^w digits of a limb of modulus q, the smallest k with 2^(w k) >= q.
inline uint32_t digits_pow2(uint64_t q, uint32_t w) { return (digits_base2(q) + w - 1) / w; }

// BaseBGad 2^w, 1 <= w <= MAX_WIDTH.  w = 1 is make_layout(q, L, true).
inline Layout make_layout_pow2(const uint64_t* q, int L, uint32_t w) {
    Layout G;
    uint32_t D = 0;
    for (int i = 0; i <= MAX_LIMBS; ++i) {
        G.first[i] = D;
        if (i < L) D += digits_pow2(q[i], w);
    }
    G.L = (uint32_t)L;
    G.D = D;
    G.w = w;
    return G;
}

// The layout of a gadget code gadget_width() accepts.
inline Layout make_layout_code(const uint64_t* q, int L, int gadget) {
    const int w = gadget_width(gadget);
    return w <= 1 ? make_layout(q, L, w == 1) : make_layout_pow2(q, L, (uint32_t)w);
}

// ---- the digits of BaseBGad b, b = 2^w, without walking them in sequence ----------------------------------------------------
// divModCent takes the remainder r of v mod b in [-b/2, b/2) and goes on with (v - r) / b; the top digit absorbs what is left.
// Adding b/2 before a floor division centres the remainder, so after t steps the running value is
//     v_t = (v + c_t) >> (w t)   (arithmetic shift),   c_t = (b/2) (1 + b + ... + b^(t-1)) = (b/2) (b^t - 1) / (b - 1),
// digit t < k - 1 is ((v_t + b/2) & (b - 1)) - b/2 and the top digit is v_(k-1).  c_t <= b^t - 1 <= 2^(w (k - 1)) - 1 < q - 1 and
// |v| <= (q - 1) / 2, so v + c_t fits the signed word for q < 2^31 (32-bit) and q < 2^62 (64-bit).  For w = 1 this is
// -((u >> t) & 1) with u = -v, the expression of the base-2 loaders.
// SW: int32_t or int64_t.  t is uniform over a workgroup in the transforms' loaders, so c_t costs a few scalar steps there.
template <typename SW>
ALCH_GADGET_HD SW pow2_offset(uint32_t w, uint32_t t) {
    SW c = 0;
    for (uint32_t s = 0; s < t; ++s) c = (SW)(c << w) | (SW)((SW)1 << (w - 1));
    return c;
}

// Digit t of the centred lift v; ct = pow2_offset(w, t); top: t is the limb's last digit.
template <typename SW>
ALCH_GADGET_HD SW pow2_digit(SW v, uint32_t w, uint32_t t, bool top, SW ct) {
    const SW vt = (SW)(v + ct) >> (w * t);
    const SW half = (SW)1 << (w - 1);
    return top ? vt : (SW)(((vt + half) & (SW)(((SW)1 << w) - 1)) - half);
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
