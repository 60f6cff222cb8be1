// Galois automorphisms sigma_j : zeta_m -> zeta_m^j on the CRT basis: the slot permutation, by definition.
//
// sigma_j fixes Z_q, so on the CRT basis (slot(u) holds a(omega_m^u), the rule at the top of include/alchemy_hip.h) it only moves
// slots:  crt(sigma_j a)[slot(u)] = (sigma_j a)(omega^u) = a(omega^(u j)) = crt(a)[slot(u j mod m)].  The table below is that
// statement: src[k] = slot(unit(k) * j mod m), the SOURCE slot of destination slot k.  It is the same for every limb (the slot rule
// does not look at q) and factorises over the prime-power axes m_l = p^e of m (first factor outermost): unit(k) is fixed by its
// residues u_l mod m_l, and u j mod m_l = u_l (j mod m_l).  Per axis, slot s_l = (i0 - 1) p^(e-1) + digitrev_p(i1) holds the unit
// u_l = i0 + p i1; for p = 2 that is u = 2 brev(s) + 1, the two-power rule.
//
// Standard headers only: a host compiler compiles this file alone (tests/sanitize/automorph_harness.cpp); alchemy_hip.hip uses
// build_table for the general-index engine, and kernel_automorph.hpp uses pow2_src -- the closed form of the same table for a
// two-power index -- per lane.
#pragma once
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define ALCH_AUTO_HD __host__ __device__
#else
#define ALCH_AUTO_HD
#endif
#if defined(__has_builtin)
#if __has_builtin(__builtin_bitreverse32)
#define ALCH_AUTO_HAS_BITREVERSE 1        // clang on the host as well: the sweep of tests/sanitize/hoist_harness.cpp evaluates it 10^10 times
#endif
#endif
#ifndef ALCH_AUTO_HAS_BITREVERSE
#define ALCH_AUTO_HAS_BITREVERSE 0
#endif

namespace alch {
namespace automorph {

constexpr int MAXAX = 8;

struct Axis {
    uint32_t p, e, mp, ml, dim, rts;    // prime, exponent, p^(e-1), p^e, (p-1) p^(e-1), stride of the axis in the slot index
};
struct Plan {
    uint32_t m = 0, n = 0;
    int nax = 0;
    Axis ax[MAXAX];
};

enum { PLAN_OK = 0, PLAN_INVALID = 1, PLAN_UNSUPPORTED = 2 };

// Factor m (prime powers ascending, first outermost) under the predicate of alch_ring_create without its word-size test: a
// two-power index >= 32 runs on the radix-16 engine up to m = 2^17; any other index on the pass engine, whose odd primes are <= 13
// and whose dimension is indexed with 16-bit quantities.
inline int plan(uint32_t m, Plan& P) {
    P = Plan();
    if (m < 1) return PLAN_INVALID;
    P.m = m;
    const bool pow2 = (m & (m - 1)) == 0;
    if (pow2 && m > (1u << 17)) return PLAN_UNSUPPORTED;
    uint32_t rem = m;
    uint64_t n = 1;
    for (uint32_t p = 2; rem > 1; p += (p == 2 ? 1 : 2)) {
        if (p > 13) return PLAN_UNSUPPORTED;
        if (rem % p) continue;
        Axis& a = P.ax[P.nax++];
        a.p = p; a.e = 0; a.mp = 1;
        while (rem % p == 0) { rem /= p; if (a.e++) a.mp *= p; }
        a.ml = a.mp * p;
        a.dim = (p - 1) * a.mp;
        n *= a.dim;
    }
    if (!(pow2 && m >= 32) && n > 65535) return PLAN_UNSUPPORTED;
    P.n = (uint32_t)n;
    uint32_t s = P.n;
    for (int l = 0; l < P.nax; ++l) { s /= P.ax[l].dim; P.ax[l].rts = s; }
    return PLAN_OK;
}

inline uint32_t digitrev(uint32_t x, uint32_t p, uint32_t digits) {
    uint32_t r = 0;
    for (uint32_t t = 0; t < digits; ++t) { r = r * p + x % p; x /= p; }
    return r;
}
// the unit mod p^e behind slot s of one axis, and the slot that holds unit u
inline uint32_t axis_unit(const Axis& a, uint32_t s) { return (s / a.mp + 1 + a.p * digitrev(s % a.mp, a.p, a.e - 1)) % a.ml; }
inline uint32_t axis_slot(const Axis& a, uint32_t u) { return (u % a.p - 1) * a.mp + digitrev(u / a.p, a.p, a.e - 1); }

inline uint32_t gcd(uint32_t a, uint32_t b) {
    while (b) { const uint32_t t = a % b; a = b; b = t; }
    return a;
}

// out[k] = source slot of destination slot k under sigma_j, k < phi(m).  false: j is not a unit mod m.
inline bool build_table(const Plan& P, uint32_t j, std::vector<uint32_t>& out) {
    j %= P.m;
    if (gcd(j, P.m) != 1) return false;
    std::vector<uint32_t> per[MAXAX];
    for (int l = 0; l < P.nax; ++l) {
        const Axis& a = P.ax[l];
        const uint64_t jl = j % a.ml;
        per[l].resize(a.dim);
        for (uint32_t s = 0; s < a.dim; ++s) per[l][s] = axis_slot(a, (uint32_t)((uint64_t)axis_unit(a, s) * jl % a.ml)) * a.rts;
    }
    out.assign(P.n, 0);
    for (uint32_t k = 0; k < P.n; ++k) {
        uint32_t src = 0;
        for (int l = 0; l < P.nax; ++l) src += per[l][(k / P.ax[l].rts) % P.ax[l].dim];
        out[k] = src;
    }
    return true;
}

// The low `bits` bits of x reversed (bits <= 32; 0 gives 0).
ALCH_AUTO_HD inline uint32_t brev_bits(uint32_t x, int bits) {
#if defined(__HIP_DEVICE_COMPILE__) || ALCH_AUTO_HAS_BITREVERSE
    return bits ? __builtin_bitreverse32(x) >> (32 - bits) : 0u;      // what __brev is: v_bfrev_b32, without the HIP runtime header
#else
    uint32_t r = 0;
    for (int t = 0; t < bits; ++t) r |= ((x >> t) & 1u) << (bits - 1 - t);
    return r;
#endif
}

// Two-power index m = 2n = 2^(logn + 1): slot k holds the unit 2 brev(k) + 1, so the source slot of k is brev(((2 brev(k) + 1) j mod
// 2n - 1) / 2).  j odd, reduced or not: the product is taken mod 2^32 and masked, and 2n divides 2^32.  What build_table gives for
// such an index (the harness compares them), without a table.
ALCH_AUTO_HD inline uint32_t pow2_src(uint32_t k, uint32_t j, int logn) {
    const uint32_t u = 2u * brev_bits(k, logn) + 1u;
    const uint32_t v = (u * j) & ((2u << logn) - 1u);
    return brev_bits(v >> 1, logn);
}

// The aligned pack of VL destination slots that starts at k0 (VL a power of two, VL | k0, VL <= n): the slots share the low bits of
// brev(k), so their units agree mod 2n / VL and so do the products with j -- all VL source slots lie in ONE aligned pack of VL.
// Returns the first slot of that pack; pick[c] is where in it destination slot k0 + c reads.  The hoisted inner product
// (kernel_hoist.hpp) computes this once per item and reuses it for c0, every digit and every ciphertext of its tile.
template <int VL>
ALCH_AUTO_HD inline uint32_t pow2_pack(uint32_t k0, uint32_t j, int logn, uint32_t (&pick)[VL]) {
    const uint32_t s0 = pow2_src(k0, j, logn);
    pick[0] = s0 & (uint32_t)(VL - 1);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int c = 1; c < VL; ++c) pick[c] = pow2_src(k0 + (uint32_t)c, j, logn) & (uint32_t)(VL - 1);
    return s0 & ~(uint32_t)(VL - 1);
}

}  // namespace automorph
}  // namespace alch
