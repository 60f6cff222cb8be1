// Host-only arithmetic of the plaintext-side entry points (include/alchemy_hip.h, "EXACTNESS"): the coefficient bound and the test
// Q / 2 > bound.  Plain C++ with no dependency on the HIP runtime or the kernel headers, so that it also compiles into a stand-alone
// sanitizer program (tests/sanitize/plain_bound_harness.cpp).
#pragma once
#include <stdint.h>

namespace alch {

typedef unsigned __int128 u128;

// phi(m) and the number of odd primes of m, by trial division (m is a 32-bit cyclotomic index).
inline void pt_index_shape(uint32_t m, uint64_t* phi, int* odd) {
    uint64_t f = 1;
    int w = 0;
    uint32_t rem = m;
    for (uint32_t p = 2; (uint64_t)p * p <= rem; p += (p == 2 ? 1 : 2)) {
        if (rem % p) continue;
        if (p != 2) ++w;
        f *= p - 1;
        rem /= p;
        while (rem % p == 0) { rem /= p; f *= p; }
    }
    if (rem > 1) { f *= rem - 1; if (rem != 2) ++w; }
    *phi = f;
    *odd = w;
}

// terms * phi(m) * 2^(odd primes of m) * floor(p/2)^2.  false when an argument is out of range: m >= 1, 2 <= p < 2^31,
// 1 <= terms <= 65536.  Then terms phi(m) < 2^48, at most 9 odd primes fit a 32-bit index, floor(p/2)^2 < 2^60: the bound is below 2^117.
inline bool pt_bound_value(uint32_t m, uint64_t p, uint64_t terms, u128* out) {
    if (m < 1 || p < 2 || p >= ((uint64_t)1 << 31) || terms < 1 || terms > 65536) return false;
    uint64_t phi = 0;
    int odd = 0;
    pt_index_shape(m, &phi, &odd);
    const uint64_t h = p / 2;
    u128 b = (u128)terms * phi;
    b <<= odd;
    b *= (u128)(h * h);
    *out = b;
    return true;
}

// prod q_j > 2 b, decided without forming a product that could wrap: Q' q > 2 b  <=>  Q' > floor(2 b / q).  b < 2^126; every q_j >= 1.
inline bool pt_q_exceeds(const uint64_t* q, int L, u128 b) {
    u128 Q = 1;
    for (int j = 0; j < L; ++j) {
        if (q[j] == 0) return false;
        if (Q > (2 * b) / q[j]) return true;                      // the remaining limbs only make Q larger
        Q *= q[j];                                                // <= 2 b
    }
    return false;
}

}  // namespace alch
