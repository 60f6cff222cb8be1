// The counter-based error sampler of the encrypt path, the part the device kernels (kernel_rlwe.hpp), the library's
// host-only entry points (alch_gauss_table, alch_gauss_plan) and the C++ host mirror (alchemy_amd/host/cycgen.hpp) share.  Plain
// C++: it compiles with hipcc and with a host compiler alone (tests/sanitize/gauss_harness.cpp).
//
// Every stored word is an integer-exact function of (seed, position): a discrete Gaussian K ~ D_{Z,64} from a cumulative table by
// one 63-bit comparison value, 32 uniform bits below it, one multiplication by `scale`, the Cholesky factors of p I - J along the odd
// axes of the index with every product and every sum rounded on its own (no fused multiply-add anywhere), one rounding.
//
// QUALITY.  The generator is splitmix64 on a counter: a STATISTICAL generator, not a cryptographic one, like the std::mt19937_64 of the
// host path it stands beside.  Nothing here is fit to protect real data -- a ring with a key (alch_ring_set_rng_key) replaces the two
// words of a coefficient by a pair of a ChaCha20 keystream (chacha_stream.hpp); everything behind the words stays.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "gauss_cdt.inc.hpp"

#if defined(__HIPCC__)
#define ALCH_HD __host__ __device__
#else
#define ALCH_HD
#endif

namespace alch {
namespace gauss {

constexpr uint32_t CDT_LEN = ALCH_GAUSS_CDT_LEN;                  // 582: T[580] = 2^63 - 2, T[581] = 2^63 - 1
static const uint64_t CDT[CDT_LEN] = {ALCH_GAUSS_CDT_VALUES};     // T[t] = floor(2^63 P(|K| <= t)), K ~ D_{Z,64}
constexpr uint32_t MAX_ODD_PRIME = 13;                            // the axis kernels are instantiated for p in {3, 5, 7, 11, 13}

// the splitmix64 of alch_buf_fill_uniform (alchemy_hip.hip)
ALCH_HD inline uint64_t mix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// One correctly rounded double operation each.  hipcc contracts a*b+c into a fused multiply-add by default, across statements and
// through the __dmul_rn / __dadd_rn of its headers (plain a*b and a+b there): the pragma takes the `contract` flag off the operation
// itself, so no neighbour can fuse with it.  Other host compilers get the result through a volatile temporary.
#if defined(__clang__)
ALCH_HD inline double rn_mul(double a, double b) {
#pragma clang fp contract(off)
    return a * b;
}
ALCH_HD inline double rn_add(double a, double b) {
#pragma clang fp contract(off)
    return a + b;
}
ALCH_HD inline double rn_sub(double a, double b) {
#pragma clang fp contract(off)
    return a - b;
}
ALCH_HD inline double rn_div(double a, double b) {
#pragma clang fp contract(off)
    return a / b;
}
#else
inline double rn_mul(double a, double b) { volatile double t = a * b; return t; }
inline double rn_add(double a, double b) { volatile double t = a + b; return t; }
inline double rn_sub(double a, double b) { volatile double t = a - b; return t; }
inline double rn_div(double a, double b) { volatile double t = a / b; return t; }
#endif

// (w0, w1) -> f = k 2^32 + (w1 >> 32) - 2^31: k = +-#{ j : T[j] <= w0 >> 1 } with the sign from bit 0 of w0, by a fixed 10-step
// binary search (CDT_LEN < 2^10).  |f| < 2^42, so (double)f is exact.  T: the table, wherever the caller keeps it (LDS on the device).
ALCH_HD inline int64_t deviate(uint64_t w0, uint64_t w1, const uint64_t* T) {
    const uint64_t u = w0 >> 1;
    uint32_t t = 0;
    for (uint32_t step = 512; step; step >>= 1) {
        const uint32_t c = t + step;
        if (c <= CDT_LEN && T[c - 1] <= u) t = c;
    }
    const int64_t k = (w0 & 1) ? -(int64_t)t : (int64_t)t;
    return k * ((int64_t)1 << 32) + (int64_t)(w1 >> 32) - ((int64_t)1 << 31);
}

// Coefficient with counter c of the stream `seed`, before the correlation: (double)f * scale.
ALCH_HD inline double sample(uint64_t seed, uint64_t c, double scale, const uint64_t* T) {
    const int64_t f = deviate(mix64(seed + 2 * c), mix64(seed + 2 * c + 1), T);
    return rn_mul((double)f, scale);
}

// R(x) = sign(x) floor(|x| + 0.5), the addition in double.
ALCH_HD inline int64_t round_half_away(double x) {
    const double a = x < 0 ? -x : x;
    const int64_t r = (int64_t)std::floor(rn_add(a, 0.5));
    return x < 0 ? -r : r;
}

// errorRounded (p = 0): R(x).  errorCoset: the element of v + p Z nearest to x, v in [0, p) taken centred -- c + p R((x - c) / p).
ALCH_HD inline int64_t round_coset(double x, uint32_t p, uint32_t v) {
    if (p == 0) return round_half_away(x);
    const int64_t c = v > (p - 1) / 2 ? (int64_t)v - (int64_t)p : (int64_t)v;      // centred(v, p) of cycgen.hpp
    return c + (int64_t)p * round_half_away(rn_div(rn_sub(x, (double)c), (double)p));
}

// z mod q in [0, q); q = 0 (the integers): z itself as a two's-complement word.  |z| < 2^62 and q < 2^62.
ALCH_HD inline uint64_t reduce(int64_t z, uint64_t q) {
    if (q == 0) return (uint64_t)z;
    const int64_t sq = (int64_t)q;
    if (z < sq && z > -sq) return (uint64_t)(z < 0 ? z + sq : z);
    const int64_t r = z % sq;
    return (uint64_t)(r < 0 ? r + sq : r);
}

// ---- the plan of an index: scale and the Cholesky factors, host only -----------------------------------------------------------
struct Axis {
    uint32_t p, mp, stride;                    // prime, m_p' = p^(e-1), stride of the axis in the element
    std::vector<double> Lc;                    // lower Cholesky factor of p I - J, (p-1) x (p-1), row-major, zeros above the diagonal
};
struct Plan {
    uint32_t m = 0, n = 0;
    double scale = 0;
    std::vector<Axis> axes;                    // the ODD primes of m, ascending (p = 2 is the identity)
    double norm = 1;                           // product over the axes of max_i sum_k |Lc[i][k]|
};

inline bool svar_ok(double svar) { return std::isfinite(svar) && svar > 0; }

// The loop of tGaussianDec (cycgen.hpp): sigma, the Cholesky factors and the strides, with every operation rounded on its own.
inline Plan make_plan(uint32_t m, double svar) {
    Plan P;
    P.m = m;
    std::vector<std::pair<uint32_t, int>> fs;
    for (uint32_t t = m, p = 2; t > 1; ++p) {
        if ((uint64_t)p * p > t) p = t;
        if (t % p == 0) { int e = 0; while (t % p == 0) { t /= p; ++e; } fs.push_back({p, e}); }
    }
    uint32_t rad = 1, n = 1;
    for (auto& f : fs) { rad *= f.first; n *= f.first - 1; for (int e = 1; e < f.second; ++e) n *= f.first; }
    P.n = n;
    const double pi = 3.14159265358979323846;
    const double sigma = std::sqrt(rn_div(rn_mul(svar, (double)(m / rad)), rn_mul(2.0, pi)));
    P.scale = rn_div(sigma, rn_mul(std::sqrt(rn_add(4096.0, rn_div(1.0, 12.0))), 4294967296.0));
    uint32_t stride = n;
    for (auto& f : fs) {
        const uint32_t p = f.first;
        uint32_t mp = 1;
        for (int e = 1; e < f.second; ++e) mp *= p;
        stride /= (p - 1) * mp;
        if (p == 2) continue;
        const uint32_t h = p - 1;
        Axis a;
        a.p = p; a.mp = mp; a.stride = stride;
        a.Lc.assign((size_t)h * h, 0.0);
        double worst = 0;
        for (uint32_t i = 0; i < h; ++i) {
            double row = 0;
            for (uint32_t j = 0; j <= i; ++j) {
                double s = (i == j ? (double)p - 1.0 : -1.0);
                for (uint32_t k = 0; k < j; ++k) s = rn_sub(s, rn_mul(a.Lc[i * h + k], a.Lc[j * h + k]));
                a.Lc[i * h + j] = i == j ? std::sqrt(s) : rn_div(s, a.Lc[j * h + j]);
                row += std::fabs(a.Lc[i * h + j]);
            }
            worst = std::max(worst, row);
        }
        P.norm *= worst;
        P.axes.push_back(std::move(a));
    }
    return P;
}

// A bound on |z| of every coefficient the plan can produce, as a double (generous: it only has to stay below 2^62).
// |f| < 583 * 2^32; the correlation multiplies by at most `norm`; the coset rounding moves by at most p.
inline double z_bound(const Plan& P, uint32_t p) {
    return P.scale * (583.0 * 4294967296.0) * P.norm * 1.000001 + 2.0 * (double)p + 2.0;
}
inline bool bound_ok(const Plan& P, uint32_t p) { const double b = z_bound(P, p); return std::isfinite(b) && b < 4611686018427387904.0; }

// Element `elem`: n integers z (Dec basis), the two words of coefficient c = elem n + i from words(c, w0, w1).  coset: n words in
// [0, p), or null with p = 0 (errorRounded).
template <typename F>
inline void element_from(const Plan& P, F&& words, uint64_t elem, uint32_t p, const uint32_t* coset, int64_t* z) {
    const uint32_t n = P.n;
    std::vector<double> x(n);
    for (uint32_t i = 0; i < n; ++i) {
        uint64_t w0, w1;
        words(elem * (uint64_t)n + i, w0, w1);
        x[i] = rn_mul((double)deviate(w0, w1, CDT), P.scale);
    }
    for (const Axis& a : P.axes) {
        const uint32_t h = a.p - 1, dim = h * a.mp;
        std::vector<double> cv(h);
        for (uint32_t base = 0; base < n; ++base) {
            if ((base / a.stride) % dim >= a.mp) continue;                      // one visit per column: j0 = 0
            for (uint32_t i = 0; i < h; ++i) cv[i] = x[base + (size_t)i * a.mp * a.stride];
            for (uint32_t i = h; i-- > 0;) {
                double s = 0.0;
                for (uint32_t k = 0; k <= i; ++k) { const double t = rn_mul(a.Lc[i * h + k], cv[k]); s = rn_add(s, t); }
                x[base + (size_t)i * a.mp * a.stride] = s;
            }
        }
    }
    for (uint32_t i = 0; i < n; ++i) z[i] = round_coset(x[i], p, coset ? coset[i] : 0u);
}

// Element `elem` of the splitmix64 stream `seed`.
inline void element(const Plan& P, uint64_t seed, uint64_t elem, uint32_t p, const uint32_t* coset, int64_t* z) {
    element_from(P, [seed](uint64_t c, uint64_t& w0, uint64_t& w1) { w0 = mix64(seed + 2 * c); w1 = mix64(seed + 2 * c + 1); }, elem, p,
                 coset, z);
}

}  // namespace gauss
}  // namespace alch
