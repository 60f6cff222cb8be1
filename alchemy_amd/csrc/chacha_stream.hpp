// Keyed ChaCha20 streams for the samplers (include/alchemy_hip.h, "keyed streams"): the block function, the
// addressing (key, nonce, domain, position) -> two 64-bit words, and the reduction of those 128 bits into a modulus.  The part the device
// kernels (kernel_rlwe.hpp), the library's host-only entry point (alch_rng_words) and the C++ host mirror (alchemy_amd/host/cycgen.hpp)
// share.  Plain C++: it compiles with hipcc and with a host compiler alone (tests/sanitize/chacha_harness.cpp).
//
// Block: ChaCha20 in its original layout (64-bit block counter in words 12, 13; 64-bit nonce in words 14, 15), 20 rounds,
// output = working state + input state, u64[t] = word[2t] | word[2t+1] << 32.  Position x < 2^58 of domain d < 256 lives in block
// (d << 56) | (x >> 2) and owns the pair (A, B) = (u64[2s], u64[2s+1]), s = x & 3.
//
// Nothing here is constant time: the reduction branches on its operands (conditional subtractions compile to selects, but nothing
// is promised), and the Gaussian that consumes domain 1 searches a table by value.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define ALCH_CHACHA_HD __host__ __device__
#else
#define ALCH_CHACHA_HD
#endif

namespace alch {
namespace chacha {

constexpr unsigned DOM_GAUSS = 1, DOM_ENCRYPT = 2, DOM_HINT = 3;   // other values are reserved
constexpr unsigned DOMAINS = 256;
constexpr uint64_t X_END = (uint64_t)1 << 58;                      // positions are 0 <= x < 2^58

struct Key { uint32_t k[8]; };                                     // the 32 key bytes as eight little-endian words; a launch argument by value

inline Key load_key(const uint8_t* b) {
    Key K;
    for (int i = 0; i < 8; ++i)
        K.k[i] = (uint32_t)b[4 * i] | (uint32_t)b[4 * i + 1] << 8 | (uint32_t)b[4 * i + 2] << 16 | (uint32_t)b[4 * i + 3] << 24;
    return K;
}

// One v_alignbit on the device.  The builtin is clang's; other host compilers get the shifts.
#if defined(__clang__)
#define ALCH_CHACHA_ROTL(x, r) __builtin_rotateleft32((x), (r))
#else
#define ALCH_CHACHA_ROTL(x, r) (((x) << (r)) | ((x) >> (32 - (r))))
#endif

#define ALCH_CHACHA_QR(a, b, c, d)                                  \
    do {                                                            \
        a += b; d ^= a; d = ALCH_CHACHA_ROTL(d, 16);                \
        c += d; b ^= c; b = ALCH_CHACHA_ROTL(b, 12);                \
        a += b; d ^= a; d = ALCH_CHACHA_ROTL(d, 8);                 \
        c += d; b ^= c; b = ALCH_CHACHA_ROTL(b, 7);                 \
    } while (0)

// The eight 64-bit words of block `counter` of the stream (K, nonce).
ALCH_CHACHA_HD inline void block(const Key& K, uint64_t counter, uint64_t nonce, uint64_t out[8]) {
    const uint32_t i0 = 0x61707865u, i1 = 0x3320646eu, i2 = 0x79622d32u, i3 = 0x6b206574u;
    const uint32_t i12 = (uint32_t)counter, i13 = (uint32_t)(counter >> 32), i14 = (uint32_t)nonce, i15 = (uint32_t)(nonce >> 32);
    uint32_t x0 = i0, x1 = i1, x2 = i2, x3 = i3, x4 = K.k[0], x5 = K.k[1], x6 = K.k[2], x7 = K.k[3], x8 = K.k[4], x9 = K.k[5],
             x10 = K.k[6], x11 = K.k[7], x12 = i12, x13 = i13, x14 = i14, x15 = i15;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        ALCH_CHACHA_QR(x0, x4, x8, x12);
        ALCH_CHACHA_QR(x1, x5, x9, x13);
        ALCH_CHACHA_QR(x2, x6, x10, x14);
        ALCH_CHACHA_QR(x3, x7, x11, x15);
        ALCH_CHACHA_QR(x0, x5, x10, x15);
        ALCH_CHACHA_QR(x1, x6, x11, x12);
        ALCH_CHACHA_QR(x2, x7, x8, x13);
        ALCH_CHACHA_QR(x3, x4, x9, x14);
    }
    out[0] = (uint64_t)(x0 + i0) | (uint64_t)(x1 + i1) << 32;
    out[1] = (uint64_t)(x2 + i2) | (uint64_t)(x3 + i3) << 32;
    out[2] = (uint64_t)(x4 + K.k[0]) | (uint64_t)(x5 + K.k[1]) << 32;
    out[3] = (uint64_t)(x6 + K.k[2]) | (uint64_t)(x7 + K.k[3]) << 32;
    out[4] = (uint64_t)(x8 + K.k[4]) | (uint64_t)(x9 + K.k[5]) << 32;
    out[5] = (uint64_t)(x10 + K.k[6]) | (uint64_t)(x11 + K.k[7]) << 32;
    out[6] = (uint64_t)(x12 + i12) | (uint64_t)(x13 + i13) << 32;
    out[7] = (uint64_t)(x14 + i14) | (uint64_t)(x15 + i15) << 32;
}
#undef ALCH_CHACHA_QR
#undef ALCH_CHACHA_ROTL

// ---- addressing --------------------------------------------------------------------------------------------------------------
ALCH_CHACHA_HD inline uint64_t block_counter(unsigned domain, uint64_t x) { return (uint64_t)domain << 56 | x >> 2; }
ALCH_CHACHA_HD inline unsigned slot(uint64_t x) { return (unsigned)(x & 3); }

// first + count <= 2^58, computed without wrap-around: the positions [first, first + count) all exist.
inline bool range_ok(unsigned __int128 first, unsigned __int128 count) { return first + count <= (unsigned __int128)X_END; }

// The pair of position x: a whole block for one position (the one-word kernels, the host paths).
ALCH_CHACHA_HD inline void pair(const Key& K, uint64_t nonce, unsigned domain, uint64_t x, uint64_t& A, uint64_t& B) {
    uint64_t u[8];
    block(K, block_counter(domain, x), nonce, u);
    const unsigned s = slot(x);
    A = u[0]; B = u[1];                                            // selects, not a run-time index: the block stays in registers
    if (s == 1) { A = u[2]; B = u[3]; }
    if (s == 2) { A = u[4]; B = u[5]; }
    if (s == 3) { A = u[6]; B = u[7]; }
}

// ---- (B 2^64 + A) mod q ------------------------------------------------------------------------------------------------------
// Montgomery constants of one modulus, word type W (u32: R = 2^32, odd q < 2^31; u64: R = 2^64, odd q < 2^62): the fields the device
// ring keeps per limb (modarith.hpp's ModP), so the kernels pass theirs and the host builds its own with make_mod.
template <typename W>
struct Mod { W q, qni, r1, r2; };                                 // modulus, -q^-1 mod R, R mod q, R^2 mod q

// a any word, b < q -> a b R^-1 mod q in [0, q)
ALCH_CHACHA_HD inline uint32_t redc_mul(uint32_t a, uint32_t b, uint32_t q, uint32_t qni) {
    const uint64_t p = (uint64_t)a * b;
    const uint32_t m = (uint32_t)p * qni;
    const uint32_t t = (uint32_t)((p + (uint64_t)m * q) >> 32);
    return t >= q ? t - q : t;
}
ALCH_CHACHA_HD inline uint64_t redc_mul(uint64_t a, uint64_t b, uint64_t q, uint64_t qni) {
    const unsigned __int128 p = (unsigned __int128)a * b;
    const uint64_t m = (uint64_t)p * qni;
    const uint64_t t = (uint64_t)((p + (unsigned __int128)m * q) >> 64);
    return t >= q ? t - q : t;
}
template <typename W>
ALCH_CHACHA_HD inline W add_q(W a, W b, W q) { const W s = a + b; return s >= q ? s - q : s; }   // a, b < q < R / 2

// x R^-1 R^k: the value of word x at weight R^(k-1).  A = A mod q comes from r1, B 2^64 from the next power.
ALCH_CHACHA_HD inline uint64_t reduce128(uint64_t A, uint64_t B, const Mod<uint64_t>& m) {
    return add_q(redc_mul(B, m.r2, m.q, m.qni), redc_mul(A, m.r1, m.q, m.qni), m.q);
}
ALCH_CHACHA_HD inline uint32_t reduce128(uint64_t A, uint64_t B, const Mod<uint32_t>& m) {
    const uint32_t r3 = redc_mul(m.r2, m.r2, m.q, m.qni), r4 = redc_mul(r3, m.r2, m.q, m.qni);      // R^3, R^4 mod q
    const uint32_t lo = add_q(redc_mul((uint32_t)A, m.r1, m.q, m.qni), redc_mul((uint32_t)(A >> 32), m.r2, m.q, m.qni), m.q);
    const uint32_t hi = add_q(redc_mul((uint32_t)B, r3, m.q, m.qni), redc_mul((uint32_t)(B >> 32), r4, m.q, m.qni), m.q);
    return add_q(lo, hi, m.q);
}

// Host: the constants of an odd modulus q (q < 2^31 for 32-bit words, q < 2^62 for 64-bit words).
inline Mod<uint32_t> make_mod32(uint32_t q) {
    Mod<uint32_t> m;
    uint32_t inv = q;                                              // Newton: correct bits double, q q = 1 mod 8
    for (int i = 0; i < 5; ++i) inv *= 2u - q * inv;
    m.q = q; m.qni = 0u - inv;
    m.r1 = (uint32_t)(((uint64_t)1 << 32) % q);
    m.r2 = (uint32_t)((uint64_t)m.r1 * m.r1 % q);
    return m;
}
inline Mod<uint64_t> make_mod64(uint64_t q) {
    Mod<uint64_t> m;
    uint64_t inv = q;
    for (int i = 0; i < 6; ++i) inv *= 2u - q * inv;
    m.q = q; m.qni = 0u - inv;
    m.r1 = (0 - q) % q;                                            // 2^64 mod q
    m.r2 = (uint64_t)((unsigned __int128)m.r1 * m.r1 % q);
    return m;
}

// Host: the uniform residue of position x, whatever the word type the device would use.
inline uint64_t uniform_word(const Key& K, uint64_t nonce, unsigned domain, uint64_t x, uint64_t q) {
    uint64_t A, B;
    pair(K, nonce, domain, x, A, B);
    return q < ((uint64_t)1 << 31) ? reduce128(A, B, make_mod32((uint32_t)q)) : reduce128(A, B, make_mod64(q));
}

// Position of word (limb j, slot k) of the odd element of pair `pair` (alch_ct_encrypt: pair = ct0 + b; hints: ct0 + e) as a plain
// integer, and the end of a call's positions: both in 128 bits, so the caller can refuse a range that would reach 2^58.
inline unsigned __int128 odd_pos_end(unsigned __int128 pair_end, uint32_t L, uint32_t n) { return 2 * pair_end * L * n; }

}  // namespace chacha
}  // namespace alch
