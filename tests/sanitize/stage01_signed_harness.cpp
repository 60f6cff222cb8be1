// AddressSanitizer / UndefinedBehaviorSanitizer program for stage01_signed (alchemy_amd/csrc/modarith.hpp): stages 0-1 of the
// key-switch kernel's pass G as one signed multiply-add chain over four centred digits, checked against __int128 arithmetic.
// Stand-alone: built and run by tests/test_stage01_signed.py; it needs neither the library nor a device.  stage01_signed,
// centre_const and mont_mul are the header's, which the kernel includes; the constants are formed here as kernel_ks_half.hpp
// forms them (c0 = R, c2 = s w1, c1 = w2, c3 = s w1 w2 in Montgomery form, centred, negated for the negated digit).
#include <cstdint>
#include <cstdio>

#include "../../alchemy_amd/csrc/modarith.hpp"

using alch::u32;
using alch::u64;
typedef __int128 i128;

static long failed = 0;
static long checked = 0;
#define EXPECT(c) do { if (!(c)) { if (++failed <= 20) printf("FAILED line %d (q = %u): %s\n", __LINE__, (unsigned)q, #c); } } while (0)

static u64 rng_state = 0x9e3779b97f4a7c15ull;
static u64 rnd() {                                  // splitmix64
    u64 z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

static u64 mod_q(i128 v, u32 q) { return (u64)(((v % q) + q) % q); }

struct Consts {
    int32_t c0, c1, c2, c3;
    u64 w1, w2;         // the residues the two Montgomery words stand for
    int sigma, sign;    // half (+1 lower, -1 upper) and the sign of the whole map (-1: the negated digit is transformed)
};

static Consts make_consts(const alch::ModP<u32>& m, u32 tw1, u32 tw2, int hf, bool neg, u64 rinv) {
    const u32 q = m.q;
    const u32 w1s = hf ? q - tw1 : tw1;
    Consts c;
    c.c0 = alch::centre_const(m.r1, q, neg);
    c.c1 = alch::centre_const(tw2, q, neg);
    c.c2 = alch::centre_const(w1s, q, neg);
    c.c3 = alch::centre_const(alch::mont_mul(w1s, tw2, m), q, neg);
    c.w1 = (u64)tw1 * rinv % q;
    c.w2 = (u64)tw2 * rinv % q;
    c.sigma = hf ? -1 : 1;
    c.sign = neg ? -1 : 1;
    return c;
}

static void check_one(const alch::ModP<u32>& m, const Consts& c, const int32_t x[4]) {
    const u32 q = m.q;
    ++checked;
    // preconditions of the helper
    const int32_t half = (int32_t)((q - 1) >> 1);
    for (int k = 0; k < 4; ++k) EXPECT(x[k] > -((int32_t)1 << 30) && x[k] < ((int32_t)1 << 30));
    EXPECT(c.c0 >= -half && c.c0 <= half && c.c1 >= -half && c.c1 <= half && c.c2 >= -half && c.c2 <= half && c.c3 >= -half && c.c3 <= half);
    // the sums in wide arithmetic: positive, below q 2^32 (the reduction's bound), so nothing wraps in 64 bits either
    const i128 C = (i128)q << 31;
    const i128 S = C + (i128)x[0] * c.c0 + (i128)x[2] * c.c2, T = (i128)x[1] * c.c1 + (i128)x[3] * c.c3;
    const i128 lim = (i128)q << 32;
    EXPECT(S + T > 0 && S + T < lim && S - T > 0 && S - T < lim);
    EXPECT(S > INT64_MIN && S < INT64_MAX && T > INT64_MIN && T < INT64_MAX);
    const u32 mp = (u32)(u64)(S + T) * m.qni, mm = (u32)(u64)(S - T) * m.qni;
    EXPECT(S + T + (i128)mp * q < ((i128)1 << 64) && S - T + (i128)mm * q < ((i128)1 << 64));
    u32 y0 = 0, y2 = 0;
    alch::stage01_signed(x[0], x[1], x[2], x[3], c.c0, c.c1, c.c2, c.c3, q, m.qni, y0, y2);
    EXPECT(y0 < 2 * (u64)q && y2 < 2 * (u64)q);
    // u = x0 + s w1 x2, v = x1 + s w1 x3, y0 = +-(u + w2 v), y2 = +-(u - w2 v)
    const i128 u = (i128)x[0] + c.sigma * (i128)c.w1 * x[2], v = (i128)x[1] + c.sigma * (i128)c.w1 * x[3];
    const u64 vr = mod_q(v, q);
    EXPECT(y0 % q == mod_q(c.sign * (u + (i128)c.w2 * vr), q));
    EXPECT(y2 % q == mod_q(c.sign * (u - (i128)c.w2 * vr), q));
}

// digits are centred lifts of a modulus qd (any limb of the ring, not only q itself)
static void check_modulus(u32 q, u32 qd) {
    const alch::ModP<u32> m = alch::make_modp<u32>(q);
    const u64 rinv = alch::h_powmod(m.r1, (u64)q - 2, q);              // R^-1 mod q
    const int32_t hd = (int32_t)((qd - 1) / 2);
    const int32_t ext[6] = {0, 1, -1, hd, -hd, hd - 1};                 // centred 0, 1, qd-1, (qd-1)/2, (qd+1)/2, (qd-3)/2
    // twiddle words: the ones whose centred form sits on the ends of the range, and random ones
    const u32 tws[6][2] = {{1, 1}, {(q - 1) / 2, (q + 1) / 2}, {(q + 1) / 2, (q + 1) / 2}, {q - 1, (q - 1) / 2},
                           {(u32)(1 + rnd() % (q - 1)), (u32)(1 + rnd() % (q - 1))}, {(u32)(1 + rnd() % (q - 1)), (u32)(1 + rnd() % (q - 1))}};
    for (const auto& tw : tws)
        for (int hf = 0; hf < 2; ++hf)
            for (int neg = 0; neg < 2; ++neg) {
                const Consts c = make_consts(m, tw[0], tw[1], hf, neg != 0, rinv);
                for (int i = 0; i < 6 * 6 * 6 * 6; ++i) {
                    const int32_t x[4] = {ext[i % 6], ext[i / 6 % 6], ext[i / 36 % 6], ext[i / 216]};
                    check_one(m, c, x);
                }
                for (int it = 0; it < 500; ++it) {                      // uniform digits, some coordinates on an extreme
                    int32_t x[4];
                    for (int k = 0; k < 4; ++k) {
                        const u64 r = rnd();
                        x[k] = (r & 3) == 0 ? ext[(r >> 2) % 6] : (int32_t)((r >> 8) % qd) - hd;
                    }
                    check_one(m, c, x);
                }
            }
}

int main() {
    const u32 qs[] = {2147352577u, 2146959361u, 2146041857u, 2145976321u,      // the headline's four moduli
                      2147483647u,                                             // just below 2^31
                      1073479681u,                                             // below 2^30
                      65537u, 786433u};                                        // small limbs of an unbalanced set
    for (u32 q : qs) {
        check_modulus(q, q);
        check_modulus(q, 2147483647u);                                         // the largest digits any limb can send: |z| <= 2^30 - 1
        check_modulus(q, 65537u);
    }
    printf("OK: %ld failed expectation(s), %ld cases\n", failed, checked);
    return failed ? 1 : 0;
}
