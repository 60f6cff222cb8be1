// AddressSanitizer / UndefinedBehaviorSanitizer program for the three-instruction Plantard product and the butterflies built on it
// (alchemy_amd/csrc/modarith.hpp: plant_close, plant_mul3, bfly_fwd(u32&, u32&, u64 br, ...), bfly_inv(u32&, u32&, u64 br, ...),
// bfly_inv_entry).  The functions are the header's, which the kernels include.  Checked here:
//   * plant_mul3(a, const(c)) is a c mod q as a value in [0, q], and the SAME WORD as the four-instruction plant_mul, for any word a;
//   * the closing step alone at t1 = 2^32 - 1 gives q (plant_mul wraps to 0 there: the one place the two forms differ);
//   * the 7-instruction forward butterfly is congruent to the Montgomery bfly_fwd and stays below 2q, with t = q forced through the
//     closing step as well;
//   * the inverse pair (entry form on [0,2q), steady form on [0, q], both inputs equal to q included) is congruent to bfly_inv and
//     stays within [0, q].
// Stand-alone: built and run by tests/test_plant3.py; it needs neither the library nor a device.
#include <cstdint>
#include <cstdio>

#include "../../alchemy_amd/csrc/modarith.hpp"

using alch::csub;
using alch::u32;
using alch::u64;

static long failed = 0, t_is_q = 0;
#define EXPECT(c) do { if (!(c)) { if (++failed <= 20) printf("FAILED line %d (q = %u, a/x = %u, c/y = %u, w = %u): %s\n", __LINE__, (unsigned)q, (unsigned)x, (unsigned)y, (unsigned)w, #c); } } while (0)

static u64 rng_state = 0x243f6a8885a308d3ull;
static u64 rnd() {                                  // splitmix64
    u64 z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// a any word, c < q
static void one_mul(u32 x, u32 y, u32 q) {
    const u32 w = 0;
    const u64 br = alch::h_plant_const(y, q);
    const u32 got = alch::plant_mul3(x, br, q), old = alch::plant_mul(x, br, q);
    const u32 want = (u32)(((u64)x * y) % q);
    EXPECT(got <= q);
    EXPECT(got % q == want);
    EXPECT(got == old);                              // the same word: a table constant never leads to t1 = 2^32 - 1
}

// x in [0,2q), y any word, w < q (plain residue): against the Montgomery butterfly with w R
static void one_fwd(u32 x, u32 y, u32 w, u32 q, const alch::ModP<u32>& m) {
    u32 a = x, b = y, c = x, d = (u32)(y % (2ull * q));                      // the Montgomery side gets a [0,2q) word congruent to y
    alch::bfly_fwd(a, b, alch::h_plant_const(w, q), q, m.qni);
    alch::bfly_fwd(c, d, (u32)alch::h_mulmod(w, m.r1, q), q, m.qni);
    EXPECT(a < 2u * q && b < 2u * q);
    EXPECT(a % q == c % q && b % q == d % q);
}
// the same butterfly with the product replaced by the closing step at t1 = 2^32 - 1, i.e. t = q (what a zero product may come out as)
static void one_fwd_t_q(u32 x, u32 q) {
    const u32 y = 0, w = 0;
    const u32 t = alch::plant_close(0xffffffffu, q);
    EXPECT(t == q);
    ++t_is_q;
    u32 xo = x, yo = y;
    alch::bfly_fwd_from_t(xo, yo, t, q);             // the header's own legs, the ones bfly_fwd runs
    EXPECT(xo < 2u * q && yo < 2u * q);
    EXPECT(xo % q == x % q && yo % q == x % q);      // t = 0 (mod q): both legs are x
}

// steady form: x, y in [0, q]; entry form: x, y in [0,2q).  Against bfly_inv on reduced-lazy inputs.
static void one_inv(u32 x, u32 y, u32 w, u32 q, const alch::ModP<u32>& m, bool entry) {
    u32 a = x, b = y, c = x, d = y;
    const u64 br = alch::h_plant_const(w, q);
    if (entry) alch::bfly_inv_entry(a, b, br, q, m.qni);
    else alch::bfly_inv(a, b, br, q, m.qni);
    alch::bfly_inv(c, d, (u32)alch::h_mulmod(w, m.r1, q), q, m.qni);          // x, y <= q < 2q: inside its domain
    EXPECT(a <= q && b <= q);
    EXPECT(a % q == c % q && b % q == d % q);
    EXPECT(a % q == (u32)(((u64)x + y) % q));
    EXPECT(b % q == (u32)(((((u64)x % q) + q - (y % q)) % q) * w % q));
}

static void check_modulus(u32 q) {
    const alch::ModP<u32> m = alch::make_modp<u32>(q);
    const u32 q2 = 2u * q;
    const u32 as[8] = {0, 1, q - 1, q, q + 1, q2 - 1, q2, 0xffffffffu};
    const u32 cs[4] = {0, 1, q - 1, m.r1};
    u32 x = 0, y = 0, w = 0;
    for (u32 a : as)
        for (u32 c : cs) one_mul(a, c, q);
    for (int it = 0; it < 100000; ++it) {
        const u64 r = rnd();
        one_mul((u32)r, (u32)((r >> 32) % q), q);
    }
    // the closing step alone
    EXPECT(alch::plant_close(0xffffffffu, q) == q);
    EXPECT(alch::plant_close(0u, q) == 0u);
    EXPECT(alch::plant_close(0xfffffffeu, q) == q - 1);                          // floor((2^32 - 1) q / 2^32) = q - 1
    // forward butterfly
    const u32 xs[6] = {0, 1, q - 1, q, q + 1, q2 - 1};
    for (u32 ww : cs)
        for (u32 xx : xs) {
            for (u32 yy : as) one_fwd(xx, yy, ww, q, m);
        }
    for (u32 xx : xs) one_fwd_t_q(xx, q);
    for (int it = 0; it < 100000; ++it) {
        const u64 r = rnd();
        one_fwd((u32)(r % q2), (u32)(r >> 32), (u32)(rnd() % q), q, m);
    }
    // inverse butterflies
    const u32 steady[5] = {0, 1, q - 1, q, q / 2};
    for (u32 ww : cs)
        for (u32 xx : steady)
            for (u32 yy : steady) one_inv(xx, yy, ww, q, m, false);
    for (u32 ww : cs)
        for (u32 xx : xs)
            for (u32 yy : xs) one_inv(xx, yy, ww, q, m, true);
    for (int it = 0; it < 100000; ++it) {
        const u64 r = rnd();
        one_inv((u32)(r % ((u64)q + 1)), (u32)((r >> 32) % ((u64)q + 1)), (u32)(rnd() % q), q, m, false);
        const u64 s = rnd();
        one_inv((u32)(s % q2), (u32)((s >> 32) % q2), (u32)(rnd() % q), q, m, true);
    }
}

int main() {
    const u32 qs[] = {2147352577u, 2146959361u, 2146041857u, 2145976321u, 1073479681u};
    for (u32 q : qs) check_modulus(q);
    printf("t = q cases: %ld\n", t_is_q);
    printf("OK: %ld failed expectation(s)\n", failed);
    return failed ? 1 : 0;
}
