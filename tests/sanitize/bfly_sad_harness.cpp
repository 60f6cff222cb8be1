// AddressSanitizer / UndefinedBehaviorSanitizer program for the forward butterflies of 32-bit rings (alchemy_amd/csrc/modarith.hpp:
// bfly_fwd(u32&, u32&, u32 w, ...) and bfly_fwd4), whose difference leg is written as an absolute difference plus xx
// (gfx950: one v_sad_u32) instead of a subtraction and an addition.  The butterflies are the header's, which the kernels include;
// the previous formulas are restated here and must give the SAME WORDS, not merely congruent ones.  Stand-alone: built and run by
// tests/test_bfly_sad.py; it needs neither the library nor a device.
#include <cstdint>
#include <cstdio>

#include "../../alchemy_amd/csrc/modarith.hpp"

using alch::csub;
using alch::mont_mul_lazy;
using alch::u32;
using alch::u64;

static long failed = 0, t_zero = 0;
#define EXPECT(c) do { if (!(c)) { if (++failed <= 20) printf("FAILED line %d (q = %u, x = %u, y = %u, w = %u): %s\n", __LINE__, (unsigned)q, (unsigned)x, (unsigned)y, (unsigned)w, #c); } } while (0)

static u64 rng_state = 0x9e3779b97f4a7c15ull;
static u64 rnd() {                                  // splitmix64
    u64 z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// the formulas the absolute-difference legs replaced
static void old_bfly_fwd(u32& x, u32& y, u32 w, u32 q, u32 qni) {
    const u32 xx = csub(x, q);
    const u32 t = csub(mont_mul_lazy(y, w, q, qni), q);
    x = xx + t;
    y = xx + (q - t);
}
static void old_bfly_fwd4(u32& x, u32& y, u32 w, u32 q, u32 qni) {
    const u32 q2 = 2u * q;
    const u32 xx = csub(x, q2);
    const u32 t = mont_mul_lazy(y, w, q, qni);
    x = xx + t;
    y = xx + (q2 - t);
}

// x, y in [0,2q), w < q
static void one_fwd(u32 x, u32 y, u32 w, u32 q, u32 qni) {
    u32 a = x, b = y, c = x, d = y;
    alch::bfly_fwd(a, b, w, q, qni);
    old_bfly_fwd(c, d, w, q, qni);
    EXPECT(a == c && b == d);
    EXPECT(a < 2u * q && b <= q + (q - 1) && b >= 1);               // [0,2q); the difference leg is xx + (q - t) with xx, t < q
    if (csub(mont_mul_lazy(y, w, q, qni), q) == 0) {                   // t = 0: the difference leg returns xx + q
        ++t_zero;
        EXPECT(b == csub(x, q) + q);
    }
}
// q < 2^30: x in [0,4q), y ANY word, w < q
static void one_fwd4(u32 x, u32 y, u32 w, u32 q, u32 qni) {
    u32 a = x, b = y, c = x, d = y;
    alch::bfly_fwd4(a, b, w, q, qni);
    old_bfly_fwd4(c, d, w, q, qni);
    EXPECT(a == c && b == d);
    EXPECT((u64)a < 4ull * q && (u64)b <= 4ull * q && b >= 1);         // xx < 2q, t < 2q
    if (mont_mul_lazy(y, w, q, qni) == 0) {
        ++t_zero;
        EXPECT(b == csub(x, 2u * q) + 2u * q);
    }
}

static void check_modulus(u32 q, bool fwd, bool fwd4) {
    const alch::ModP<u32> m = alch::make_modp<u32>(q);
    const u32 qni = m.qni, q2 = 2u * q;
    const u32 ws[4] = {0, 1, q - 1, m.r1};                             // R mod q: the Montgomery form of 1
    const u32 xy[6] = {0, 1, q - 1, q, q + 1, q2 - 1};
    if (fwd) {
        const long z0 = t_zero;
        for (u32 w : ws)
            for (u32 x : xy)
                for (u32 y : xy) one_fwd(x, y, w, q, qni);
        for (int it = 0; it < 100000; ++it) {
            const u64 r = rnd();
            one_fwd((u32)(r % q2), (u32)((r >> 32) % q2), (u32)(rnd() % q), q, qni);
        }
        u32 x = 0, y = 0, w = 0;
        EXPECT(t_zero - z0 >= 6 * 6 + 3 * 6);                          // w = 0 with every (x, y); y = 0 with the other three w
    }
    if (fwd4) {
        const u32 x4[9] = {0, 1, q - 1, q, q + 1, q2 - 1, q2, 3u * q, 4u * q - 1};
        const u32 y4[7] = {0, 1, q - 1, q, q + 1, q2 - 1, 0xffffffffu};
        const long z0 = t_zero;
        for (u32 w : ws)
            for (u32 x : x4)
                for (u32 y : y4) one_fwd4(x, y, w, q, qni);
        for (int it = 0; it < 100000; ++it) {
            const u64 r = rnd();
            one_fwd4((u32)(r % (4ull * q)), (u32)(r >> 32), (u32)(rnd() % q), q, qni);
        }
        u32 x = 0, y = 0, w = 0;
        EXPECT(t_zero - z0 >= 9 * 7 + 3 * 9);
    }
}

int main() {
    // the headline's four moduli and the largest prime below 2^31 that is 1 mod 2^16 (the first of them)
    const u32 q31[] = {2147352577u, 2146959361u, 2146041857u, 2145976321u};
    for (u32 q : q31) check_modulus(q, true, false);
    check_modulus(1073479681u, true, true);                            // the largest of the benchmark's primes below 2^30
    printf("t = 0 cases: %ld\n", t_zero);
    printf("OK: %ld failed expectation(s)\n", failed);
    return failed ? 1 : 0;
}
