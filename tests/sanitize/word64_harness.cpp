// AddressSanitizer / UndefinedBehaviorSanitizer program for the 64-bit word path of alchemy_amd/csrc/modarith.hpp (the header the
// kernels include), checked against unsigned __int128 arithmetic at both ends of the accepted modulus range (2^31 < q < 2^62).
// Stand-alone: built and run by tests/test_word64_host.py; it needs neither the library nor a device.
//
//   word64_harness q_0 q_1 ...      every check below for every modulus given; "OK: 0 failed expectation(s)" and status 0 when all hold
//   word64_harness --negative q     the range expectations alone ("4q fits the word", the [0,4q) butterfly chain) for a modulus the
//                                   library does NOT accept: with q > 2^62 they must report violations (status 1)
//
// make_modp, h_shoup_const, mont_mul_lazy, shoup_mul_lazy, the butterflies, csub, add_mod and sub_mod are the header's.  The
// digit-entry expressions of k_ks_accum<u64> (kernels_ntt.hpp) and DevRing::dig_off (alchemy_hip.hip, build_dev_ring) are restated.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../alchemy_amd/csrc/modarith.hpp"

using alch::Sh64;
using alch::u64;
typedef unsigned __int128 u128;
typedef __int128 i128;

static long failed = 0;
static u64 cur_q = 0;
#define EXPECT(c) do { if (!(c)) { if (++failed <= 20) printf("FAILED line %d (q = %llu): %s\n", __LINE__, (unsigned long long)cur_q, #c); } } while (0)

static u64 rng_state = 0x9e3779b97f4a7c15ull;
static u64 rnd() {                                  // splitmix64
    u64 z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

static u64 mulmod(u128 a, u128 b, u64 q) { return (u64)((a % q) * (b % q) % q); }
static const u128 WORD = (u128)1 << 64;

// ---- the range expectations: what "4q < 2^64 for every supported modulus" buys.  Also the negative control's whole run.
// One radix-16 pass: four butterfly stages over 16 values, distances 8, 4, 2, 1, FIRST on the first and LAST on the last.
static void check_ranges_and_chain(u64 q, int trials) {
    cur_q = q;
    const u128 q2 = (u128)2 * q, q4 = (u128)4 * q;
    EXPECT(q4 < WORD);                                                  // 4q fits the word
    EXPECT(q2 < ((u128)1 << 63));                                       // 2q < 2^63: the range the header states for lazy data
    const u64 corner[7] = {0, 1, q - 1, q, q + 1, (u64)(q2 - 2), (u64)(q2 - 1)};
    for (int it = 0; it < trials; ++it) {
        u64 v[16], ref[16];
        for (int k = 0; k < 16; ++k) {
            const u64 r = rnd();
            v[k] = (r & 3) ? corner[(r >> 2) % 7] : (u64)(((u128)rnd() << 64 | rnd()) % q2);   // [0, 2q)
            ref[k] = v[k] % q;
        }
        for (int st = 0; st < 4; ++st) {
            const int dist = 8 >> st;
            const bool first = st == 0, last = st == 3;
            for (int k = 0; k < 16; ++k) {
                if (k & dist) continue;
                const u64 wsel = rnd();
                const u64 wc[4] = {1, q - 1, (q + 1) / 2, 1 + rnd() % (q - 1)};
                const u64 w = wc[wsel & 3];
                const Sh64 tw = alch::h_shoup_const(w, q);
                u64 x = v[k], y = v[k + dist];
                // the same butterfly as 128-bit values: nothing may wrap, intermediate values stay below 4q
                const u128 xx = first ? (u128)x : ((u128)x >= q2 ? (u128)x - q2 : (u128)x);
                const u64 t = alch::shoup_mul_lazy(y, tw, q);
                EXPECT((u128)t < q2);
                EXPECT(t % q == mulmod(y, w, q));
                const u128 X = xx + t, Y = xx + (q2 - t);
                EXPECT(X < q4 && Y < q4);
                EXPECT(X < WORD && Y < WORD);
                alch::bfly_fwd_st(x, y, tw, q, (u64)0, first, last);
                if (!last) { EXPECT((u128)x == X && (u128)y == Y); }
                else { EXPECT((u128)x < q2 && (u128)y < q2); EXPECT((u128)x == (X >= q2 ? X - q2 : X) && (u128)y == (Y >= q2 ? Y - q2 : Y)); }
                const u64 rx = ref[k], ry = mulmod(ref[k + dist], w, q);
                ref[k] = (u64)(((u128)rx + ry) % q);
                ref[k + dist] = (u64)(((u128)rx + q - ry) % q);
                EXPECT(x % q == ref[k] && y % q == ref[k + dist]);
                v[k] = x;
                v[k + dist] = y;
            }
        }
    }
}

static void check_modulus(u64 q) {
    cur_q = q;
    const alch::ModP<u64> m = alch::make_modp<u64>(q);
    const u64 qni = m.qni;
    const u128 q2 = (u128)2 * q;

    // ---- make_modp<u64>, h_shoup_const
    EXPECT(m.q == q);
    EXPECT((u64)(q * qni) == ~(u64)0);                                  // q qni = -1 (mod 2^64)
    EXPECT(m.r1 == (u64)(WORD % q));
    EXPECT(m.r2 == mulmod(WORD % q, WORD % q, q));
    const u64 rinv = alch::h_powmod(m.r1, q - 2, q);                    // R^-1 mod q
    EXPECT(mulmod(rinv, m.r1, q) == 1);
    const u64 bs[8] = {0, 1, q - 2, q - 1, (q - 1) / 2, (q + 1) / 2, rnd() % q, rnd() % q};
    for (u64 c : bs) {
        const Sh64 t = alch::h_shoup_const(c, q);
        EXPECT(t.w == c);
        EXPECT((u128)t.wp * q <= ((u128)c << 64) && ((u128)c << 64) < ((u128)t.wp + 1) * q);   // wp = floor(c 2^64 / q)
    }

    // ---- mont_mul_lazy(u64), shoup_mul_lazy: a ANY word, b < q  ->  [0, 2q), congruent
    const u64 as[12] = {0, 1, q - 1, q, q + 1, (u64)(q2 - 1), (u64)q2, (u64)((u128)4 * q - 1), ~(u64)0, (q - 1) / 2, (q + 1) / 2, rnd()};
    auto check_pair = [&](u64 a, u64 b) {
        const u64 p = alch::mont_mul_lazy(a, b, q, qni);
        EXPECT((u128)p < q2);
        EXPECT(p % q == mulmod(mulmod(a, b, q), rinv, q));
        const u64 s = alch::shoup_mul_lazy(a, alch::h_shoup_const(b, q), q);
        EXPECT((u128)s < q2);
        EXPECT(s % q == mulmod(a, b, q));
        EXPECT(alch::mont_mul(a, b, m) == mulmod(mulmod(a, b, q), rinv, q));
    };
    for (u64 a : as)
        for (int ib = 0; ib < 6; ++ib) check_pair(a, bs[ib]);
    for (int it = 0; it < 1000000; ++it) check_pair(rnd(), rnd() % q);

    // ---- the forward pass
    check_ranges_and_chain(q, 20000);
    cur_q = q;

    // ---- inverse butterflies (Shoup and Montgomery twiddles) and the generic forward one: [0,2q) in and out
    const u64 corner[7] = {0, 1, q - 1, q, q + 1, (u64)(q2 - 2), (u64)(q2 - 1)};
    const u64 ws[5] = {1, q - 1, (q + 1) / 2, (q - 1) / 2, 1 + rnd() % (q - 1)};
    auto check_bfly = [&](u64 x0, u64 y0, u64 w) {
        const u64 wm = mulmod(w, m.r1, q);                              // Montgomery form
        const u64 sum = (u64)(((u128)x0 + y0) % q), dif = mulmod(((u128)x0 % q + q - y0 % q) % q, w, q);
        u64 x = x0, y = y0;
        alch::bfly_inv(x, y, alch::h_shoup_const(w, q), q, qni);
        EXPECT((u128)x < q2 && (u128)y < q2 && x % q == sum && y % q == dif);
        x = x0; y = y0;
        alch::bfly_inv<u64>(x, y, wm, q, qni);
        EXPECT((u128)x < q2 && (u128)y < q2 && x % q == sum && y % q == dif);
        x = x0; y = y0;
        alch::bfly_fwd<u64>(x, y, wm, q, qni);
        const u64 wy = mulmod(y0, w, q);
        EXPECT((u128)x < q2 && (u128)y < q2);
        EXPECT(x % q == (u64)(((u128)x0 % q + wy) % q) && y % q == (u64)(((u128)x0 % q + q - wy) % q));
    };
    for (u64 x : corner)
        for (u64 y : corner)
            for (u64 w : ws) check_bfly(x, y, w);
    for (int it = 0; it < 200000; ++it)
        check_bfly((u64)(((u128)rnd() << 64 | rnd()) % q2), (u64)(((u128)rnd() << 64 | rnd()) % q2), 1 + rnd() % (q - 1));

    // ---- csub, add_mod, sub_mod on the corner grid.  csub: [0,2q) -> [0,q).  add_mod is csub(a + b): exact whenever a + b < 2q
    // (its contract a, b < q included).  sub_mod: exact whenever -q <= a - b < q (its contract a, b < q included).
    for (u64 a : corner) {
        EXPECT(alch::csub(a, q) == a % q);
        for (u64 b : corner) {
            if ((u128)a + b < q2) { const u64 s = alch::add_mod<u64>(a, b, q); EXPECT(s < q && s == (u64)(((u128)a + b) % q)); }
            const i128 d = (i128)a - (i128)b;
            if (d >= -(i128)q && d < (i128)q) { const u64 s = alch::sub_mod<u64>(a, b, q); EXPECT(s < q && s == (u64)((d + (i128)q) % (i128)q)); }
        }
    }
}

// ---- the digit-entry expressions of k_ks_accum<u64, BALANCED>: a TrivGad digit z of limb q_i (|z| <= (q_i - 1) / 2, stored as a
// signed 64-bit word) enters limb q_j's transform as
//     BALANCED (every (q - 1) / 2 of the ring below every q):  v = (W)z + q_j                                  in (0, 2 q_j)
//     otherwise:  v = mont_mul_lazy((W)z + dig_off_j, r1_j),  dig_off_j = ceil(maxhalf / q_j) q_j, maxhalf = max_i (q_i - 1) / 2   in [0, 2 q_j)
static void check_digit_entry(u64 qi, u64 qj) {
    cur_q = qj;
    const alch::ModP<u64> m = alch::make_modp<u64>(qj);
    const u64 maxhalf = (qi - 1) / 2;
    const u64 dig_off = ((maxhalf + qj - 1) / qj) * qj;
    EXPECT((u128)dig_off == ((u128)maxhalf + qj - 1) / qj * qj);        // the table builder's expression does not wrap
    EXPECT(dig_off % qj == 0 && dig_off >= maxhalf);
    const int64_t h = (int64_t)maxhalf;
    const int64_t zs[11] = {0, 1, -1, h, -h, h - 1, -(h - 1), (int64_t)(rnd() % (maxhalf + 1)), -(int64_t)(rnd() % (maxhalf + 1)),
                            (int64_t)(qj % (maxhalf + 1)), -(int64_t)(qj % (maxhalf + 1))};
    for (int64_t z : zs) {
        const u64 want = (u64)((((i128)z % (i128)qj) + (i128)qj) % (i128)qj);
        const i128 exact = (i128)z + (i128)dig_off;                     // the sum as an integer
        EXPECT(exact >= 0 && (u128)exact < WORD);                       // it does not wrap
        const u64 s = (u64)z + dig_off;
        EXPECT((i128)s == exact);
        const u64 v = alch::mont_mul_lazy(s, m.r1, qj, m.qni);
        EXPECT((u128)v < (u128)2 * qj && v % qj == want);
        if (maxhalf < qj) {                                             // a balanced pair
            const i128 eb = (i128)z + (i128)qj;
            EXPECT(eb > 0 && (u128)eb < (u128)2 * qj);
            const u64 vb = (u64)z + qj;
            EXPECT((i128)vb == eb && vb % qj == want);
        }
    }
}

int main(int argc, char** argv) {
    if (argc == 3 && !strcmp(argv[1], "--negative")) {
        const u64 q = strtoull(argv[2], nullptr, 10);
        check_ranges_and_chain(q, 2000);
        printf("NEGATIVE CONTROL: %ld failed expectation(s)\n", failed);
        return failed ? 1 : 0;
    }
    if (argc < 2) { fprintf(stderr, "usage: word64_harness q_0 q_1 ... | --negative q\n"); return 2; }
    std::vector<u64> qs;
    for (int i = 1; i < argc; ++i) qs.push_back(strtoull(argv[i], nullptr, 10));
    for (u64 q : qs) {
        cur_q = q;
        EXPECT(q > 2 && (q & 1) && q < ((u64)1 << 62));
        if (failed) break;
        check_modulus(q);
    }
    for (u64 qi : qs)
        if (qi > ((u64)1 << 61))
            for (u64 qj : qs) check_digit_entry(qi, qj);
    printf("checked %zu moduli\n", qs.size());
    printf("OK: %ld failed expectation(s)\n", failed);
    return failed ? 1 : 0;
}
