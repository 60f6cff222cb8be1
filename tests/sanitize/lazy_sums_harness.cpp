// AddressSanitizer / UndefinedBehaviorSanitizer program for the four lazy 64-bit sums of the 32-bit word path
// (alchemy_amd/csrc/modarith.hpp: lazy_group, mont_red_lazy, dense_level, dense_row), checked against unsigned __int128
// arithmetic at the moduli where their inequalities are tight.  Stand-alone: built and run by tests/test_lazy_sums_host.py; it
// needs neither the library nor a device.  Every function under test is the header's, which the kernels include; the group loop
// (accumulate K products, carry with mont_red_lazy(acc) * r1) is restated here from k_tunnel_mac_e / k_tun2_mac / k_pt_mac.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../alchemy_amd/csrc/modarith.hpp"

using alch::csub;
using alch::dense_level;
using alch::dense_row;
using alch::lazy_group;
using alch::mont_red_lazy;
using alch::u32;
using alch::u64;
typedef unsigned __int128 u128;

static long failed = 0;
static u64 cur_q = 0;
#define EXPECT(...) do { if (!(__VA_ARGS__)) { if (++failed <= 20) printf("FAILED line %d (q = %llu): %s\n", __LINE__, (unsigned long long)cur_q, #__VA_ARGS__); } } while (0)

static u64 rng_state = 0x9e3779b97f4a7c15ull;
static u64 rnd() {                                  // splitmix64
    u64 z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// R^-1 mod q for ANY odd q (the class tops are not primes): 2^-1 = (q + 1) / 2
static const u128 TWO32 = (u128)1 << 32;
static const u128 TWO64 = (u128)1 << 64;

// ---- lazy_group ------------------------------------------------------------------------------------------------------------
static void check_group_rule(u32 q) {
    cur_q = q;
    const u32 K = lazy_group(q);
    const u64 kmax = 0xFFFFFFFFull / q;
    const u64 want = kmax < 4 ? 0 : (kmax - 2 > 8 ? 8 : kmax - 2);
    EXPECT(K == 0 || (K >= 2 && K <= 8));
    EXPECT(K == want);
    if (K >= 2) EXPECT((u128)(K + 2) * q < TWO32);
}

// ---- the group chain of the three inner-product kernels --------------------------------------------------------------------
// start: the value the sum starts from (< q); xs, ys: 3 K operand pairs (< q).  Returns the stored residue.
static u32 group_chain(u32 q, u32 qni, u32 r1, u32 K, u32 start, const u32* xs, const u32* ys, u32 nprod) {
    const u128 bound = (u128)q << 32;
    u64 acc = (u64)start * r1;
    u128 wide = (u128)start * r1;                                    // the same accumulator without a word size
    for (u32 d0 = 0; d0 < nprod; d0 += K) {
        const u32 dend = d0 + K < nprod ? d0 + K : nprod;
        for (u32 d = d0; d < dend; ++d) { acc += (u64)xs[d] * ys[d]; wide += (u128)xs[d] * ys[d]; }
        EXPECT(wide < bound);                                        // the precondition of mont_red_lazy
        EXPECT((u128)acc == wide);                                   // ... and nothing wrapped on the way
        if (dend < nprod) {
            const u32 t = mont_red_lazy(acc, q, qni);
            EXPECT(t < 2 * (u64)q);
            acc = (u64)t * r1;
            wide = (u128)t * r1;
        }
    }
    const u32 t = mont_red_lazy(acc, q, qni);
    EXPECT(t < 2 * (u64)q);
    return csub(t, q);
}

static u32 exact_chain(u32 q, u32 start, const u32* xs, const u32* ys, u32 nprod, u64 rinv) {
    u128 s = start;                                                  // start + R^-1 sum x y
    for (u32 d = 0; d < nprod; ++d) s = (s + (u128)xs[d] * ys[d] % q * rinv) % q;
    return (u32)s;
}

static void check_chain(u32 q) {
    cur_q = q;
    const alch::ModP<u32> m = alch::make_modp<u32>(q);
    const u64 rinv = alch::h_powmod(((u64)q + 1) / 2, 32, q);
    const u32 K = lazy_group(q);
    EXPECT(K >= 2);
    if (K < 2) return;
    const u32 n = 3 * K;
    std::vector<u32> xs(n), ys(n);
    // the bound itself: start q - 1, every product (q - 1)^2
    for (u32 d = 0; d < n; ++d) xs[d] = ys[d] = q - 1;
    EXPECT(group_chain(q, m.qni, m.r1, K, q - 1, xs.data(), ys.data(), n) == exact_chain(q, q - 1, xs.data(), ys.data(), n, rinv));
    // a last group that is not full, and a single group
    for (u32 np : {K - 1, K, K + 1, 2 * K + 1})
        EXPECT(group_chain(q, m.qni, m.r1, K, q - 1, xs.data(), ys.data(), np) == exact_chain(q, q - 1, xs.data(), ys.data(), np, rinv));
    const u32 corner[6] = {0, 1, q - 2, q - 1, (q - 1) / 2, (q + 1) / 2};
    for (u32 st : corner)
        for (u32 a : corner)
            for (u32 b : corner) {
                for (u32 d = 0; d < n; ++d) { xs[d] = a; ys[d] = b; }
                EXPECT(group_chain(q, m.qni, m.r1, K, st, xs.data(), ys.data(), n) == exact_chain(q, st, xs.data(), ys.data(), n, rinv));
                // the corner pair at one position of an otherwise worst-case chain
                for (u32 pos = 0; pos < n; ++pos) {
                    for (u32 d = 0; d < n; ++d) { xs[d] = ys[d] = q - 1; }
                    xs[pos] = a; ys[pos] = b;
                    EXPECT(group_chain(q, m.qni, m.r1, K, st, xs.data(), ys.data(), n) == exact_chain(q, st, xs.data(), ys.data(), n, rinv));
                }
            }
    for (int it = 0; it < 100000; ++it) {
        for (u32 d = 0; d < n; ++d) {
            const u64 r = rnd();
            // one word in four from the corner grid
            xs[d] = (r & 3) == 0 ? corner[(r >> 2) % 6] : (u32)((r >> 8) % q);
            const u64 r2 = rnd();
            ys[d] = (r2 & 3) == 0 ? corner[(r2 >> 2) % 6] : (u32)((r2 >> 8) % q);
        }
        const u32 st = (u32)(rnd() % q);
        EXPECT(group_chain(q, m.qni, m.r1, K, st, xs.data(), ys.data(), n) == exact_chain(q, st, xs.data(), ys.data(), n, rinv));
    }
}

// ---- dense_row -------------------------------------------------------------------------------------------------------------
template <typename W>
static W exact_row(const W* x, const W* M, int R, W q, u64 rinv) {
    u128 s = 0;
    for (int t = 0; t < R; ++t) s = (s + (u128)x[t] * M[t] % q * rinv) % q;
    return (W)s;
}

template <int R, int LVL>
static void check_row(u32 q) {
    cur_q = q;
    const alch::ModP<u32> m = alch::make_modp<u32>(q);
    const u64 rinv = alch::h_powmod(((u64)q + 1) / 2, 32, q);
    u32 x[R], M[R];
    auto one = [&]() {
        const u32 got = dense_row<R, LVL>((const u32*)x, (const u32*)M, q, m.qni);
        EXPECT(got < q);
        EXPECT(got == exact_row<u32>(x, M, R, q, rinv));
    };
    for (int t = 0; t < R; ++t) x[t] = M[t] = q - 1;                  // the bound: every product (q - 1)^2
    one();
    const u32 corner[6] = {0, 1, q - 2, q - 1, (q - 1) / 2, (q + 1) / 2};
    for (u32 a : corner)
        for (u32 b : corner) {
            for (int t = 0; t < R; ++t) { x[t] = a; M[t] = b; }
            one();
            for (int pos = 0; pos < R; ++pos) {                       // the corner pair at one position of a worst-case row
                for (int t = 0; t < R; ++t) x[t] = M[t] = q - 1;
                x[pos] = a; M[pos] = b;
                one();
                for (int t = 0; t < R; ++t) x[t] = M[t] = 0;          // ... and of an empty one
                x[pos] = a; M[pos] = b;
                one();
            }
        }
    for (int it = 0; it < 100000; ++it) {
        for (int t = 0; t < R; ++t) {
            const u64 r = rnd(), r2 = rnd();
            x[t] = (r & 3) == 0 ? corner[(r >> 2) % 6] : (u32)((r >> 8) % q);
            M[t] = (r2 & 3) == 0 ? corner[(r2 >> 2) % 6] : (u32)((r2 >> 8) % q);
        }
        one();
    }
}

template <int LVL>
static void check_rows(u32 q) {
    cur_q = q;
    EXPECT(dense_level(q) >= LVL);                                   // a ring of such moduli may run this variant
    // every H = (p - 1) / 2 and P - 1 the passes instantiate (p = 3, 5, 7, 11, 13)
    check_row<1, LVL>(q); check_row<2, LVL>(q); check_row<3, LVL>(q); check_row<4, LVL>(q);
    check_row<5, LVL>(q); check_row<6, LVL>(q); check_row<10, LVL>(q); check_row<12, LVL>(q);
}

static u32 largest_odd_at_level(int lvl) {                            // by dense_level itself, from above
    u32 q = 0x7FFFFFFFu;
    while (dense_level(q) < lvl) q -= 2;
    return q;
}

static void check_row64() {
    const u64 q = 4611686018427322369ull;                              // a 62-bit prime = 1 mod 2^16
    cur_q = q;
    EXPECT((q >> 61) == 1 && alch::h_powmod(3, q - 1, q) == 1);
    const alch::ModP<u64> m = alch::make_modp<u64>(q);
    const u64 rinv = alch::h_powmod((q + 1) / 2, 64, q);
    u64 x[12], M[12];
    for (int it = 0; it < 20000; ++it) {
        for (int t = 0; t < 12; ++t) {
            x[t] = it == 0 ? q - 1 : rnd() % q;
            M[t] = it == 0 ? q - 1 : rnd() % q;
        }
        u128 s = 0;
        for (int t = 0; t < 12; ++t) s = (s + (u128)((u128)x[t] * M[t] % q) * rinv) % q;
        const u64 got = dense_row<12, 0>((const u64*)x, (const u64*)M, q, m.qni);
        EXPECT(got < q && got == (u64)s);
        u128 s6 = 0;
        for (int t = 0; t < 6; ++t) s6 = (s6 + (u128)((u128)x[t] * M[t] % q) * rinv) % q;
        EXPECT(dense_row<6, 1>((const u64*)x, (const u64*)M, q, m.qni) == (u64)s6);
    }
}

int main() {
    // lazy_group: every odd q within 2^16 of 2^32 / k, k = 3 .. 12, and 10^6 random odd q < 2^31
    for (u32 k = 3; k <= 12; ++k) {
        const u64 c = (u64)(TWO32 / k);
        for (u64 q = (c - 65536) | 1; q <= c + 65536; q += 2)
            if (q < ((u64)1 << 31)) check_group_rule((u32)q);
    }
    for (int it = 0; it < 1000000; ++it) check_group_rule((u32)(rnd() % (1u << 31)) | 1u);
    check_group_rule(3); check_group_rule(12289); check_group_rule(0x7FFFFFFFu);

    // group chain: the largest odd q of each class kmax = 4 .. 11 (least headroom: (K + 2) q closest to 2^32)
    for (u32 kmax = 4; kmax <= 11; ++kmax) {
        u32 q = (u32)(0xFFFFFFFFull / kmax);
        if (!(q & 1)) --q;
        cur_q = q;
        EXPECT(0xFFFFFFFFu / q == kmax && 0xFFFFFFFFu / (q + 2) == kmax - 1);
        EXPECT(lazy_group(q) == (kmax - 2 > 8 ? 8 : kmax - 2));
        check_chain(q);
    }
    check_chain(12289);

    // dense_level: the two constants, and the inequality each one stands for
    cur_q = 0;
    EXPECT(dense_level(715827881ull) == 2 && dense_level(715827882ull) == 1 && dense_level(715827883ull) == 1);
    EXPECT(dense_level(1753413055ull) == 1 && dense_level(1753413056ull) == 0 && dense_level(1753413057ull) == 0);
    EXPECT(dense_level(3) == 2 && dense_level(0x7FFFFFFFull) == 0 && dense_level(((u64)1 << 61) + 1) == 0);
    {
        u64 q1 = 0x7FFFFFFFull, q2 = 0x7FFFFFFFull;
        while (dense_level(q1) < 1) --q1;                              // the largest q that gets level >= 1 / level 2
        while (dense_level(q2) < 2) --q2;
        EXPECT((u128)6 * q1 * q1 < TWO64);
        EXPECT((u128)6 * q2 < TWO32);
        EXPECT(!((u128)6 * (q1 + 2) * (q1 + 2) < TWO64));              // and each constant is the bound rounded down: it gives one modulus away
        EXPECT(!((u128)6 * (q2 + 2) < TWO32));
    }

    // dense_row<R, LVL>: every level at the largest odd q dense_level maps to it, level 0 at 2^31 - 1 too, every level at 12289
    const u32 top2 = largest_odd_at_level(2), top1 = largest_odd_at_level(1);
    cur_q = 0;
    EXPECT(top2 == 715827881u && top1 == 1753413055u);
    check_rows<2>(top2);
    check_rows<1>(top2); check_rows<1>(top1);
    check_rows<0>(top2); check_rows<0>(top1); check_rows<0>(0x7FFFFFFFu);
    check_rows<2>(12289); check_rows<1>(12289); check_rows<0>(12289);

    check_row64();
    printf("OK: %ld failed expectation(s)\n", failed);
    return failed ? 1 : 0;
}
