// AddressSanitizer / UndefinedBehaviorSanitizer program for the weighted sums of alch_ct_automorph_lincomb
// (alchemy_amd/csrc/modarith.hpp: lincomb_step, lincomb_close; alchemy_amd/csrc/kernel_lincomb.hpp: the row-block walk), checked against
// unsigned __int128 arithmetic.  Stand-alone: built and run by tests/test_lincomb_host.py; it needs neither the library nor a device.
// The functions under test are the headers', which the kernel evaluates; what is restated here from k_hoist_lincomb is the group
// counter (carry when K products are in the open group) and, below K = 2 and on 8-byte words, the product-at-a-time form with its
// closing product by R^2 mod q.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../alchemy_amd/csrc/modarith.hpp"
#include "../../alchemy_amd/csrc/kernel_lincomb.hpp"

using alch::lazy_group;
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

static bool is_prime(u64 q) {                       // Miller-Rabin, deterministic below 2^64 on these bases
    if (q < 2) return false;
    for (u64 p : {2ull, 3ull, 5ull, 7ull, 11ull, 13ull, 17ull, 19ull, 23ull, 29ull, 31ull, 37ull}) {
        if (q == p) return true;
        if (q % p == 0) return false;
    }
    u64 d = q - 1;
    int s = 0;
    while (!(d & 1)) { d >>= 1; ++s; }
    for (u64 a : {2ull, 3ull, 5ull, 7ull, 11ull, 13ull, 17ull, 19ull, 23ull, 29ull, 31ull, 37ull}) {
        u64 x = alch::h_powmod(a, d, q);
        if (x == 1 || x == q - 1) continue;
        bool comp = true;
        for (int r = 1; r < s && comp; ++r) {
            x = alch::h_mulmod(x, x, q);
            if (x == q - 1) comp = false;
        }
        if (comp) return false;
    }
    return true;
}

// sum_r y[r] w[r] mod q as the 4-byte kernel path evaluates it: lazy groups where K >= 2, else one Montgomery product at a time
static u32 weighted32(const alch::ModP<u32>& m, const u32* y, const u32* w, u32 n) {
    const u32 q = m.q, K = lazy_group(q);
    if (K >= 2) {
        const u128 bound = (u128)q << 32;
        u64 acc = 0;
        u128 wide = 0;
        u32 grp = 0;
        for (u32 r = 0; r < n; ++r) {
            const bool carry = grp == K;
            if (carry) {
                grp = 0;
                wide = (u128)alch::mont_red_lazy(acc, q, m.qni) * m.r1;      // what lincomb_step carries
            }
            ++grp;
            acc = alch::lincomb_step(acc, carry, y[r], w[r], q, m.qni, m.r1);
            wide += (u128)y[r] * w[r];
            EXPECT(wide < bound);                                            // the precondition of the next reduction
            EXPECT((u128)acc == wide);                                       // nothing wrapped
        }
        return alch::lincomb_close(acc, q, m.qni, m.r2);
    }
    u32 acc = 0;
    for (u32 r = 0; r < n; ++r) acc = alch::add_mod(acc, alch::mont_mul(y[r], w[r], m), q);
    return alch::mont_mul(acc, m.r2, m);
}

static u64 weighted64(const alch::ModP<u64>& m, const u64* y, const u64* w, u32 n) {
    u64 acc = 0;
    for (u32 r = 0; r < n; ++r) acc = alch::add_mod(acc, alch::mont_mul(y[r], w[r], m), m.q);
    return alch::mont_mul(acc, m.r2, m);
}

template <typename W>
static W exact(W q, const W* y, const W* w, u32 n) {
    u128 s = 0;
    for (u32 r = 0; r < n; ++r) s = (s + (u128)y[r] * w[r] % q) % q;
    return (W)s;
}

static void check32(u32 q, u32 kmax) {
    cur_q = q;
    EXPECT(is_prime(q) && 0xFFFFFFFFu / q == kmax);
    const alch::ModP<u32> m = alch::make_modp<u32>(q);
    const u32 K = lazy_group(q);
    EXPECT(K == (kmax < 4 ? 0u : (kmax - 2 > 8 ? 8u : kmax - 2)));
    const u32 Ke = K ? K : 1;
    std::vector<u32> y(3 * 8 + 2), w(3 * 8 + 2);
    // every operand q - 1: group lengths on either side of K, at 2 K and beyond it; 32 is the largest set
    for (u32 n : {1u, Ke - 1, Ke, Ke + 1, 2 * Ke - 1, 2 * Ke, 2 * Ke + 1, 3 * Ke + 2, 32u}) {
        if (n == 0) continue;
        y.assign(n, q - 1);
        w.assign(n, q - 1);
        const u32 got = weighted32(m, y.data(), w.data(), n);
        EXPECT(got < q);
        EXPECT(got == exact<u32>(q, y.data(), w.data(), n));
        EXPECT(got == (u32)(n % q));                                         // (q - 1)^2 = 1
    }
    const u32 corner[6] = {0, 1, q - 2, q - 1, (q - 1) / 2, (q + 1) / 2};
    for (int it = 0; it < 20000; ++it) {
        const u32 n = 1 + (u32)(rnd() % 32);
        y.resize(n);
        w.resize(n);
        for (u32 r = 0; r < n; ++r) {
            const u64 a = rnd(), b = rnd();
            y[r] = (a & 3) == 0 ? corner[(a >> 2) % 6] : (u32)((a >> 8) % q);
            w[r] = (b & 3) == 0 ? corner[(b >> 2) % 6] : (u32)((b >> 8) % q);
        }
        const u32 got = weighted32(m, y.data(), w.data(), n);
        EXPECT(got < q && got == exact<u32>(q, y.data(), w.data(), n));
    }
}

static void check64(u64 q) {
    cur_q = q;
    EXPECT(is_prime(q) && (q >> 61) == 1);
    const alch::ModP<u64> m = alch::make_modp<u64>(q);
    std::vector<u64> y, w;
    for (u32 n : {1u, 2u, 7u, 8u, 9u, 17u, 32u}) {
        y.assign(n, q - 1);
        w.assign(n, q - 1);
        const u64 got = weighted64(m, y.data(), w.data(), n);
        EXPECT(got < q && got == exact<u64>(q, y.data(), w.data(), n) && got == n);
    }
    for (int it = 0; it < 20000; ++it) {
        const u32 n = 1 + (u32)(rnd() % 32);
        y.resize(n);
        w.resize(n);
        for (u32 r = 0; r < n; ++r) { y[r] = (rnd() & 7) ? rnd() % q : q - 1; w[r] = (rnd() & 7) ? rnd() % q : q - 1; }
        const u64 got = weighted64(m, y.data(), w.data(), n);
        EXPECT(got < q && got == exact<u64>(q, y.data(), w.data(), n));
    }
}

// the launches of one call: block i covers rows [i ROWS, i ROWS + lincomb_block_rows), as do_lincomb walks them
static void check_row_walk() {
    cur_q = 0;
    const size_t ROWS = (size_t)alch::LINCOMB_ROWS;
    EXPECT(ROWS >= 1 && alch::LINCOMB_TILE >= 1);
    EXPECT(alch::lincomb_blocks(0, ROWS) == 0);
    for (size_t n_out = 1; n_out <= 3 * ROWS + 1; ++n_out) {
        std::vector<int> hit(n_out, 0);
        const size_t nblk = alch::lincomb_blocks(n_out, ROWS);
        EXPECT(nblk == (n_out + ROWS - 1) / ROWS);
        for (size_t i = 0; i < nblk; ++i) {
            const size_t g0 = i * ROWS, rows = alch::lincomb_block_rows(n_out, ROWS, i);
            EXPECT(rows >= 1 && rows <= ROWS && g0 + rows <= n_out);
            EXPECT(i + 1 == nblk || rows == ROWS);                           // only the last block is short
            for (size_t g = g0; g < g0 + rows && g < n_out; ++g) ++hit[g];   // the vector is indexed under ASan
        }
        for (size_t g = 0; g < n_out; ++g) EXPECT(hit[g] == 1);
    }
}

int main() {
    // every class kmax = floor((2^32 - 1) / q) = 2 .. 11 on the primes at both ends of the class (2 and 3: K = 0)
    for (u32 kmax = 2; kmax <= 11; ++kmax) {
        u32 top = (u32)(0xFFFFFFFFull / kmax), bottom = (u32)(0xFFFFFFFFull / (kmax + 1)) + 1;
        while (!is_prime(top)) --top;
        while (!is_prime(bottom)) ++bottom;
        cur_q = top;
        EXPECT(top < (1u << 31) && bottom < top);
        check32(top, kmax);
        check32(bottom, kmax);
    }
    check32(12289, 0xFFFFFFFFu / 12289);
    // the two largest primes below 2^62
    u64 q = ((u64)1 << 62) - 1;
    int found = 0;
    for (; found < 2; q -= 2)
        if (is_prime(q)) { check64(q); ++found; }
    check_row_walk();
    printf("ROWS %d TILE %d\n", alch::LINCOMB_ROWS, alch::LINCOMB_TILE);
    printf("OK: %ld failed expectation(s)\n", failed);
    return failed ? 1 : 0;
}
