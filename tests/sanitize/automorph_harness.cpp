// Stand-alone program for tests/test_automorph_host.py: the slot tables of the Galois automorphisms
// (alchemy_amd/csrc/automorph_host.hpp) built under AddressSanitizer and UndefinedBehaviorSanitizer for every index
// 2^a 3^b 5^c 7^d 11^e 13^f with phi <= PHI_MAX and every unit j of it:
//   - the table is a permutation of [0, phi);
//   - slot k's unit times j is the unit of the slot the table names (the definition, through axis_unit and Chinese remaindering);
//   - table(1) is the identity, table(j + m) = table(j), and the group law table(j1 j2) = table(j2) o table(j1) holds;
//   - for a two-power index the table equals pow2_src, the closed form the radix-16 kernel evaluates per lane (shared header);
//   - plan() refuses what alch_ring_create refuses on both engines.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../alchemy_amd/csrc/automorph_host.hpp"

#ifndef PHI_MAX
#define PHI_MAX 384
#endif

namespace am = alch::automorph;

static int failed = 0;
#define EXPECT(cond, ...)                                          \
    do {                                                           \
        if (!(cond)) {                                             \
            if (++failed <= 20) { std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                          \
    } while (0)

// the unit of Z_m^* behind slot k: Chinese remaindering of the per-axis units
static uint32_t slot_unit(const am::Plan& P, uint32_t k) {
    uint64_t u = 0, mod = 1;
    for (int l = 0; l < P.nax; ++l) {
        const am::Axis& a = P.ax[l];
        const uint64_t ul = am::axis_unit(a, (k / a.rts) % a.dim);
        uint64_t t = ul;
        if (mod > 1) {
            uint64_t inv = 1;
            for (uint64_t c = 1; c < a.ml; ++c) if (mod % a.ml * c % a.ml == 1) { inv = c; break; }
            t = (ul + a.ml - u % a.ml) % a.ml * inv % a.ml;
        }
        u += mod * t;
        mod *= a.ml;
    }
    return (uint32_t)(P.m > 1 ? u % P.m : 0);
}

int main() {
    const uint32_t primes[6] = {2, 3, 5, 7, 11, 13};
    std::vector<uint32_t> indices;
    for (uint32_t m = 1; m <= 6 * PHI_MAX; ++m) {           // m / phi(m) <= 2 * 3/2 * 5/4 * 7/6 * 11/10 * 13/12 < 5.3 for these primes
        uint32_t r = m;
        for (uint32_t p : primes) while (r % p == 0) r /= p;
        if (r != 1) continue;
        am::Plan P;
        if (am::plan(m, P) != am::PLAN_OK || P.n > PHI_MAX) continue;
        indices.push_back(m);
    }
    size_t tables = 0, units_total = 0, pow2_checked = 0;
    for (uint32_t m : indices) {
        am::Plan P;
        EXPECT(am::plan(m, P) == am::PLAN_OK, "m=%u", m);
        const uint32_t n = P.n;
        std::vector<uint32_t> unit(n), where(m + 1, 0xffffffffu);
        for (uint32_t k = 0; k < n; ++k) {
            unit[k] = slot_unit(P, k);
            EXPECT(am::gcd(unit[k], m) == 1 && where[unit[k]] == 0xffffffffu, "m=%u slot %u unit %u", m, k, unit[k]);
            where[unit[k]] = k;
        }
        std::vector<uint32_t> us;
        for (uint32_t j = 0; j < m; ++j) if (am::gcd(j, m) == 1) us.push_back(j);
        EXPECT(us.size() == n, "m=%u: %zu units, phi %u", m, us.size(), n);
        units_total += us.size();
        std::vector<std::vector<uint32_t>> tab(m);
        for (uint32_t j : us) {
            std::vector<uint32_t>& t = tab[j];
            EXPECT(am::build_table(P, j, t) && t.size() == n, "m=%u j=%u", m, j);
            ++tables;
            std::vector<char> seen(n, 0);
            for (uint32_t k = 0; k < n; ++k) {
                EXPECT(t[k] < n && !seen[t[k]], "m=%u j=%u k=%u: not a permutation", m, j, k);
                if (t[k] < n) seen[t[k]] = 1;
                EXPECT(t[k] < n && unit[t[k]] == (uint64_t)unit[k] * j % m, "m=%u j=%u k=%u: wrong unit", m, j, k);
            }
            std::vector<uint32_t> shifted;
            EXPECT(am::build_table(P, j + m, shifted) && shifted == t, "m=%u j=%u: j + m differs", m, j);
            if ((m & (m - 1)) == 0 && m >= 2) {
                int logn = 0;
                while ((1u << logn) < n) ++logn;
                for (uint32_t k = 0; k < n; ++k) EXPECT(am::pow2_src(k, j, logn) == t[k] && am::pow2_src(k, j + 3 * m, logn) == t[k], "m=%u j=%u k=%u: closed form", m, j, k);
                ++pow2_checked;
            }
        }
        for (uint32_t k = 0; k < n; ++k) EXPECT(tab[1 % m][k] == k, "m=%u: table(1) is not the identity", m);
        // the group law on every pair (few units) or on a fixed stride of pairs
        const size_t step = us.size() <= 24 ? 1 : us.size() / 24;
        for (size_t x = 0; x < us.size(); x += step)
            for (size_t y = 0; y < us.size(); y += step) {
                const uint32_t j1 = us[x], j2 = us[y], j12 = (uint32_t)((uint64_t)j1 * j2 % m);
                for (uint32_t k = 0; k < n; ++k) EXPECT(tab[j12][k] == tab[j2][tab[j1][k]], "m=%u: table(%u * %u) is not the composition at %u", m, j1, j2, k);
            }
        std::vector<uint32_t> none;
        for (uint32_t p : primes) if (m % p == 0) EXPECT(!am::build_table(P, p, none), "m=%u: the non-unit %u was accepted", m, p);
    }
    // the closed form at the sizes of the radix-16 engine, against the table, for a few units
    for (int logn = 4; logn <= 16; ++logn) {
        am::Plan P;
        EXPECT(am::plan(2u << logn, P) == am::PLAN_OK && P.n == (1u << logn), "logn=%d", logn);
        for (uint32_t j : {3u, 5u, (2u << logn) - 1u, 0x9E3779B1u % (2u << logn) | 1u}) {
            std::vector<uint32_t> t;
            EXPECT(am::build_table(P, j, t), "logn=%d j=%u", logn, j);
            for (uint32_t k = 0; k < P.n && k < t.size(); ++k) EXPECT(am::pow2_src(k, j, logn) == t[k], "logn=%d j=%u k=%u", logn, j, k);
            // an aligned group of four destination slots reads one aligned group of four source slots (kernel_automorph.hpp)
            for (uint32_t k = 0; k + 3 < P.n && k + 3 < t.size(); k += 4)
                EXPECT((t[k] >> 2) == (t[k + 1] >> 2) && (t[k] >> 2) == (t[k + 2] >> 2) && (t[k] >> 2) == (t[k + 3] >> 2), "logn=%d j=%u k=%u: group", logn, j, k);
            ++pow2_checked;
        }
    }
    am::Plan P;
    EXPECT(am::plan(0, P) == am::PLAN_INVALID, "m=0");
    for (uint32_t m : {17u, 34u, 204u, 1u << 18, 1u << 31, 177147u, 4294967295u}) EXPECT(am::plan(m, P) == am::PLAN_UNSUPPORTED, "m=%u", m);
    for (uint32_t m : {1u, 2u, 16u, 1u << 17, 11648u, 20475u, 65536u}) EXPECT(am::plan(m, P) == am::PLAN_OK, "m=%u", m);
    std::printf("walked %zu indices with phi <= %d: %zu tables, %zu units, %zu closed-form comparisons\n", indices.size(), PHI_MAX, tables, units_total, pow2_checked);
    std::printf("OK: %d failed expectation(s)\n", failed);
    return failed ? 1 : 0;
}
