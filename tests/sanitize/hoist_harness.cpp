// Stand-alone program for tests/test_hoist_host.py: where the hoisted inner product (alchemy_amd/csrc/kernel_hoist.hpp) reads, checked
// on the host under AddressSanitizer and UndefinedBehaviorSanitizer.
//   Radix-16 engine: for every two-power n from 16 to 2^16, EVERY unit j of Z_2n^* and VL in {2, 4}, the pack address and the picks of
//   automorph::pow2_pack (the expression the kernel evaluates once per item) name, slot by slot, the source slot of the table BY ITS
//   DEFINITION -- slot k holds the unit 2 brev(k) + 1; the source of k is the slot that holds unit(k) j mod 2n -- and every aligned
//   pack of VL destination slots reads exactly one aligned pack of VL source slots, each of its slots once.  That table is what
//   alch_automorph_table returns: automorph::build_table is compared with it for every unit up to n = 2^9 and for eight units of every
//   larger n (build_table costs a thousand cycles an entry; the sweep has 5.7 10^9 entries).
//   General engine, indices 9, 45, 21, 11648 and every unit (11648: 64 of them): the VL table entries one 16-byte (VL = 4) or 8-byte
//   (VL = 2) load of piece p brings are entries VL p .. VL p + VL - 1, the words the one-word form reads one by one; all lie below n;
//   the one-word form is the one chosen exactly where VL does not divide n (n = 6, VL = 4).
// The sweep runs on up to eight threads, each with counters of its own.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../../alchemy_amd/csrc/automorph_host.hpp"

namespace am = alch::automorph;

static std::atomic<int> failed{0};
#define EXPECT(cond, ...)                                          \
    do {                                                           \
        if (!(cond)) {                                             \
            if (failed.fetch_add(1) < 20) { std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                          \
    } while (0)

template <int VL>
static bool packs_ok(const uint32_t* tab, uint32_t n, uint32_t j, int logn) {
    bool ok = true;
    for (uint32_t k0 = 0; k0 < n; k0 += VL) {
        uint32_t pick[VL];
        const uint32_t pack = am::pow2_pack<VL>(k0, j, logn, pick);
        uint32_t seen = 0;
        ok = ok && pack % VL == 0 && pack + VL <= n;
        for (int c = 0; c < VL; ++c) {
            ok = ok && pick[c] < (uint32_t)VL && pack + pick[c] == tab[k0 + c];
            seen |= 1u << (pick[c] & 31u);
        }
        ok = ok && seen == (1u << VL) - 1u;                  // the pack is read whole: a permutation inside
    }
    return ok;
}

template <int VL>
struct alignas(4 * VL) Piece { uint32_t v[VL]; };

template <int VL>
static void general_pieces(uint32_t m, uint32_t j, const std::vector<uint32_t>& t, size_t& pieces) {
    const uint32_t n = (uint32_t)t.size();
    if (n % VL) return;                                     // the one-word form serves this ring
    for (uint32_t p = 0; p < n / VL; ++p) {
        Piece<VL> x;
        std::memcpy(&x, t.data() + (size_t)p * VL, sizeof x);            // what one load of the piece brings
        for (int c = 0; c < VL; ++c) EXPECT(x.v[c] == t[(size_t)p * VL + c] && x.v[c] < n, "m=%u j=%u piece %u word %d", m, j, p, c);
        ++pieces;
    }
}

int main() {
    size_t units_total = 0, cross = 0;
    const unsigned hw = std::thread::hardware_concurrency();
    const unsigned nthreads = hw < 1 ? 1 : hw > 8 ? 8 : hw;
    for (int logn = 4; logn <= 16; ++logn) {
        const uint32_t n = 1u << logn, m = 2 * n;
        // the definition: slot k holds the unit 2 brev(k) + 1 (brev restated here, bit by bit)
        std::vector<uint32_t> unit(n), where(m, 0xffffffffu);
        for (uint32_t k = 0; k < n; ++k) {
            uint32_t r = 0;
            for (int b = 0; b < logn; ++b) r |= ((k >> b) & 1u) << (logn - 1 - b);
            unit[k] = 2 * r + 1;
            where[unit[k]] = k;
        }
        am::Plan P;
        EXPECT(am::plan(m, P) == am::PLAN_OK && P.n == n, "logn=%d", logn);
        std::vector<std::thread> pool;
        std::vector<size_t> bad(nthreads, 0);
        for (unsigned t = 0; t < nthreads; ++t)
            pool.emplace_back([&, t]() {
                std::vector<uint32_t> tab(n);
                for (uint32_t j = 1 + 2 * t; j < m; j += 2 * nthreads) {
                    for (uint32_t k = 0; k < n; ++k) tab[k] = where[(unit[k] * j) & (m - 1)];
                    if (!packs_ok<2>(tab.data(), n, j, logn) || !packs_ok<4>(tab.data(), n, j, logn) ||
                        (j < 64 && !packs_ok<4>(tab.data(), n, j + 3 * m, logn)))          // an unreduced unit reads the same slots
                        ++bad[t];
                }
            });
        for (auto& th : pool) th.join();
        for (unsigned t = 0; t < nthreads; ++t) EXPECT(bad[t] == 0, "logn=%d: %zu units whose packs or picks differ from the table (thread %u)", logn, bad[t], t);
        units_total += n;
        // the definition against build_table, what alch_automorph_table returns
        const uint32_t step = logn <= 9 ? 2 : (m / 8) | 2u;
        for (uint32_t j = 1; j < m; j += step) {
            const uint32_t ju = j | 1u;
            std::vector<uint32_t> t;
            EXPECT(am::build_table(P, ju, t) && t.size() == n, "logn=%d j=%u", logn, ju);
            bool same = t.size() == n;
            for (uint32_t k = 0; same && k < n; ++k) same = t[k] == where[(unit[k] * ju) & (m - 1)];
            EXPECT(same, "logn=%d j=%u: build_table differs from the definition", logn, ju);
            ++cross;
        }
    }
    size_t pieces = 0, gen_units = 0;
    for (uint32_t m : {9u, 45u, 21u, 11648u}) {
        am::Plan P;
        EXPECT(am::plan(m, P) == am::PLAN_OK, "m=%u", m);
        uint32_t taken = 0;
        for (uint32_t j = 1; j < m && taken < 64; ++j) {
            if (am::gcd(j, m) != 1) continue;
            std::vector<uint32_t> t;
            EXPECT(am::build_table(P, j, t) && t.size() == P.n, "m=%u j=%u", m, j);
            general_pieces<4>(m, j, t, pieces);
            general_pieces<2>(m, j, t, pieces);
            ++taken;
            ++gen_units;
        }
        EXPECT((P.n % 4 != 0) == (m == 9u), "m=%u: n=%u", m, P.n);       // n = 6 alone takes the one-word form on 4-byte words
    }
    std::printf("swept %zu units of 13 two-power sizes on %u thread(s), %zu tables against build_table; %zu general units, %zu pieces\n", units_total,
                nthreads, cross, gen_units, pieces);
    std::printf("OK: %d failed expectation(s)\n", failed.load());
    return failed.load() ? 1 : 0;
}
