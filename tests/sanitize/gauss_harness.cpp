// Stand-alone host program (own main, no device, no library): prints what the shared sampler code of the encrypt path computes, for
// tests/test_gauss_host.py to compare with the Python model value for value.  Built with -fsanitize=address,undefined.
//
//   D <w0> <w1> <f>                                   the scalar deviate gauss::deviate at crafted table boundaries
//   E <m> <svar bits> <seed> <elem> <p> | <coset words, or nothing> | <z ...>
//                                                     one whole element of the host mirror (cycgen.hpp: gaussDecCounter)
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../alchemy_amd/host/cycgen.hpp"

using namespace alch;

static void deviate_line(uint64_t w0) {
    const uint64_t w1 = gauss::mix64(w0 ^ 0xC0FFEEull);
    std::printf("D %" PRIu64 " %" PRIu64 " %" PRId64 "\n", w0, w1, gauss::deviate(w0, w1, gauss::CDT));
}

int main() {
    const uint32_t ts[] = {0, 1, 290, 580, 581};
    for (uint32_t t : ts)
        for (int d = -1; d <= 2; ++d) deviate_line(2 * gauss::CDT[t] + (uint64_t)(int64_t)d);    // wraps at t = 581, d = 2
    deviate_line(0);
    deviate_line(~(uint64_t)0);

    const uint32_t ms[] = {16, 21, 45, 91};
    const int64_t ps[] = {0, 2, 32, 7};
    for (uint32_t m : ms)
        for (int64_t p : ps)
            for (int big = 0; big < 2; ++big) {
                const uint32_t n = alchemy::gen::totient(m);
                const double svar = (big ? 5.0 * 1024.0 : 3.0) / std::sqrt((double)n) * (p ? (double)p * (double)p : 1.0);
                const uint64_t seed = gauss::mix64(1000 * m + (uint64_t)p), elem = big ? ~(uint64_t)0 - 2 : 3;   // counters wrap mod 2^64
                std::vector<int64_t> coset;
                for (uint32_t i = 0; p && i < n; ++i) coset.push_back((int64_t)(gauss::mix64(seed + 77 + i) % (uint64_t)p));
                const std::vector<int64_t> z = alchemy::gen::gaussDecCounter(m, svar, seed, elem, p, p ? &coset : nullptr);
                uint64_t sb;
                std::memcpy(&sb, &svar, sizeof sb);
                std::printf("E %u %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRId64 " |", m, sb, seed, elem, p);
                for (int64_t v : coset) std::printf(" %" PRId64, v);
                std::printf(" |");
                for (int64_t v : z) std::printf(" %" PRId64, v);
                std::printf("\n");
            }
    std::printf("OK\n");
    return 0;
}
