// Stand-alone host program (own main, no device, no library): runs the gadget bookkeeping the hint kernel shares with the host
// (alchemy_amd/csrc/hint_gadget.hpp) against plain loops, and prints what it computed for tests/test_hints_host.py to compare with
// Python integers.  Built with -fsanitize=address,undefined.
//
//   G <bits> <L> <gadget> <D> | <q_0 .. q_{L-1}> | <first_0 .. first_L>     one layout; every entry checked against the nested loop here
//   P <pair> <L> <j> <n> <k> <pos>                                          one counter of a uniform word
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "../../alchemy_amd/csrc/hint_gadget.hpp"

using namespace alch;

static void die(const char* what, unsigned bits, int L, int gadget, uint32_t t) {
    std::printf("MISMATCH %s bits %u L %d gadget %d entry %u\n", what, bits, L, gadget, t);
    std::exit(1);
}

int main() {
    const unsigned classes[] = {17, 31, 32, 62};
    for (unsigned bits : classes)
        for (int L = 1; L <= 6; ++L)
            for (int gadget = 0; gadget < 2; ++gadget) {
                // moduli of exactly `bits` bits: the smallest (2^(bits-1) + 1: its top digit is 2^(bits-1)), the largest, and odd ones between
                uint64_t q[hintgad::MAX_LIMBS] = {0};
                const uint64_t lo = ((uint64_t)1 << (bits - 1)) + 1, hi = (((uint64_t)1 << (bits - 1)) - 1) * 2 + 1;
                for (int i = 0; i < L; ++i) q[i] = i == 0 ? lo : i == 1 ? hi : lo + 2 * (uint64_t)(977 * i);
                const hintgad::Layout G = hintgad::make_layout(q, L, gadget == 1);
                uint32_t t = 0;
                for (int i = 0; i < L; ++i) {                                   // the plain loop: limb by limb, digit by digit
                    if (G.first[i] != t) die("first", bits, L, gadget, t);
                    uint32_t digits = 1;
                    if (gadget == 1) {
                        digits = 0;
                        while (((unsigned __int128)1 << digits) < q[i]) ++digits;
                        if (digits != bits) die("digit count", bits, L, gadget, t);
                    }
                    for (uint32_t d = 0; d < digits; ++d, ++t) {
                        uint32_t limb = ~0u, ex = ~0u;
                        hintgad::entry(G, t, limb, ex);
                        if (limb != (uint32_t)i || ex != d) die("entry", bits, L, gadget, t);
                        if (((uint64_t)1 << ex) >= q[i]) die("2^d < q", bits, L, gadget, t);
                    }
                }
                if (t != G.D || G.L != (uint32_t)L) die("total", bits, L, gadget, t);
                for (int i = L; i <= hintgad::MAX_LIMBS; ++i)
                    if (G.first[i] != G.D) die("tail", bits, L, gadget, (uint32_t)i);
                std::printf("G %u %d %d %u |", bits, L, gadget, G.D);
                for (int i = 0; i < L; ++i) std::printf(" %" PRIu64, q[i]);
                std::printf(" |");
                for (int i = 0; i <= L; ++i) std::printf(" %u", G.first[i]);
                std::printf("\n");
            }

    // counters: position (2 pair + 1, j, k) of an [element][L][n] array, mod 2^64, against 128-bit arithmetic
    const uint64_t pairs[] = {0, 1, 5, ((uint64_t)1 << 31) - 1, ((uint64_t)1 << 63) - 1, (uint64_t)1 << 63, ~(uint64_t)0 - 1, ~(uint64_t)0};
    const uint32_t ns[] = {1, 24, 4608, 65536, 0xFFFFFFFFu};
    for (uint64_t pair : pairs)
        for (uint32_t L = 1; L <= 6; ++L)
            for (uint32_t n : ns) {
                const uint32_t j = L - 1, k = n - 1;
                const unsigned __int128 wide = (((unsigned __int128)2 * pair + 1) * L + j) * n + k;
                const uint64_t pos = hintgad::odd_word_pos(pair, L, j, n, k);
                if (pos != (uint64_t)wide) die("counter", 0, (int)L, 0, n);
                if (hintgad::odd_word_pos(pair, L, 0, n, 0) + (uint64_t)j * n + k != pos) die("counter step", 0, (int)L, 0, n);
                std::printf("P %" PRIu64 " %u %u %u %u %" PRIu64 "\n", pair, L, j, n, k, pos);
            }
    std::printf("OK\n");
    return 0;
}
