// Stand-alone host program (own main, no device, no library): prints what the shared keyed-stream code (alchemy_amd/csrc/chacha_stream.hpp)
// and the keyed host mirror (cycgen.hpp: gaussDecCounter with a key) compute, for tests/test_chacha_host.py to compare with the known
// answers and the Python model value for value.  Built with -fsanitize=address,undefined.  Arguments: the moduli of the R lines.
//
//   V <label> <16 block words, hex>                   the block of a known-answer vector
//   P <domain> <x> <A> <B>                            chacha::pair through the public addressing
//   R <q> <A> <B> <r as 64-bit words> <r as 32-bit words, or - when q >= 2^31>
//                                                     chacha::reduce128; checked here against unsigned __int128 as well
//   E <m> <svar bits> <seed> <elem> <p> | <coset words, or nothing> | <z ...>
//                                                     one whole keyed element of the host mirror
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../alchemy_amd/host/cycgen.hpp"

using namespace alch;

static void block_line(const char* label, const chacha::Key& K, uint64_t counter, uint64_t nonce) {
    uint64_t u[8];
    chacha::block(K, counter, nonce, u);
    std::printf("V %s", label);
    for (int t = 0; t < 8; ++t) std::printf(" %08x %08x", (unsigned)(uint32_t)u[t], (unsigned)(uint32_t)(u[t] >> 32));
    std::printf("\n");
}

static int reduce_line(uint64_t q, uint64_t A, uint64_t B) {
    const uint64_t want = (uint64_t)((((unsigned __int128)B << 64) | A) % q);
    const uint64_t r64 = chacha::reduce128(A, B, chacha::make_mod64(q));
    std::printf("R %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64, q, A, B, r64);
    int bad = r64 != want;
    if (q < ((uint64_t)1 << 31)) {
        const uint32_t r32 = chacha::reduce128(A, B, chacha::make_mod32((uint32_t)q));
        std::printf(" %u\n", (unsigned)r32);
        bad |= r32 != want;
    } else {
        std::printf(" -\n");
    }
    return bad;
}

int main(int argc, char** argv) {
    uint8_t kb[32];
    for (int i = 0; i < 32; ++i) kb[i] = (uint8_t)i;
    const chacha::Key rfc = chacha::load_key(kb);
    uint8_t zb[32] = {0};
    const chacha::Key zero = chacha::load_key(zb);
    block_line("rfc8439", rfc, chacha::block_counter(9, 4), 0x000000004a000000ull);
    block_line("zero0", zero, chacha::block_counter(0, 0), 0);
    block_line("zero1", zero, chacha::block_counter(0, 4), 0);
    for (uint64_t x = 3; x < 9; ++x) {
        uint64_t A, B;
        chacha::pair(rfc, 0x000000004a000000ull, 9, x, A, B);
        std::printf("P 9 %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", x, A, B);
    }
    {
        uint64_t A, B;
        chacha::pair(rfc, 77, 3, chacha::X_END - 1, A, B);
        std::printf("P 3 %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", chacha::X_END - 1, A, B);
    }

    int bad = 0;
    const uint64_t edge[3] = {0, 1, ~(uint64_t)0};
    for (int a = 1; a < argc; ++a) {
        const uint64_t q = std::strtoull(argv[a], nullptr, 10);
        for (uint64_t A : edge)
            for (uint64_t B : edge) bad |= reduce_line(q, A, B);
        for (uint64_t i = 0; i < 24; ++i) bad |= reduce_line(q, gauss::mix64(q + 2 * i), gauss::mix64(q + 2 * i + 1));
        // uniform_word is the same value whichever word type serves q
        uint64_t A, B;
        chacha::pair(rfc, 5, chacha::DOM_ENCRYPT, 1234567, A, B);
        bad |= chacha::uniform_word(rfc, 5, chacha::DOM_ENCRYPT, 1234567, q) != (uint64_t)((((unsigned __int128)B << 64) | A) % q);
    }
    if (bad) { std::printf("MISMATCH against unsigned __int128\n"); return 1; }

    const uint32_t ms[] = {16, 9, 21};
    const int64_t ps[] = {0, 2, 7};
    uint8_t key[32];
    for (int i = 0; i < 32; ++i) key[i] = (uint8_t)(200 - 5 * i);
    for (uint32_t m : ms)
        for (int64_t p : ps)
            for (int big = 0; big < 2; ++big) {
                const uint32_t n = alchemy::gen::totient(m);
                const double svar = (big ? 5.0 * 1024.0 : 3.0) / std::sqrt((double)n) * (p ? (double)p * (double)p : 1.0);
                const uint64_t seed = gauss::mix64(1000 * m + (uint64_t)p);
                const uint64_t elem = big ? chacha::X_END / n - 1 : 3;          // the last element whose positions stay below 2^58
                std::vector<int64_t> coset;
                for (uint32_t i = 0; p && i < n; ++i) coset.push_back((int64_t)(gauss::mix64(seed + 77 + i) % (uint64_t)p));
                const std::vector<int64_t> z = alchemy::gen::gaussDecCounter(m, svar, seed, elem, p, p ? &coset : nullptr, key);
                uint64_t sb;
                std::memcpy(&sb, &svar, sizeof sb);
                std::printf("E %u %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRId64 " |", m, sb, seed, elem, p);
                for (int64_t v : coset) std::printf(" %" PRId64, v);
                std::printf(" |");
                for (int64_t v : z) std::printf(" %" PRId64, v);
                std::printf("\n");
            }
    // one element further is refused
    bool refused = false;
    try { alchemy::gen::gaussDecCounter(16, 3.0, 1, chacha::X_END / 8, 0, nullptr, key); } catch (const std::exception&) { refused = true; }
    if (!refused) { std::printf("the element past 2^58 was not refused\n"); return 1; }
    std::printf("OK\n");
    return 0;
}
