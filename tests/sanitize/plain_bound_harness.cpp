// AddressSanitizer / UndefinedBehaviorSanitizer program for the host-only arithmetic of the plaintext-side entry points
// (alchemy_amd/csrc/plain_host.hpp: the coefficient bound of alch_pt_bound and the test Q / 2 > bound of every multiplying call).
// Stand-alone: built and run by tests/test_plaintext_sanitizers.py; it needs neither the library nor a device.
#include <cstdint>
#include <cstdio>

#include "../../alchemy_amd/csrc/plain_host.hpp"

using alch::u128;

static int failed = 0;
#define EXPECT(c) do { if (!(c)) { ++failed; printf("FAILED line %d: %s\n", __LINE__, #c); } } while (0)

int main() {
    u128 b = 0;
    // the formula on the reference's indices: phi and the number of odd primes
    uint64_t phi = 0; int odd = 0;
    alch::pt_index_shape(448, &phi, &odd);   EXPECT(phi == 192 && odd == 1);
    alch::pt_index_shape(20475, &phi, &odd); EXPECT(phi == 8640 && odd == 4);
    alch::pt_index_shape(1, &phi, &odd);     EXPECT(phi == 1 && odd == 0);
    alch::pt_index_shape(4, &phi, &odd);     EXPECT(phi == 2 && odd == 0);
    alch::pt_index_shape(4294967291u, &phi, &odd); EXPECT(phi == 4294967290ull && odd == 1);           // the largest 32-bit prime
    alch::pt_index_shape(3234846615u, &phi, &odd); EXPECT(odd == 9);                                    // 3 5 7 11 13 17 19 23 29
    EXPECT(alch::pt_bound_value(448, 32, 1, &b) && b == (u128)192 * 2 * 256);
    EXPECT(alch::pt_bound_value(91, 7, 6, &b) && b == (u128)6 * 72 * 4 * 9);
    // argument ranges
    EXPECT(!alch::pt_bound_value(0, 32, 1, &b) && !alch::pt_bound_value(448, 1, 1, &b) && !alch::pt_bound_value(448, (uint64_t)1 << 31, 1, &b));
    EXPECT(!alch::pt_bound_value(448, 32, 0, &b) && !alch::pt_bound_value(448, 32, 65537, &b));
    // the extremes stay inside 128 bits: most terms, largest modulus, largest phi, most odd primes
    EXPECT(alch::pt_bound_value(4294967291u, ((uint64_t)1 << 31) - 1, 65536, &b) && (b >> 105) != 0 && (b >> 117) == 0);
    EXPECT(alch::pt_bound_value(3234846615u, ((uint64_t)1 << 31) - 1, 65536, &b) && (b >> 117) == 0);
    const u128 big = b;
    // Q against the bound: one small prime fails, enough limbs pass, and limbs whose full product passes 2^128 do not wrap
    const uint64_t q13[1] = {4481};
    EXPECT(alch::pt_bound_value(448, 32, 1, &b) && !alch::pt_q_exceeds(q13, 1, b));
    const uint64_t q31[2] = {1073741857, 1073742113};
    EXPECT(alch::pt_q_exceeds(q31, 2, b) && !alch::pt_q_exceeds(q31, 0, b));
    const uint64_t q62[8] = {4611686018427387847ull, 4611686018427387817ull, 4611686018427387787ull, 4611686018427387761ull,
                             4611686018427387751ull, 4611686018427387733ull, 4611686018427387709ull, 4611686018427387701ull};
    EXPECT(alch::pt_q_exceeds(q62, 8, b) && alch::pt_q_exceeds(q62, 8, big) && alch::pt_q_exceeds(q62, 2, big) && !alch::pt_q_exceeds(q62, 1, big));
    const uint64_t q30[8] = {1073479681, 1071513601, 1070727169, 1068236801, 1065484289, 1064697857, 1073741857, 1073742113};
    EXPECT(alch::pt_q_exceeds(q30, 8, big) && !alch::pt_q_exceeds(q30, 3, big));
    const uint64_t qz[2] = {0, 5};
    EXPECT(!alch::pt_q_exceeds(qz, 2, b));
    // exact threshold: Q > 2 b, not >=
    const uint64_t qe[2] = {2, 98304};                                                                  // 2 * 98304 = 2 b
    EXPECT(b == 98304 && !alch::pt_q_exceeds(qe, 2, b));
    const uint64_t qo[2] = {2, 98305};
    EXPECT(alch::pt_q_exceeds(qo, 2, b));
    printf("OK: %d failed expectation(s)\n", failed);
    return failed ? 1 : 0;
}
