// AddressSanitizer / UndefinedBehaviorSanitizer program for the lazy accumulator arithmetic of the key-switch kernel
// (alchemy_amd/csrc/modarith.hpp: sub_lazy, and the three expressions kernel_ks_half.hpp builds from it), checked
// against unsigned __int128 arithmetic.  Stand-alone: built and run by tests/test_modarith_lazy.py; it needs neither
// the library nor a device.  sub_lazy, csub and mont_mul_lazy are the header's, which the kernel includes; the accumulate step
// and stage 0 are restated here from kernel_ks_half.hpp.
#include <cstdint>
#include <cstdio>

#include "../../alchemy_amd/csrc/modarith.hpp"

using alch::csub;
using alch::mont_mul_lazy;
using alch::sub_lazy;
using alch::u32;
using alch::u64;
typedef unsigned __int128 u128;

static long failed = 0;
#define EXPECT(c) do { if (!(c)) { if (++failed <= 20) printf("FAILED line %d (q = %u): %s\n", __LINE__, (unsigned)q, #c); } } while (0)

static u64 rng_state = 0x9e3779b97f4a7c15ull;
static u64 rnd() {                                  // splitmix64
    u64 z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// (a - b) mod q for any a, b, in wide arithmetic
static u32 ref_sub(u128 a, u128 b, u32 q) { return (u32)((a % q + q - b % q) % q); }

static void check_modulus(u32 q) {
    const alch::ModP<u32> m = alch::make_modp<u32>(q);
    const u32 q2 = 2u * q, qni = m.qni;
    const u64 rinv = alch::h_powmod(m.r1, (u64)q - 2, q);              // R^-1 mod q: mont_mul_lazy(a, b) = a b R^-1
    EXPECT((u64)q2 == 2 * (u64)q);                                     // 2q fits the word

    // ---- sub_lazy: a, u in [0,2q) -> [0,2q), congruent to a - u
    const u32 corner[7] = {0, 1, q - 1, q, q + 1, q2 - 2, q2 - 1};
    for (u32 a : corner)
        for (u32 u : corner) {
            const u32 d = sub_lazy(a, u, q2);
            EXPECT(d < q2 && d % q == ref_sub(a, u, q));
        }
    for (int it = 0; it < 1000000; ++it) {
        const u64 r = rnd();
        const u32 a = (u32)(r % q2), u = (u32)((r >> 32) % q2);
        const u32 d = sub_lazy(a, u, q2);
        EXPECT(d < q2 && d % q == ref_sub(a, u, q));
    }

    // ---- the accumulate step  acc = sub_lazy(acc, mont_mul_lazy(x, h), 2q):  x ANY word, h < q, acc in [0,2q)
    const u32 xs[6] = {0, q2 - 1, 0xffffffffu, 1, q - 1, q};
    const u32 hs[7] = {0, 1, q - 2, q - 1, (q - 1) / 2, (q + 1) / 2, (u32)(rnd() % q)};
    for (u32 x : xs)
        for (u32 h : hs) {
            const u32 p = mont_mul_lazy(x, h, q, qni);
            EXPECT(p < q2);
            EXPECT(p % q == (u32)((u128)x * h % q * rinv % q));
            for (u32 acc : corner) {
                const u32 r = sub_lazy(acc, p, q2);
                EXPECT(r < q2 && r % q == ref_sub(acc, (u128)x * h % q * rinv, q));
            }
        }
    // with x the transform of the NEGATED digit the step adds d h: the same word as the sum of reduced values it replaces
    for (int it = 0; it < 100000; ++it) {
        const u64 r = rnd();
        const u32 d = (u32)(r % q2), h = (u32)((r >> 32) % q), acc = (u32)(rnd() % q2);
        const u32 xneg = (q2 - d) % q2;                                 // a word in [0,2q) congruent to -d
        EXPECT(xneg < q2 && (xneg % q + d % q) % q == 0);
        const u32 now = csub(sub_lazy(acc, mont_mul_lazy(xneg, h, q, qni), q2), q);
        const u32 was = csub(csub(acc, q) + csub(mont_mul_lazy(d, h, q, qni), q), q);
        EXPECT(now == was);
    }

    // ---- the negated stage 0 of pass G.  w is the twiddle in Montgomery form (any residue, 0 excluded), w' = q - w for the
    // lower half (result -(x + w y)) and w for the upper half (result -(x - w y)); balanced digits have |z| < q.
    const int32_t zs[9] = {0, 1, -1, (int32_t)(q - 1), -(int32_t)(q - 1), (int32_t)((q - 1) / 2), -(int32_t)((q - 1) / 2),
                           (int32_t)((q + 1) / 2), -(int32_t)((q + 1) / 2)};
    // unbalanced: digits of a limb of up to 31 bits (|z| <= 2^30), made non-negative by a multiple of q (DevRing::dig_off)
    const int32_t big = (int32_t)1 << 30;
    const int32_t zg[9] = {0, 1, -1, big, -big, big - 1, -(big - 1), (int32_t)(q % (u32)big), -(int32_t)(q % (u32)big)};
    const u32 off = (u32)(((u64)big + q - 1) / q * q);
    const u32 nr1 = q - m.r1;                                          // -1 in Montgomery form
    EXPECT(nr1 < q && (u64)off + (u64)big < ((u64)1 << 32));
    const u32 ws[4] = {1, q - 1, (q + 1) / 2, (u32)(1 + rnd() % (q - 1))};
    for (u32 w : ws)
        for (int hf = 0; hf < 2; ++hf)
            for (int bal = 0; bal < 2; ++bal)
                for (int ix = 0; ix < 9; ++ix)
                    for (int iy = 0; iy < 9; ++iy) {
                        const int32_t zx = bal ? zs[ix] : zg[ix], zy = bal ? zs[iy] : zg[iy];
                        const u32 w1 = hf ? w : q - w;
                        EXPECT(w1 < q);
                        const u64 wtrue = (u64)w * rinv % q;           // the residue the Montgomery word stands for
                        const u64 x = (u64)(((int64_t)zx % (int64_t)q + q) % q), y = (u64)(((int64_t)zy % (int64_t)q + q) % q);
                        const u64 pos = hf ? (x + q - wtrue * y % q) % q : (x + wtrue * y) % q;
                        const u32 want = (u32)((q - pos) % q);         // the negated stage-0 output
                        u32 xh, yh;
                        if (bal) { xh = q - (u32)zx; yh = q - (u32)zy; }
                        else { xh = mont_mul_lazy((u32)zx + off, nr1, q, qni); yh = mont_mul_lazy((u32)zy + off, nr1, q, qni); }
                        EXPECT(xh < q2 && yh < q2 && (xh % q + x) % q == 0 && (yh % q + y) % q == 0);
                        const u32 u = sub_lazy(xh, mont_mul_lazy(yh, w1, q, qni), q2);
                        EXPECT(u < q2 && u % q == want);
                    }
}

int main() {
    // every modulus the GPU tests of the kernel use (tests/test_gpu_ks_lazy_acc.py), and 12289
    const u32 qs[] = {2147352577u, 2146959361u, 2146041857u, 2145976321u,                                         // CFG3_QS
                      2147389441u, 2147377153u, 2147295233u, 2147217409u, 2147205121u, 2147196929u, 2147082241u,  // EIGHT_QS
                      65537u, 786433u,                                                                            // UNBAL_QS
                      2144468993u, 2142502913u,                                                                   // SIX_QS[:5]
                      12289u};
    for (u32 q : qs) check_modulus(q);
    printf("OK: %ld failed expectation(s)\n", failed);
    return failed ? 1 : 0;
}
