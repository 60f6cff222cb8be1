// Stand-alone host check of the BaseBGad 2^w bookkeeping the digit loaders, the hint kernel and the host share
// (alchemy_amd/csrc/hint_gadget.hpp): the closed form of the digits (pow2_offset / pow2_digit) against a sequential divModCent in
// __int128, for w = 1 .. 16 and both word types; the layout (counts sum to D, entry() inverts first, 2^(w (k - 1)) < q); the gadget
// codes.  Built with AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_gadget_pow2_host.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../alchemy_amd/csrc/hint_gadget.hpp"

using namespace alch;
typedef __int128 i128;

static long failed = 0;
static void expect(bool ok, const char* what, uint64_t q, uint32_t w, uint64_t x, uint32_t t) {
    if (ok) return;
    if (++failed <= 20) std::printf("FAIL %s: q=%llu w=%u x=%llu t=%u\n", what, (unsigned long long)q, w, (unsigned long long)x, t);
}

static uint64_t splitmix64(uint64_t& s) {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// Lol's divModCent, one digit after the other: remainder in [-b/2, b/2), the top digit absorbs the rest.
static void sequential(i128 v, uint32_t w, uint32_t k, std::vector<i128>& out) {
    const i128 b = (i128)1 << w;
    out.assign(k, 0);
    for (uint32_t t = 0; t < k; ++t) {
        if (t + 1 == k) { out[t] = v; break; }
        i128 r = v % b;
        if (r < 0) r += b;
        if (2 * r >= b) r -= b;
        out[t] = r;
        v = (v - r) / b;
    }
}

template <typename SW>
static void check_word(uint64_t q, uint32_t w, uint64_t x) {
    const uint32_t k = hintgad::digits_pow2(q, w);
    const SW v = x > (q - 1) / 2 ? (SW)((i128)x - (i128)q) : (SW)x;
    std::vector<i128> want;
    sequential((i128)v, w, k, want);
    i128 back = 0;
    for (uint32_t t = k; t-- > 0;) back = back * ((i128)1 << w) + want[t];
    expect(back == (i128)v, "sequential digits recompose", q, w, x, 0);
    for (uint32_t t = 0; t < k; ++t) {
        const SW ct = hintgad::pow2_offset<SW>(w, t);
        const SW d = hintgad::pow2_digit<SW>(v, w, t, t + 1 == k, ct);
        expect((i128)d == want[t], "closed form", q, w, x, t);
        if (t + 1 < k) expect((i128)d >= -((i128)1 << (w - 1)) && (i128)d < ((i128)1 << (w - 1)), "digit range", q, w, x, t);
    }
}

template <typename SW>
static void check_modulus(uint64_t q, bool exhaustive, uint64_t seed) {
    for (uint32_t w = 1; w <= hintgad::MAX_WIDTH; ++w) {
        if (exhaustive) {
            for (uint64_t x = 0; x < q; ++x) check_word<SW>(q, w, x);
            continue;
        }
        const uint64_t ext[] = {0, 1, q - 2, q - 1, (q - 1) / 2, (q + 1) / 2, (q - 3) / 2, (q + 3) / 2};
        for (uint64_t x : ext) check_word<SW>(q, w, x);
        uint64_t s = seed + w;
        for (int i = 0; i < 20000; ++i) check_word<SW>(q, w, splitmix64(s) % q);
    }
}

static void check_layout(const uint64_t* q, int L) {
    for (uint32_t w = 1; w <= hintgad::MAX_WIDTH; ++w) {
        const hintgad::Layout G = hintgad::make_layout_pow2(q, L, w);
        expect(G.w == w && G.L == (uint32_t)L, "layout members", q[0], w, 0, 0);
        uint32_t sum = 0;
        for (int i = 0; i < L; ++i) {
            const uint32_t k = hintgad::digits_pow2(q[i], w);
            expect(G.first[i] == sum, "first", q[i], w, 0, (uint32_t)i);
            sum += k;
            // the smallest k with 2^(w k) >= q, and the top gadget entry below q
            expect(((i128)1 << (w * k)) >= (i128)q[i], "2^(wk) >= q", q[i], w, 0, k);
            expect(k == 1 || ((i128)1 << (w * (k - 1))) < (i128)q[i], "2^(w(k-1)) < q", q[i], w, 0, k);
            for (uint32_t t = 0; t < k; ++t) {
                uint32_t limb, ex;
                hintgad::entry(G, G.first[i] + t, limb, ex);
                expect(limb == (uint32_t)i && ex == t, "entry inverts first", q[i], w, 0, t);
            }
        }
        expect(G.D == sum, "counts sum to D", q[0], w, 0, 0);
        for (int i = L; i <= hintgad::MAX_LIMBS; ++i) expect(G.first[i] == G.D, "first past L", q[0], w, 0, (uint32_t)i);
        if (w == 1) {
            const hintgad::Layout B = hintgad::make_layout(q, L, true);
            bool same = B.D == G.D && B.w == 1;
            for (int i = 0; i <= hintgad::MAX_LIMBS; ++i) same = same && B.first[i] == G.first[i];
            expect(same, "w = 1 is BaseBGad 2", q[0], w, 0, 0);
        }
    }
    expect(hintgad::make_layout(q, L, false).w == 0 && hintgad::make_layout(q, L, false).D == (uint32_t)L, "TrivGad layout", q[0], 0, 0, 0);
}

int main() {
    // gadget codes
    expect(hintgad::gadget_width(0) == 0 && hintgad::gadget_width(1) == 1, "codes 0, 1", 0, 0, 0, 0);
    for (int w = 1; w <= 16; ++w) expect(hintgad::gadget_width(0x100 | w) == w, "BASEPOW2(w)", 0, (uint32_t)w, 0, 0);
    const int bad[] = {2, 7, -1, 0x100, 0x111, 0x1ff, 0x200, 0x201, 0x10001, 0x1101};
    for (int g : bad) expect(hintgad::gadget_width(g) == -1, "unknown code", (uint64_t)(int64_t)g, 0, 0, 0);

    // exhaustive on small moduli, both word types
    const uint64_t small[] = {17, 257, 12289};
    for (uint64_t q : small) { check_modulus<int32_t>(q, true, 0); check_modulus<int64_t>(q, true, 0); }
    // 32-bit words: q < 2^31
    const uint64_t q32[] = {2147483647ull /* largest prime below 2^31 */, 1073741827ull /* first above 2^30 */, 65537, 786433};
    for (uint64_t q : q32) { check_modulus<int32_t>(q, false, q); check_modulus<int64_t>(q, false, q ^ 5); }
    // 64-bit words: q < 2^62
    const uint64_t q64[] = {4611686018427387847ull /* largest prime below 2^62 */, 2147483659ull /* first above 2^31 */};
    for (uint64_t q : q64) check_modulus<int64_t>(q, false, q);

    const uint64_t ring_a[] = {12289, 65537, 2147483647ull};
    const uint64_t ring_b[] = {65537, 4611686018427387847ull, 2147483659ull, 17, 257, 786433, 1073741827ull, 12289};
    check_layout(ring_a, 3);
    check_layout(ring_b, 8);
    check_layout(ring_b, 1);

    std::printf("OK: %ld failed expectation(s)\n", failed);
    return failed ? 1 : 0;
}
