// Stand-alone host check of the scratch planning every chunked walk of the library shares (alchemy_amd/csrc/scratch_plan.hpp):
// scratch_chunk and fused_chunk against the formulas the walks used to spell out one by one, their bounds, that no product wraps, and
// the carve cursor (regions in order, disjoint, the arena used to its last byte, a wrong per-item sum noticed).  Built with
// AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_scratch_plan_host.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../alchemy_amd/csrc/scratch_plan.hpp"

using namespace alch;
typedef unsigned __int128 u128;

static long failed = 0;
static void expect(bool ok, const char* what, size_t a, size_t b, size_t c) {
    if (ok) return;
    if (++failed <= 20) std::printf("FAIL %s: %zu %zu %zu\n", what, a, b, c);
}

static void check_scratch_chunk() {
    const size_t batches[] = {0, 1, 2, 37, (size_t)1 << 20};
    for (int lb = 20; lb <= 36; ++lb) {                                  // budgets 1 MiB .. 64 GiB
        const size_t budget = (size_t)1 << lb;
        std::vector<size_t> pers = {1, 2, 3, 7, 864, 4096, 131072, budget - 1, budget, budget + 1, 2 * budget, 3 * budget + 5};
        for (int lp = 0; lp <= 40; ++lp) { pers.push_back((size_t)1 << lp); pers.push_back(((size_t)1 << lp) + 1); }
        for (size_t per : pers)
            for (size_t batch : batches) {
                const size_t got = scratch_chunk(budget, batch, per);
                // the two spellings of the walks: min outside (do_tunnel, do_ct_mul, ...) and max outside (do_decrypt, do_pt_mul, ...)
                expect(got == std::min(batch, std::max<size_t>(1, budget / per)), "min(batch, max(1, budget / per))", budget, batch, per);
                if (batch >= 1) expect(got == std::max<size_t>(1, std::min<size_t>(batch, budget / per)), "max(1, min(batch, budget / per))", budget, batch, per);
                if (batch >= 1) expect(got >= 1, "at least one item", budget, batch, per);
                expect(got <= batch, "at most the batch", budget, batch, per);
                const u128 arena = (u128)got * per;                      // what the walk reserves
                expect(got == 1 || arena <= budget, "within the budget unless alone", budget, batch, per);
                expect(arena == (u128)(size_t)(got * per), "chunk * per_item does not wrap", budget, batch, per);
            }
    }
    // alch_buf_gauss_dec's rule, 2^27 doubles per chunk, is the 1 GiB budget over 8 n bytes per element
    for (size_t n = 1; n <= 70000; n += (n < 64 ? 1 : 997))
        expect(scratch_chunk((size_t)1 << 30, (size_t)1 << 40, n * sizeof(double)) == std::max<size_t>(1, ((size_t)1 << 27) / n), "2^27 / n", n, 0, 0);
}

static void check_fused_chunk() {
    const size_t batches[] = {1, 7, 8, 9, 1025}, ring_chunks[] = {8, 1024};
    for (int lp = 11; lp <= 33; ++lp)                                    // pair_bytes 2 KiB .. 8 GiB
        for (size_t pair : {(size_t)1 << lp, ((size_t)1 << lp) + 4096, ((size_t)3 << lp) / 2})
            for (size_t batch : batches)
                for (size_t rc : ring_chunks) {
                    const size_t got = fused_chunk(rc, pair, batch);
                    const size_t cap = std::max<size_t>(8, (((size_t)1 << 32) - 1) / pair / 8 * 8);
                    expect(got == std::min(std::min(rc, cap), (batch + 7) / 8 * 8), "fused formula", rc, pair, batch);
                    expect(got % 8 == 0 && got >= 8, "a multiple of 8, at least 8", rc, pair, batch);
                    expect(got == 8 || (u128)got * pair < ((u128)1 << 32), "32-bit byte offsets unless one group", rc, pair, batch);
                }
}

static void check_carve() {
    for (size_t chunk : {(size_t)1, (size_t)3, (size_t)64}) {
        const size_t sizes[] = {16, 0, 40, 8, 0};                        // a zero-size region: `fused ? 0 : ...`
        size_t per_ct = 0;
        for (size_t s : sizes) per_ct += s;
        std::vector<char> arena(chunk * per_ct);                         // exactly what a walk reserves: a byte past it trips ASan
        Carve cv(arena.data(), chunk);
        char* prev_end = arena.data();
        unsigned char tag = 1;
        for (size_t s : sizes) {
            char* p = cv.take(s);
            expect(p == prev_end, "regions in layout order, back to back", chunk, s, 0);
            std::memset(p, tag++, chunk * s);
            prev_end = p + chunk * s;
        }
        expect(prev_end == arena.data() + chunk * per_ct, "the last region ends at base + chunk * sum", chunk, per_ct, 0);
        expect(cv.taken_per_item() == per_ct, "taken_per_item is the sum", chunk, per_ct, 0);
        // the comparison every walk makes after its last take: its own per_ct passes, a per_ct off by one region or one byte does not
        expect(cv.matches(per_ct), "the right per_ct matches", chunk, per_ct, 0);
        expect(!cv.matches(per_ct + 8) && !cv.matches(per_ct - 8) && !cv.matches(per_ct + 1) && !cv.matches(0), "a wrong per_ct is a mismatch", chunk, per_ct, 0);
        Carve early(arena.data(), chunk);                                // a walk that forgets its last region
        early.take(16); early.take(0); early.take(40);
        expect(!early.matches(per_ct) && early.matches(56), "a missing region is a mismatch", chunk, per_ct, 0);
        // disjoint: every region still holds its own tag
        const char* q = arena.data();
        tag = 1;
        for (size_t s : sizes) {
            for (size_t i = 0; i < chunk * s; ++i) expect((unsigned char)q[i] == tag, "regions are disjoint", chunk, s, i);
            q += chunk * s;
            ++tag;
        }
    }
    Carve none(nullptr, 5);                                              // a walk with no scratch this call: nothing reserved, nothing taken
    expect(none.take(0) == nullptr && none.taken_per_item() == 0, "zero-size takes on an empty arena", 0, 0, 0);
    // per-item sizes up to 2^40 on chunks the budgets give: the cursor's products stay inside size_t
    for (int lp = 0; lp <= 40; ++lp) {
        const size_t per = (size_t)1 << lp, chunk = scratch_chunk((size_t)64 << 30, (size_t)1 << 20, per);
        expect((u128)chunk * per < ((u128)1 << 63), "cursor advance fits", chunk, per, 0);
    }
}

int main() {
    check_scratch_chunk();
    check_fused_chunk();
    check_carve();
    std::printf("OK: %ld failed expectation(s)\n", failed);
    return failed ? 1 : 0;
}
