// AddressSanitizer / UndefinedBehaviorSanitizer program for the planner of the general-index engine
// (alchemy_amd/csrc/gen_host.hpp: gen_plan; the kernels of kernel_gen.hpp walk the plan it lays out).  Stand-alone: built and
// run by tests/test_gen_plan_host.py with hipcc (gen_host.hpp pulls in the HIP runtime header); it needs neither the library nor
// a device.
//
// Without arguments it plans every index m = 2^a 3^b 5^c 7^d 11^e 13^f with m != 2 (mod 4) and phi(m) <= 65535 (the bound of
// gen_plan itself; alch_ring_create serves phi(m) * word <= 160 KiB of them) and checks
//   * the plan succeeds within GEN_MAXPASS passes and GEN_MAXFACT factors;
//   * along every prime-power axis the passes' group sizes multiply to the axis length;
//   * stride, axis_stride and axis_len of every pass follow the rule of kernel_gen.hpp: the axis of factor l has stride
//     rts_l = prod_{l' > l} phi(p_l'^e_l') and length phi(p_l^e_l); the i-th pass of an axis has the stride
//     rts_l * dim_l / (r_1 .. r_i), and a two-power block's aux is log2 (r_1 .. r_{i-1});
//   * fdiv -- one mulhi with the plan's own reciprocal -- is exact against `/` for every dividend a kernel can form:
//     w < n / r over stride, base < n over axis_stride, stride over axis_stride (the twiddle step), ap < ceil(n / axis_stride) over
//     axis_len, and the column index c < n / (p - 1) over step = mp * rts with the reciprocal as gen_columns_lds computes it.
//     mulhi(w, rcp) is monotone in w and w / d steps only at the multiples of d, so agreement at w = k d - 1 and w = k d for every
//     k, and at the largest w, is agreement at every w: the check is exhaustive, in a few milliseconds for all indices.
// With indices as arguments it prints their plans (factors and passes) for the driver's structural assertions.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../alchemy_amd/csrc/gen_host.hpp"

using alch::GenHost;
using alch::GenPass;
using alch::u32;
using alch::u64;

static long failed = 0;
static u32 cur_m = 0;
#define EXPECT(...) do { if (!(__VA_ARGS__)) { if (++failed <= 20) printf("FAILED line %d (m = %u): %s\n", __LINE__, cur_m, #__VA_ARGS__); } } while (0)

// fdiv of kernel_gen.hpp on the host: the d == 1 shortcut, else the high word of w * rcp
static u32 fdiv_host(u32 w, u32 d, u32 rcp) { return d == 1 ? w : (u32)(((u64)w * rcp) >> 32); }

// every dividend below `count` (see the header comment for why the multiples of d and their predecessors suffice)
static void check_fdiv(u32 d, u32 rcp, u32 count) {
    EXPECT(d >= 1);
    if (d < 1 || count == 0) return;
    for (u64 kd = 0; kd < count; kd += d) {
        const u32 k = (u32)(kd / d);
        EXPECT(fdiv_host((u32)kd, d, rcp) == k);
        if (kd) EXPECT(fdiv_host((u32)kd - 1, d, rcp) == k - 1);
    }
    EXPECT(fdiv_host(count - 1, d, rcp) == (count - 1) / d);
}

static u32 phi_pp(u32 p, int e) { u32 r = p - 1; for (int t = 1; t < e; ++t) r *= p; return r; }

static void check_index(u32 m, const int (&expo)[6]) {
    static const u32 primes[6] = {2, 3, 5, 7, 11, 13};
    cur_m = m;
    GenHost g;
    const bool ok = alch::gen_plan(m, g);
    EXPECT(ok);
    if (!ok) { printf("  gen_plan(%u): %s\n", m, g.error.c_str()); return; }
    EXPECT(g.npass >= 0 && g.npass <= alch::GEN_MAXPASS);
    EXPECT(g.nfact >= 0 && g.nfact <= alch::GEN_MAXFACT);
    // the factorisation, from the exponents this program chose
    int nf = 0;
    u64 n = 1;
    for (int i = 0; i < 6; ++i) if (expo[i]) { ++nf; n *= phi_pp(primes[i], expo[i]); }
    EXPECT(g.nfact == nf);
    EXPECT((u64)g.n == n);
    u32 rts = g.n;
    int l = 0, ps = 0;
    for (int i = 0; i < 6; ++i) {
        if (!expo[i]) continue;
        const alch::GenFact& f = g.fact[l++];
        const u32 dim = phi_pp(primes[i], expo[i]);
        rts /= dim;
        EXPECT(f.p == (int)primes[i] && f.e == expo[i] && f.dim == dim && f.rts == rts && (u64)f.mp * (primes[i] - 1) == dim);
        // the passes of this axis, in plan order
        u32 done = 1;
        int lg_done = 0, on_axis = 0;
        while (ps < g.npass && g.pass[ps].axis_stride == rts && g.pass[ps].axis_len == dim && done < dim) {
            const GenPass& P = g.pass[ps++];
            ++on_axis;
            EXPECT(P.r >= 2 && P.r <= 13);
            if (primes[i] == 2) {
                EXPECT(P.kind == alch::GK_R2BLOCK && (P.r == 2 || P.r == 4 || P.r == 8) && P.aux == lg_done);
                for (u32 t = (u32)P.r; t > 1; t >>= 1) ++lg_done;
            } else if (on_axis == 1) EXPECT(P.kind == alch::GK_SYM_CRT && P.r == (int)primes[i] - 1 && P.tw_off == 0xffffffffu);
            else EXPECT(P.kind == alch::GK_SYM_DFT && P.r == (int)primes[i] && P.tw_off != 0xffffffffu);
            done *= (u32)P.r;
            EXPECT(dim % done == 0);
            if (dim % done) return;
            EXPECT(P.stride == (dim / done) * rts);
            EXPECT(g.n % (u32)P.r == 0);
            // fdiv at the plan's own reciprocals
            check_fdiv(P.stride, P.rcp_stride, g.n / (u32)P.r);
            check_fdiv(P.axis_stride, P.rcp_axis_stride, g.n);
            EXPECT(fdiv_host(P.stride, P.axis_stride, P.rcp_axis_stride) == P.stride / P.axis_stride && P.stride % P.axis_stride == 0);
            check_fdiv(P.axis_len, P.rcp_axis_len, (g.n - 1) / P.axis_stride + 1);
        }
        EXPECT(done == dim);                                    // the group sizes of the axis multiply to its length
        if (primes[i] != 2) {                                   // the column recurrences (gen_columns_lds)
            const u32 step = f.mp * f.rts, ncol = g.n / (primes[i] - 1);
            const u32 rcp = step > 1 ? (u32)(((u64)1 << 32) / step) + 1u : 0u;
            check_fdiv(step, rcp, ncol);
            EXPECT((u64)(ncol - 1) / step * ((u64)f.dim * f.rts) + (ncol - 1) % step + (u64)(primes[i] - 2) * step == (u64)g.n - 1);   // the last column ends at n - 1
        }
    }
    EXPECT(ps == g.npass && l == g.nfact && rts == 1);
}

static void print_plan(u32 m) {
    GenHost g;
    if (!alch::gen_plan(m, g)) { printf("index %u refused %s\n", m, g.error.c_str()); return; }
    printf("index %u n %u nfact %d npass %d\n", m, g.n, g.nfact, g.npass);
    for (int l = 0; l < g.nfact; ++l)
        printf("fact %d p %d e %d mp %u dim %u rts %u\n", l, g.fact[l].p, g.fact[l].e, g.fact[l].mp, g.fact[l].dim, g.fact[l].rts);
    for (int ps = 0; ps < g.npass; ++ps) {
        const GenPass& P = g.pass[ps];
        const char* kind = P.kind == alch::GK_R2BLOCK ? "R2BLOCK" : P.kind == alch::GK_SYM_CRT ? "SYM_CRT" : P.kind == alch::GK_SYM_DFT ? "SYM_DFT" : "?";
        printf("pass %d kind %s r %d aux %d stride %u axis_stride %u axis_len %u groups %u\n", ps, kind, P.r, P.aux, P.stride, P.axis_stride,
               P.axis_len, g.n / (u32)P.r);
    }
}

int main(int argc, char** argv) {
    if (argc > 1) {
        for (int i = 1; i < argc; ++i) print_plan((u32)strtoul(argv[i], nullptr, 10));
        return 0;
    }
    static const u32 primes[6] = {2, 3, 5, 7, 11, 13};
    const u64 PHI_MAX = 65535, M_MAX = (u64)1 << 31;
    long planned = 0, served32 = 0, served64 = 0;
    int e[6] = {0, 0, 0, 0, 0, 0};
    // every exponent vector, prime by prime; phi(m) > m / 6 for these primes, so m < 2^31 loses nothing
    struct Rec {
        static void go(int i, u64 m, u64 phi, int (&e)[6], long& planned, long& s32, long& s64, u64 PHI_MAX, u64 M_MAX) {
            if (i == 6) {
                if (m % 4 == 2 || m < 3) return;
                check_index((u32)m, e);
                ++planned;
                if (phi * 4 <= 163840) ++s32;
                if (phi * 8 <= 163840) ++s64;
                return;
            }
            u64 mm = m, ph = phi;
            for (int k = 0;; ++k) {
                e[i] = k;
                go(i + 1, mm, ph, e, planned, s32, s64, PHI_MAX, M_MAX);
                ph *= k == 0 ? primes[i] - 1 : primes[i];
                mm *= primes[i];
                if (ph > PHI_MAX || mm >= M_MAX) break;
            }
            e[i] = 0;
        }
    };
    Rec::go(0, 1, 1, e, planned, served32, served64, PHI_MAX, M_MAX);
    // the planner's own limits: one coefficient more than 65535 and a prime above 13 are refused with a message
    {
        GenHost g;
        cur_m = 65537;
        EXPECT(!alch::gen_plan(65537, g) && !g.error.empty());
        cur_m = 17;
        EXPECT(!alch::gen_plan(17, g) && !g.error.empty());
        cur_m = 1u << 17;
        EXPECT(!alch::gen_plan(1u << 17, g) && !g.error.empty());
    }
    printf("planned %ld indices, %ld with phi <= 40960, %ld with phi <= 20480\n", planned, served32, served64);
    printf("OK: %ld failed expectation(s)\n", failed);
    return failed ? 1 : 0;
}
