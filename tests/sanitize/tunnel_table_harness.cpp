// AddressSanitizer / UndefinedBehaviorSanitizer program for the index tables of a general-index ring tunnel
// (alchemy_amd/csrc/gen_host.hpp: gen_tunnel_table; alch_tunnel_create uploads them, k_tunnel_gather, k_tunnel_lin, k_hint_mac_e / _v,
// k_tunnel_mac_e and k_gen_tunnel_ks read through them; alch_pt_linear_create shares the first).  Stand-alone: built and run by
// tests/test_tunnel_table_host.py with hipcc (gen_host.hpp pulls in the HIP runtime header); it needs neither the library nor a device.
//
// Without arguments it walks every ordered pair r' != s' of indices 2^a 3^b 5^c 7^d 11^e 13^f (m >= 3, m != 2 mod 4) with both
// phi <= PHI_MAX for which gen_plan succeeds on r', s' and e' = gcd(r', s'), builds the tables with table_e and slot_e, and checks
//   * d_rel phi(e') = phi(r');
//   * every entry of `table` is -1 or below phi(r'); the rows together hit every position of R' exactly once (so the non-negative
//     entries of a row are distinct);
//   * row i of `table` has exactly phi(e') non-negative entries, and in ascending position they are table_e[i][0 .. phi(e') - 1]
//     (embedPow keeps the order of the mixed-radix index: both rings list their primes ascending);
//   * every slot_e[s] < phi(e'), and every E' slot has exactly phi(s') / phi(e') preimages;
//   * the unit of Z_s'^* behind slot s, reduced mod e', is the unit behind slot slot_e[s] of E' (embedCRT by its definition, with the
//     slot rule of include/alchemy_hip.h restated here);
//   * linv_skip_mask has bit l set exactly when prime l of r' divides e'.
// The table of one pair has d_rel phi(s') entries (phi(r') phi(s') where e' = 1), so PHI_MAX bounds the run time quadratically.
//
// With pairs "r:s" as arguments it prints what alch_tunnel_create and do_tunnel decide from the pair alone, at 4-byte words and default
// options: the dimensions, d_rel, whether E' gets a ring of its own, pieces_ok, dec_c0, and the instantiation of the fused kernel
// (NG under tunnel_fused = 4, NP) or "none".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../alchemy_amd/csrc/gen_host.hpp"

using alch::GenHost;
using alch::u32;
using alch::u64;

#ifndef PHI_MAX
#define PHI_MAX 2048
#endif

static long failed = 0;
static u32 cur_r = 0, cur_s = 0;
#define EXPECT(...) do { if (!(__VA_ARGS__)) { if (++failed <= 20) printf("FAILED line %d (%u -> %u): %s\n", __LINE__, cur_r, cur_s, #__VA_ARGS__); } } while (0)

static u32 gcd32(u32 a, u32 b) { while (b) { const u32 t = a % b; a = b; b = t; } return a; }

struct Tables {
    GenHost ge, gr, gs;
    u32 d_rel = 0, mask = 0;
    std::vector<int32_t> table, table_e;
    std::vector<u32> slot_e;
};

static bool build(u32 rp, u32 sp, Tables& T) {
    const u32 ep = gcd32(rp, sp);
    if (!alch::gen_plan(ep, T.ge) || !alch::gen_plan(rp, T.gr) || !alch::gen_plan(sp, T.gs)) return false;
    return alch::gen_tunnel_table(T.ge, T.gr, T.gs, T.d_rel, T.table, T.mask, &T.table_e, &T.slot_e);
}

// The unit u of Z_m^* behind CRT slot sl, by the slot rule of include/alchemy_hip.h (first factor outermost; within a factor
// s = (i0 - 1) p^(e-1) + digitrev(i1) stands for the unit i0 + p i1 mod p^e), as residues mod every prime power: unit[l] for factor l.
static void slot_units(const GenHost& g, u32 sl, u32 (&unit)[alch::GEN_MAXFACT]) {
    for (int l = 0; l < g.nfact; ++l) {
        const alch::GenFact& f = g.fact[l];
        const u32 s = (sl / f.rts) % f.dim;
        const u32 i0 = s / f.mp + 1, i1 = alch::h_digitrev(s % f.mp, (u32)f.p, f.e - 1);
        unit[l] = (i0 + (u32)f.p * i1) % (f.mp * (u32)f.p);
    }
}

static void check_pair(u32 rp, u32 sp, std::vector<u32>& hits, std::vector<u32>& pre) {
    cur_r = rp; cur_s = sp;
    Tables T;
    const bool ok = build(rp, sp, T);
    EXPECT(ok);
    if (!ok) return;
    const u32 n_e = T.ge.n, n_r = T.gr.n, n_s = T.gs.n, d = T.d_rel;
    EXPECT((u64)d * n_e == n_r);
    EXPECT(T.table.size() == (size_t)d * n_s && T.table_e.size() == (size_t)d * n_e && T.slot_e.size() == n_s);
    if ((u64)d * n_e != n_r || T.table.size() != (size_t)d * n_s || T.table_e.size() != (size_t)d * n_e || T.slot_e.size() != n_s) return;
    hits.assign(n_r, 0);
    for (u32 i = 0; i < d; ++i) {
        u32 k = 0;
        bool row_ok = true;
        for (u32 pos = 0; pos < n_s; ++pos) {
            const int32_t v = T.table[(size_t)i * n_s + pos];
            if (v == -1) continue;
            if (v < 0 || (u32)v >= n_r) { row_ok = false; continue; }
            ++hits[(u32)v];
            if (k >= n_e || T.table_e[(size_t)i * n_e + k] != v) row_ok = false;
            ++k;
        }
        EXPECT(row_ok);
        EXPECT(k == n_e);
    }
    bool once = true;
    for (u32 p = 0; p < n_r; ++p) once = once && hits[p] == 1;
    EXPECT(once);
    EXPECT(n_s % n_e == 0);
    pre.assign(n_e, 0);
    bool below = true;
    for (u32 s = 0; s < n_s; ++s) { if (T.slot_e[s] < n_e) ++pre[T.slot_e[s]]; else below = false; }
    EXPECT(below);
    bool even = true;
    for (u32 t = 0; t < n_e; ++t) even = even && pre[t] == n_s / n_e;
    EXPECT(even);
    // embedCRT: the unit behind slot s of S', reduced mod e', is the unit behind slot slot_e[s] of E'
    bool units = below;
    for (u32 s = 0; s < n_s && units; ++s) {
        u32 us[alch::GEN_MAXFACT], ue[alch::GEN_MAXFACT];
        slot_units(T.gs, s, us);
        slot_units(T.ge, T.slot_e[s], ue);
        for (int le = 0; le < T.ge.nfact; ++le)
            for (int l = 0; l < T.gs.nfact; ++l)
                if (T.gs.fact[l].p == T.ge.fact[le].p) units = units && us[l] % (T.ge.fact[le].mp * (u32)T.ge.fact[le].p) == ue[le];
    }
    EXPECT(units);
    u32 want = 0;
    for (int l = 0; l < T.gr.nfact; ++l) if (T.ge.m % (u32)T.gr.fact[l].p == 0) want |= 1u << l;
    EXPECT(T.mask == want);
}

static bool two_power_engine(u32 m) { return m >= 32 && (m & (m - 1)) == 0; }     // alchemy_hip.hip: such an index gets no general-index ring

static void print_pair(u32 rp, u32 sp) {
    cur_r = rp; cur_s = sp;
    Tables T;
    if (rp == sp || !build(rp, sp, T)) { printf("pair %u %u refused\n", rp, sp); return; }
    const u32 n_e = T.ge.n, n_s = T.gs.n, word = 4;
    // alch_tunnel_create: E' smaller than S', served by alch_ring_create as a general-index ring, both dimensions a multiple of 4
    const bool e_ring = T.ge.m != sp && !two_power_engine(T.ge.m) && (size_t)n_e * word <= 163840 && n_e % 4 == 0 && n_s % 4 == 0;
    bool pieces_ok = e_ring;
    if (e_ring)
        for (size_t k = 0; k + 3 < T.slot_e.size(); k += 4)
            if (T.slot_e[k] % 4 || T.slot_e[k + 1] != T.slot_e[k] + 1 || T.slot_e[k + 2] != T.slot_e[k] + 2 || T.slot_e[k + 3] != T.slot_e[k] + 3) { pieces_ok = false; break; }
    // do_tunnel
    const bool dec_c0 = T.gr.rad > 1 && T.mask != ((1u << T.gr.nfact) - 1);
    const bool fused = e_ring && pieces_ok && n_s % 4 == 0 && n_e % 4 == 0 && n_s <= (u32)(alch::GEN_TUN_T * 4 * 6) && 2 * (size_t)n_e * word <= 65536;
    const int ng = 4 * (size_t)n_e * word <= 65536 ? 4 : 2;
    const u32 pieces = (n_s / 4 + alch::GEN_TUN_T - 1) / alch::GEN_TUN_T;             // gen_launch_tunnel_ks
    const int np = pieces <= 3 ? 3 : pieces <= 5 ? 5 : 6;
    printf("pair %u %u ep %u phi_r %u phi_s %u phi_e %u d_rel %u e_ring %d pieces_ok %d dec_c0 %d ", rp, sp, T.ge.m, T.gr.n, n_s, n_e, T.d_rel,
           e_ring ? 1 : 0, pieces_ok ? 1 : 0, dec_c0 ? 1 : 0);
    if (fused) printf("fused %d/%d\n", ng, np);
    else printf("fused none\n");
}

int main(int argc, char** argv) {
    if (argc > 1) {
        for (int i = 1; i < argc; ++i) {
            unsigned rp = 0, sp = 0;
            if (sscanf(argv[i], "%u:%u", &rp, &sp) != 2) { printf("bad argument %s\n", argv[i]); return 2; }
            print_pair(rp, sp);
        }
        return 0;
    }
    static const u32 primes[6] = {2, 3, 5, 7, 11, 13};
    std::vector<u32> idx;
    struct Rec {
        static void go(int i, u64 m, u64 phi, std::vector<u32>& idx) {
            if (i == 6) { if (m >= 3 && m % 4 != 2) idx.push_back((u32)m); return; }
            u64 mm = m, ph = phi;
            for (int k = 0;; ++k) {
                go(i + 1, mm, ph, idx);
                ph *= k == 0 ? primes[i] - 1 : primes[i];
                mm *= primes[i];
                if (ph > PHI_MAX) break;
            }
        }
    };
    Rec::go(0, 1, 1, idx);
    long pairs = 0, e_one = 0, e_is_s = 0, e_is_r = 0;
    std::vector<u32> hits, pre;
    for (u32 rp : idx)
        for (u32 sp : idx) {
            if (rp == sp) continue;
            check_pair(rp, sp, hits, pre);
            ++pairs;
            const u32 ep = gcd32(rp, sp);
            e_one += ep == 1; e_is_s += ep == sp; e_is_r += ep == rp;
        }
    printf("walked %ld pairs of %zu indices with phi <= %d: %ld with e' = 1, %ld with e' = s', %ld with e' = r'\n", pairs, idx.size(), (int)PHI_MAX,
           e_one, e_is_s, e_is_r);
    printf("OK: %ld failed expectation(s)\n", failed);
    return failed ? 1 : 0;
}
