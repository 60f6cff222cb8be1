// Hoisted automorphisms (include/alchemy_hip.h, "Hoisted automorphisms"): the gathered hint inner product behind
// alch_ct_automorph_hoisted.  Included from alchemy_hip.hip after kernel_automorph.hpp.
//
// The digits d_t of s_pre c1 are decomposed and transformed ONCE per ciphertext; sigma_j fixes Z_q, so sigma_j(s_pre c1) =
// sum_t g_t sigma_j(d_t), and on the CRT basis sigma_j only moves slots.  With src_r the slot table of rotation r (automorph_host.hpp):
//   out_r.c0[k] = s_pre c0[src_r[k]] + sum_t crt(d_t)[src_r[k]] b_{r,t}[k]
//   out_r.c1[k] =                      sum_t crt(d_t)[src_r[k]] a_{r,t}[k]
// k_tun2_mac / k_tunnel_mac_e with sh = 0 and d_rel = 1, the digit and c0 words read through the permutation: a lane owns VW
// consecutive destination slots of one limb (16 bytes, or one word where n is no multiple of that), a tile of TILE ciphertexts shares
// the hint words, 32-bit words sum groups of K = lazy_group(q) products in 64 bits per Montgomery reduction (product-at-a-time where
// K < 2 and on 8-byte words).  c0 is read from the caller's CRT-basis input where it lies and scaled on the fly.
//   POW2   radix-16 engine: no table.  The aligned pack of VW destination slots reads one aligned pack of VW source slots
//          (automorph::pow2_pack); its address and the VW picks are computed once per (item, rotation) and serve c0, all D digits and
//          all TILE ciphertexts, so every access stays a 16-byte one.
//   !POW2  general engine: the VW table entries of the piece come with one load from the cached device table; one word per slot
//          per digit is gathered.
// Rotations r0 .. r0 + nrot - 1 of the set are accumulated into ONE output batch: nrot = 1 is a single rotation (one launch per
// rotation over the shared digits), nrot = R the sum form sum_r out_r, whose lazy groups run across the flattened (rotation, digit)
// sequence.  The set's pointers and units travel by value, hence HOIST_MAX.
#pragma once
#include "automorph_host.hpp"

namespace alch {

constexpr int HOIST_MAX = 32;

template <typename W>
struct HoistSet {
    const W* hint[HOIST_MAX];      // rotation r: [2 D][L][n], Montgomery form
    const u32* tab[HOIST_MAX];     // general engine: device slot table of sigma_(j_r)
    u32 j[HOIST_MAX];              // reduced mod m
};

template <typename W, int VW, int TILE, bool POW2>
__global__ void __launch_bounds__(256) k_hoist_mac(DevRing<W> R, W* out, const W* digits, const W* cin, size_t nct, u32 D, HoistSet<W> S, u32 r0,
                                                   u32 nrot, int logn, Scal<W> s_m, int scale) {
    typedef Pack<W, VW> P;
    typedef Pack<u32, VW> T;
    static_assert(!POW2 || VW == Vec4<W>::LANES, "the closed form serves whole 16-byte packs");
    const size_t n = (size_t)R.n;
    const size_t Ln = (size_t)R.L * n;
    const size_t ntile = (nct + TILE - 1) / TILE;
    const u32 nv = R.n / VW;
    ALCH_WALK_INIT(nv, R.L);
    ALCH_WALK(w, ntile * (size_t)R.L * nv, wk) {
        const size_t ct0 = wk.outer * TILE, rem = (size_t)wk.mid * n + (size_t)wk.k * VW;
        const u32 limb = wk.mid;
        const ModP<W> m = R.mod[limb];
        const W q = m.q, qni = m.qni;
        bool lazy = false;
        u32 K = 0;
        if constexpr (sizeof(W) == 4) {
            K = lazy_group((u32)q);                                // (K + 2) q < 2^32
            lazy = K >= 2;
        }
        const u64 r1 = lazy ? (u64)m.r1 : 1;                       // not lazy: the accumulators hold the running sum itself, in [0, q)
        u64 a0[TILE][VW], a1[TILE][VW];
        W c0s[TILE][VW];                                           // sum_r s_pre c0[src_r[k]], in [0, q): kept out of the lazy groups
        const W *dv[TILE], *cv[TILE];
#pragma unroll
        for (int c = 0; c < TILE; ++c) {
            const size_t ct = ct0 + c < nct ? ct0 + c : ct0;       // a dead lane of the tile recomputes ciphertext ct0 and stores nothing
            dv[c] = digits + (ct * (size_t)D * R.L + limb) * n;
            cv[c] = cin + (2 * ct * (size_t)R.L + limb) * n;
#pragma unroll
            for (int e = 0; e < VW; ++e) { a0[c][e] = 0; a1[c][e] = 0; c0s[c][e] = 0; }
        }
        const size_t dstep = (size_t)R.L * n;
        u32 grp = 0;                                               // products in the open lazy group
        for (u32 r = r0; r < r0 + nrot; ++r) {
            // where this piece reads: one aligned pack and VW picks (closed form), or VW table entries
            u32 at[VW], pack = 0;
            if constexpr (POW2) {
                pack = automorph::pow2_pack<VW>(wk.k * (u32)VW, S.j[r], logn, at);
            } else {
                const T t = reinterpret_cast<const T*>(S.tab[r])[wk.k];
#pragma unroll
                for (int e = 0; e < VW; ++e) at[e] = t.v[e];
            }
            auto fetch = [&](const W* poly) -> P {
                P x;
                if constexpr (POW2) {
                    const P p = *reinterpret_cast<const P*>(poly + pack);
#pragma unroll
                    for (int e = 0; e < VW; ++e) x.v[e] = automorph_pick<W, VW>(p, at[e]);
                } else {
#pragma unroll
                    for (int e = 0; e < VW; ++e) x.v[e] = poly[at[e]];
                }
                return x;
            };
            const W* hint = S.hint[r];
#pragma unroll
            for (int c = 0; c < TILE; ++c) {
                const P x = fetch(cv[c]);
#pragma unroll
                for (int e = 0; e < VW; ++e) c0s[c][e] = add_mod(c0s[c][e], scale ? mont_mul(x.v[e], s_m.v[limb], m) : x.v[e], q);
            }
            for (u32 d = 0; d < D; ++d) {
                const P h0 = *reinterpret_cast<const P*>(hint + (size_t)(2 * d) * Ln + rem);
                const P h1 = *reinterpret_cast<const P*>(hint + (size_t)(2 * d + 1) * Ln + rem);
                if (lazy) {
                    if constexpr (sizeof(W) == 4) {
                        if (grp == K) {                            // carry the running sum into the next group: t (R mod q) < 2 q^2
#pragma unroll
                            for (int c = 0; c < TILE; ++c)
#pragma unroll
                                for (int e = 0; e < VW; ++e) {
                                    a0[c][e] = (u64)mont_red_lazy(a0[c][e], (u32)q, (u32)qni) * r1;
                                    a1[c][e] = (u64)mont_red_lazy(a1[c][e], (u32)q, (u32)qni) * r1;
                                }
                            grp = 0;
                        }
                        ++grp;
#pragma unroll
                        for (int c = 0; c < TILE; ++c) {
                            const P x = fetch(dv[c] + (size_t)d * dstep);
#pragma unroll
                            for (int e = 0; e < VW; ++e) {
                                a0[c][e] += (u64)x.v[e] * h0.v[e];
                                a1[c][e] += (u64)x.v[e] * h1.v[e];
                            }
                        }
                    }
                } else {
#pragma unroll
                    for (int c = 0; c < TILE; ++c) {
                        const P x = fetch(dv[c] + (size_t)d * dstep);
#pragma unroll
                        for (int e = 0; e < VW; ++e) {
                            a0[c][e] = (u64)add_mod((W)a0[c][e], mont_mul(x.v[e], h0.v[e], m), q);
                            a1[c][e] = (u64)add_mod((W)a1[c][e], mont_mul(x.v[e], h1.v[e], m), q);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int c = 0; c < TILE; ++c) {
            if (ct0 + c >= nct) continue;
            P z0, z1;
#pragma unroll
            for (int e = 0; e < VW; ++e) {
                W s0 = (W)a0[c][e], s1 = (W)a1[c][e];
                if constexpr (sizeof(W) == 4) {
                    if (lazy) {
                        s0 = csub(mont_red_lazy(a0[c][e], (u32)q, (u32)qni), (u32)q);
                        s1 = csub(mont_red_lazy(a1[c][e], (u32)q, (u32)qni), (u32)q);
                    }
                }
                z0.v[e] = add_mod(s0, c0s[c][e], q);
                z1.v[e] = s1;
            }
            *reinterpret_cast<P*>(out + 2 * (ct0 + c) * Ln + rem) = z0;
            *reinterpret_cast<P*>(out + (2 * (ct0 + c) + 1) * Ln + rem) = z1;
        }
    }
}

}  // namespace alch
