// Slot-wise linear maps (include/alchemy_hip.h, "Weighted sums of hoisted rotations"): the kernel behind
// alch_ct_automorph_lincomb.  Included from alchemy_hip.hip after kernel_hoist.hpp.
//
//   out[g batch + b].c_i[k] = sum_r w[g R + r][k] y_r[b].c_i[k]   (mod q_limb),   y_r = rotation r as k_hoist_mac stores it
//
// y_r does not depend on the row g: per rotation a lane runs k_hoist_mac's gathered inner product for ONE rotation -- the same piece
// addressing (POW2 closed form / table), the same lazy groups over the D digits, opened afresh for every rotation, reduced to [0, q)
// and the scaled c0 term added -- and multiplies the value into up to ROWS row accumulators that stay in registers; the R rotations
// never reach memory.  A call with more rows walks them in blocks of ROWS (lincomb_blocks; the inner products are redone per block:
// the price of not storing y_r).  The weights are canonical residues, not in Montgomery form: the products y w are summed as they
// are and the one factor R^-1 of the closing reduction is taken out by R^2 mod q (lincomb_step / lincomb_close in modarith.hpp; where
// K < 2 and on 8-byte words one Montgomery product at a time, closed by the same R^2).
//
// LINCOMB_ROWS / LINCOMB_TILE from the compiler's resource report (DESIGN section 24 has the table): no instantiation uses scratch.
// The part above the __HIPCC__ guard needs standard headers only: a host compiler reads it in tests/sanitize/lincomb_harness.cpp.
#pragma once
#include <cstddef>
#if defined(__HIPCC__)
#include "kernel_hoist.hpp"
#endif

namespace alch {

constexpr int LINCOMB_ROWS = 4;      // row accumulators per lane
constexpr int LINCOMB_TILE = 2;      // ciphertexts that share the hint and weight words of a lane

// Row blocks of a call: block i covers rows [i ROWS, min(n_out, (i + 1) ROWS)).  Host-callable (tests/sanitize/lincomb_harness.cpp).
inline size_t lincomb_blocks(size_t n_out, size_t rows) { return (n_out + rows - 1) / rows; }
inline size_t lincomb_block_rows(size_t n_out, size_t rows, size_t i) { return n_out - i * rows < rows ? n_out - i * rows : rows; }

#if defined(__HIPCC__)
// wts: row 0 of the block, [row][R][L][n]; out: row 0 of the block at the chunk's first ciphertext, rows `ostride` words apart.
template <typename W, int VW, int TILE, bool POW2, int ROWS>
__global__ void __launch_bounds__(256) k_hoist_lincomb(DevRing<W> R, W* out, const W* digits, const W* cin, size_t nct, u32 D, HoistSet<W> S, u32 nrot,
                                                       int logn, Scal<W> s_m, int scale, const W* wts, u32 nrows, size_t ostride) {
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
        const u64 r1 = lazy ? (u64)m.r1 : 1;
        u64 z0[ROWS][TILE][VW], z1[ROWS][TILE][VW];                // the row accumulators: 64-bit sums (lazy) or values in [0, q)
        const W *dv[TILE], *cv[TILE];
#pragma unroll
        for (int c = 0; c < TILE; ++c) {
            const size_t ct = ct0 + c < nct ? ct0 + c : ct0;       // a dead lane of the tile recomputes ciphertext ct0 and stores nothing
            dv[c] = digits + (ct * (size_t)D * R.L + limb) * n;
            cv[c] = cin + (2 * ct * (size_t)R.L + limb) * n;
        }
#pragma unroll
        for (int g = 0; g < ROWS; ++g)
#pragma unroll
            for (int c = 0; c < TILE; ++c)
#pragma unroll
                for (int e = 0; e < VW; ++e) { z0[g][c][e] = 0; z1[g][c][e] = 0; }
        const size_t dstep = (size_t)R.L * n;
        u32 wgrp = 0;                                              // weighted products in the open lazy group of the rows
        for (u32 r = 0; r < nrot; ++r) {
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
            // ---- y_r of the tile: k_hoist_mac's inner product for this one rotation
            const W* hint = S.hint[r];
            u64 a0[TILE][VW], a1[TILE][VW];
#pragma unroll
            for (int c = 0; c < TILE; ++c)
#pragma unroll
                for (int e = 0; e < VW; ++e) { a0[c][e] = 0; a1[c][e] = 0; }
            u32 grp = 0;
            for (u32 d = 0; d < D; ++d) {
                const P h0 = *reinterpret_cast<const P*>(hint + (size_t)(2 * d) * Ln + rem);
                const P h1 = *reinterpret_cast<const P*>(hint + (size_t)(2 * d + 1) * Ln + rem);
                if (lazy) {
                    if constexpr (sizeof(W) == 4) {
                        if (grp == K) {
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
            W y0[TILE][VW], y1[TILE][VW];
#pragma unroll
            for (int c = 0; c < TILE; ++c) {
                const P x = fetch(cv[c]);
#pragma unroll
                for (int e = 0; e < VW; ++e) {
                    W s0 = (W)a0[c][e], s1 = (W)a1[c][e];
                    if constexpr (sizeof(W) == 4) {
                        if (lazy) {
                            s0 = csub(mont_red_lazy(a0[c][e], (u32)q, (u32)qni), (u32)q);
                            s1 = csub(mont_red_lazy(a1[c][e], (u32)q, (u32)qni), (u32)q);
                        }
                    }
                    y0[c][e] = add_mod(s0, scale ? mont_mul(x.v[e], s_m.v[limb], m) : x.v[e], q);
                    y1[c][e] = s1;
                }
            }
            // ---- into the rows
            bool carry = false;
            if (lazy) {
                carry = wgrp == K;
                if (carry) wgrp = 0;
                ++wgrp;
            }
#pragma unroll
            for (int g = 0; g < ROWS; ++g) {
                if ((u32)g >= nrows) break;
                const P wv = *reinterpret_cast<const P*>(wts + ((size_t)g * nrot + r) * Ln + rem);
#pragma unroll
                for (int c = 0; c < TILE; ++c)
#pragma unroll
                    for (int e = 0; e < VW; ++e) {
                        if constexpr (sizeof(W) == 4) {
                            if (lazy) {
                                z0[g][c][e] = lincomb_step(z0[g][c][e], carry, (u32)y0[c][e], (u32)wv.v[e], (u32)q, (u32)qni, (u32)r1);
                                z1[g][c][e] = lincomb_step(z1[g][c][e], carry, (u32)y1[c][e], (u32)wv.v[e], (u32)q, (u32)qni, (u32)r1);
                                continue;
                            }
                        }
                        z0[g][c][e] = (u64)add_mod((W)z0[g][c][e], mont_mul(y0[c][e], wv.v[e], m), q);
                        z1[g][c][e] = (u64)add_mod((W)z1[g][c][e], mont_mul(y1[c][e], wv.v[e], m), q);
                    }
            }
        }
#pragma unroll
        for (int g = 0; g < ROWS; ++g) {
            if ((u32)g >= nrows) break;
#pragma unroll
            for (int c = 0; c < TILE; ++c) {
                if (ct0 + c >= nct) continue;
                P o0, o1;
#pragma unroll
                for (int e = 0; e < VW; ++e) {
                    if constexpr (sizeof(W) == 4) {
                        if (lazy) {
                            o0.v[e] = lincomb_close(z0[g][c][e], (u32)q, (u32)qni, (u32)m.r2);
                            o1.v[e] = lincomb_close(z1[g][c][e], (u32)q, (u32)qni, (u32)m.r2);
                            continue;
                        }
                    }
                    o0.v[e] = mont_mul((W)z0[g][c][e], m.r2, m);   // the products carried one R^-1 each
                    o1.v[e] = mont_mul((W)z1[g][c][e], m.r2, m);
                }
                W* po = out + (size_t)g * ostride + 2 * (ct0 + c) * Ln + rem;
                *reinterpret_cast<P*>(po) = o0;
                *reinterpret_cast<P*>(po + Ln) = o1;
            }
        }
    }
}
#endif

}  // namespace alch
