// Galois automorphisms on CRT-basis elements (include/alchemy_hip.h, "Galois automorphisms"): the gather kernels behind
// alch_buf_automorph and alch_ct_automorph.  Included from alchemy_hip.hip after the element-wise helpers (Walk3, Pack, ALCH_WALK).
//
//   dst[e][limb][k] = src[e][limb][src_slot(k)],  src_slot(k) = slot(unit(k) * j mod m)      (automorph_host.hpp)
//
// One permutation for every limb and every element.  A lane owns VW consecutive destination words (16 bytes when n is a multiple of
// it, else one word: the split of k_scale), so stores are coalesced; the reads are the scattered side.
//   k_automorph_pow2   radix-16 engine (two-power m >= 32): the source slot is a closed form per lane (automorph::pow2_src: __brev, one
//                      multiply, a mask mod 2n); no table.  An aligned group of 2^t destination slots shares the low bits of brev(k),
//                      i.e. its units agree mod 2n / 2^t, and multiplication by j keeps that: the group reads ONE aligned group of
//                      2^t source slots, permuted inside.  So a lane also loads 16 bytes and picks its words from them.
//   k_automorph_tab    general engine: the phi(m)-entry table, device-resident.
#pragma once
#include "automorph_host.hpp"

namespace alch {

template <typename W, int VW>
__device__ __forceinline__ W automorph_pick(const Pack<W, VW>& x, u32 i) {
    W r = x.v[0];
#pragma unroll
    for (int t = 1; t < VW; ++t) r = i == (u32)t ? x.v[t] : r;
    return r;
}

template <typename W, int VW>
__global__ void k_automorph_pow2(DevRing<W> R, W* dst, const W* src, size_t words, u32 j, int logn) {
    typedef Pack<W, VW> P;
    const u32 nv = R.n / VW;
    ALCH_WALK_INIT(nv, R.L);
    ALCH_WALK(w, words / VW, wk) {
        const size_t base = (wk.outer * (size_t)R.L + wk.mid) * nv;        // first pack of this limb-polynomial
        const u32 k0 = wk.k * VW;
        u32 s[VW];
#pragma unroll
        for (int c = 0; c < VW; ++c) s[c] = automorph::pow2_src(k0 + c, j, logn);
        const P x = reinterpret_cast<const P*>(src)[base + s[0] / VW];
        P z;
#pragma unroll
        for (int c = 0; c < VW; ++c) z.v[c] = automorph_pick<W, VW>(x, s[c] % VW);
        reinterpret_cast<P*>(dst)[w] = z;
    }
}

template <typename W, int VW>
__global__ void k_automorph_tab(DevRing<W> R, W* dst, const W* src, size_t words, const u32* __restrict__ tab) {
    typedef Pack<W, VW> P;
    typedef Pack<u32, VW> T;
    const u32 nv = R.n / VW;
    ALCH_WALK_INIT(nv, R.L);
    ALCH_WALK(w, words / VW, wk) {
        const W* poly = src + (wk.outer * (size_t)R.L + wk.mid) * R.n;
        const T t = reinterpret_cast<const T*>(tab)[wk.k];
        P z;
#pragma unroll
        for (int c = 0; c < VW; ++c) z.v[c] = poly[t.v[c]];
        reinterpret_cast<P*>(dst)[w] = z;
    }
}

}  // namespace alch
