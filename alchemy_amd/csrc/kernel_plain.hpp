// Plaintext-side mul_, div2_ and linearCyc_ on resident batches (include/alchemy_hip.h, "plaintext ring elements on resident
// batches"): the kernels behind alch_pt_mul, alch_pt_eval_lin, alch_pt_rescale and alch_buf_add_bcast.  Included from
// alchemy_hip.hip after the element-wise helpers (Walk3, Pack, ALCH_WALK, reduce_signed) it uses.
//
// A plaintext ring Z_p[zeta_m] (p = 2^e, or 7: no CRT basis) multiplies over a LIFTING ring, any CRT ring of the same index with
// modulus product Q: residues are lifted centred to the integers, reduced into every limb, the ring operation runs exactly mod Q
// with the existing transforms, and k_lift (kernel_lift.hpp) brings the centred result back mod p.
//
//   k_pt_lift_in      Z_p words -> centred lift -> residues in every limb of the lifting ring
//   k_pt_lift_gather  the same through a position table: embed(coeffs(x)_i) arrives in the lifting ring of index s in one pass
//   k_pt_mac          d_rel-term slot-wise inner product with the resident linear-function values (Montgomery form)
//   k_pt_rescale      coefficient-wise division by p / p' with a non-divisibility flag
//   k_pt_add_bcast    dst[e] = src[e] + one   (addLit_ on a batch)
#pragma once

namespace alch {

// Centred representative of v in [0, p), p < 2^31: in [-(p/2), (p-1)/2], so |z| <= p/2 (p/2 itself goes to -p/2 when p is even).
__device__ __forceinline__ int32_t pt_centre(u32 v, u32 p) { return v > ((p - 1) >> 1) ? (int32_t)v - (int32_t)p : (int32_t)v; }

// src: count elements [n] of 32-bit Z_p words.  dst: count elements [L][n] of the lifting ring R.  A thread owns VW consecutive
// coefficients: one 16-byte read (VW = 4), and per limb one (32-bit words) or two (64-bit words) 16-byte writes.
template <typename W, int VW>
__global__ void k_pt_lift_in(DevRing<W> R, W* dst, const u32* src, size_t count, u32 p) {
    typedef typename Signed<W>::type SW;
    const u32 nv = R.n / VW, L = (u32)R.L;
    ALCH_WALK_INIT(nv, 1);
    ALCH_WALK(w, count * (size_t)nv, wk) {
        const Pack<u32, VW> x = reinterpret_cast<const Pack<u32, VW>*>(src)[w];
        int32_t z[VW];
#pragma unroll
        for (int c = 0; c < VW; ++c) z[c] = pt_centre(x.v[c], p);
        Pack<W, VW>* o = reinterpret_cast<Pack<W, VW>*>(dst) + wk.outer * (size_t)L * nv + wk.k;
        for (u32 j = 0; j < L; ++j) {
            const W q = R.mod[j].q;
            Pack<W, VW> y;
#pragma unroll
            for (int c = 0; c < VW; ++c) y.v[c] = (W)reduce_signed<W>((SW)z[c], q);
            o[(size_t)j * nv] = y;
        }
    }
}

// The table form.  tab: [d_rel][n_s] source positions in the index-r element (n_r words), -1 = zero -- `coeffs` (R -> E, relative
// index i) followed by embedPow (E -> S).  dst: count * d_rel elements [L][n_s] of the lifting ring R (index s), row i of batch
// element b at element b * d_rel + i.  The table is read 16 bytes at a time, the Z_p words are gathered, the writes are 16 bytes.
template <typename W, int VW>
__global__ void k_pt_lift_gather(DevRing<W> R, W* dst, const u32* src, const int32_t* tab, size_t count, u32 d_rel, u32 n_r, u32 p) {
    typedef typename Signed<W>::type SW;
    const u32 nv = R.n / VW, L = (u32)R.L;
    ALCH_WALK_INIT(nv, d_rel);
    ALCH_WALK(w, count * (size_t)d_rel * nv, wk) {
        const Pack<int32_t, VW> t = reinterpret_cast<const Pack<int32_t, VW>*>(tab)[(size_t)wk.mid * nv + wk.k];
        const u32* x = src + wk.outer * (size_t)n_r;
        int32_t z[VW];
#pragma unroll
        for (int c = 0; c < VW; ++c) z[c] = t.v[c] < 0 ? 0 : pt_centre(x[(u32)t.v[c]], p);
        Pack<W, VW>* o = reinterpret_cast<Pack<W, VW>*>(dst) + (wk.outer * d_rel + wk.mid) * (size_t)L * nv + wk.k;
        for (u32 j = 0; j < L; ++j) {
            const W q = R.mod[j].q;
            Pack<W, VW> y;
#pragma unroll
            for (int c = 0; c < VW; ++c) y.v[c] = (W)reduce_signed<W>((SW)z[c], q);
            o[(size_t)j * nv] = y;
        }
    }
}

// out[b] = sum_i x[b * d_rel + i] * y[i] slot by slot (CRT basis): x, out plain residues in [0, q), y in Montgomery form.
// 32-bit words: groups of K products are summed in 64 bits and reduced once, by the rule of k_tunnel_mac_e -- with t the running
// sum in [0, 2q), acc = t (R mod q) + sum_K x y < q 2^32 as long as (K + 2) q < 2^32; moduli too close to 2^31 for a group of two
// (and 64-bit words) take one Montgomery product at a time.  Same residues either way.
template <typename W, int VW>
__global__ void k_pt_mac(DevRing<W> R, W* out, const W* x, const W* y, size_t count, u32 d_rel) {
    typedef Pack<W, VW> P;
    const u32 nv = R.n / VW, L = (u32)R.L;
    const size_t ev = (size_t)L * nv;                         // packs per ring element
    ALCH_WALK_INIT(nv, L);
    ALCH_WALK(w, count * ev, wk) {
        const ModP<W> m = R.mod[wk.mid];
        const size_t pos = (size_t)wk.mid * nv + wk.k;
        const P* xs = reinterpret_cast<const P*>(x) + wk.outer * (size_t)d_rel * ev + pos;
        const P* ys = reinterpret_cast<const P*>(y) + pos;
        P z;
        bool done = false;
        if constexpr (sizeof(W) == 4) {
            const u32 q = (u32)m.q, qni = (u32)m.qni, r1 = (u32)m.r1;
            const u32 K = lazy_group(q);
            if (K >= 2) {
                u64 acc[VW];
#pragma unroll
                for (int c = 0; c < VW; ++c) acc[c] = 0;
                auto redc = [&](u64 t) -> u32 { return mont_red_lazy(t, q, qni); };   // t < q 2^32 -> [0, 2q)
                for (u32 i0 = 0; i0 < d_rel; i0 += K) {
                    const u32 iend = i0 + K < d_rel ? i0 + K : d_rel;
                    for (u32 i = i0; i < iend; ++i) {
                        const P a = xs[(size_t)i * ev], b = ys[(size_t)i * ev];
#pragma unroll
                        for (int c = 0; c < VW; ++c) acc[c] += (u64)(u32)a.v[c] * (u32)b.v[c];
                    }
                    if (iend < d_rel) {
#pragma unroll
                        for (int c = 0; c < VW; ++c) acc[c] = (u64)redc(acc[c]) * r1;
                    }
                }
#pragma unroll
                for (int c = 0; c < VW; ++c) z.v[c] = (W)csub(redc(acc[c]), q);
                done = true;
            }
        }
        if (!done) {
#pragma unroll
            for (int c = 0; c < VW; ++c) z.v[c] = 0;
            for (u32 i = 0; i < d_rel; ++i) {
                const P a = xs[(size_t)i * ev], b = ys[(size_t)i * ev];
#pragma unroll
                for (int c = 0; c < VW; ++c) z.v[c] = add_mod(z.v[c], mont_mul(a.v[c], b.v[c], m), m.q);
            }
        }
        reinterpret_cast<P*>(out)[w] = z;
    }
}

// dst = floor(src / d) word by word (src over Z_p, dst over Z_{p/d}); *flag |= 1 when some word is not a multiple of d.  The flag
// is reduced over the wave (ballot), over the workgroup's four waves through LDS, and leaves with one atomic per workgroup.
template <int VW>
__global__ void __launch_bounds__(256) k_pt_rescale(u32* dst, const u32* src, size_t words, u32 d, int* flag) {
    typedef Pack<u32, VW> P;
    bool bad = false;
    for (size_t w = blockIdx.x * (size_t)blockDim.x + threadIdx.x; w < words / VW; w += (size_t)gridDim.x * blockDim.x) {
        P x = reinterpret_cast<const P*>(src)[w];
#pragma unroll
        for (int c = 0; c < VW; ++c) {
            const u32 t = x.v[c] / d;
            bad = bad || (x.v[c] - t * d) != 0u;
            x.v[c] = t;
        }
        reinterpret_cast<P*>(dst)[w] = x;
    }
    __shared__ int part[4];
    const bool wave_bad = __ballot(bad) != 0;
    if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = wave_bad ? 1 : 0;
    __syncthreads();
    if (threadIdx.x == 0 && (part[0] | part[1] | part[2] | part[3])) atomicOr(flag, 1);
}

// dst[e] = src[e] + one (limb by limb): `one` is a single ring element, re-read by every element of the batch (it stays in L2).
template <typename W, int VW>
__global__ void k_pt_add_bcast(DevRing<W> R, W* dst, const W* src, const W* one, size_t words) {
    typedef Pack<W, VW> P;
    const u32 nv = R.n / VW;
    ALCH_WALK_INIT(nv, R.L);
    ALCH_WALK(w, words / VW, wk) {
        P x = reinterpret_cast<const P*>(src)[w];
        const P o = reinterpret_cast<const P*>(one)[(size_t)wk.mid * nv + wk.k];
        const W q = R.mod[wk.mid].q;
#pragma unroll
        for (int c = 0; c < VW; ++c) x.v[c] = add_mod(x.v[c], o.v[c], q);
        reinterpret_cast<P*>(dst)[w] = x;
    }
}

}  // namespace alch
