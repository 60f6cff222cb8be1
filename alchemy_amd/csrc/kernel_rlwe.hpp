// encrypt on resident batches (include/alchemy_hip.h, "encrypt"): the kernels behind alch_buf_gauss_dec and alch_ct_encrypt.
// Included from alchemy_hip.hip after the element-wise helpers (Walk3, Pack, ALCH_WALK) it uses; the arithmetic of one coefficient
// is gauss_sampler.hpp's, shared with the host.
//
//   k_gauss_sample    one lane per coefficient: counter -> two splitmix64 words -> table search in LDS -> (double)f * scale.
//                     FUSED (two-power index: no odd axis): rounds and stores the residues of every limb at once, no scratch
//   k_gauss_axis<P>   the Cholesky factor of P I - J along one odd axis of the scratch: one lane per column, column in registers
//   k_gauss_round     scratch doubles -> (coset) rounding -> residues of every limb, limb-major
//   k_ct_encrypt      c1 = the uniform words of alch_buf_fill_uniform's odd elements, c0 = err - c1 s, one pass on the CRT basis
//   k_ct_ks_hint      the same pass per gadget entry with g_t v added: key-switch and tunnel hints (alch_ct_ks_hint)
//   k_*_keyed         the same three with their words from ChaCha20 keystreams (chacha_stream.hpp; a ring with alch_ring_set_rng_key):
//                     one lane per keystream block, which is four consecutive positions
#pragma once

#include "chacha_stream.hpp"
#include "gauss_sampler.hpp"
#include "hint_gadget.hpp"

namespace alch {

__device__ const u64 d_gauss_cdt[gauss::CDT_LEN] = {ALCH_GAUSS_CDT_VALUES};

struct GaussPar {
    u64 q[MAXL];               // destination moduli (0: the integers)
    u64 seed, ctr0;            // stream, counter of coefficient 0 of the launch's first element: (elem0 + e0) n mod 2^64
    double scale;
    u32 L, n, logn;            // logn: only read by the fused kernel (n a power of two)
    u32 p;                     // coset modulus, 0 = errorRounded
};

// The table, once per workgroup: 582 words, 4.7 KiB of LDS.
__device__ __forceinline__ void gauss_load_cdt(u64* T) {
    for (u32 i = threadIdx.x; i < gauss::CDT_LEN; i += blockDim.x) T[i] = d_gauss_cdt[i];
    __syncthreads();
}

// total = coefficients of the launch (elements * n).  FUSED: dst = limb-major words of the first element, coset (nullable) = the
// Z_p words of the first element; otherwise xs = scratch doubles, dst and coset unused.
template <typename W, bool FUSED>
__global__ void __launch_bounds__(256) k_gauss_sample(GaussPar G, double* xs, W* dst, const u32* coset, size_t total) {
    __shared__ u64 T[gauss::CDT_LEN];
    gauss_load_cdt(T);
    for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const double x = gauss::sample(G.seed, G.ctr0 + (u64)idx, G.scale, T);
        if (!FUSED) { xs[idx] = x; continue; }
        const int64_t z = gauss::round_coset(x, G.p, G.p ? coset[idx] : 0u);
        const size_t e = idx >> G.logn, i = idx & ((size_t)G.n - 1);
        W* o = dst + (e * G.L) * (size_t)G.n + i;
#pragma unroll
        for (int j = 0; j < MAXL; ++j)
            if ((u32)j < G.L) o[(size_t)j * G.n] = (W)gauss::reduce(z, G.q[j]);
    }
}

// Keyed form: the two words of coefficient c are the pair of position c of domain 1 (G.seed the nonce, G.ctr0 a plain integer, the
// launch's last position below 2^58).  A lane owns one absolute block, positions 4 blk .. 4 blk + 3, intersected with the launch's
// range [ctr0, ctr0 + total): ctr0 = elem0 n is 2 mod 4 for n = 2 mod 4 and odd elem0, so a launch may begin and end inside a block.
// blocks = number of blocks that meet the range.
template <typename W, bool FUSED>
__global__ void __launch_bounds__(256) k_gauss_sample_keyed(GaussPar G, chacha::Key K, double* xs, W* dst, const u32* coset, size_t total,
                                                            size_t blocks) {
    __shared__ u64 T[gauss::CDT_LEN];
    gauss_load_cdt(T);
    const u64 blk0 = G.ctr0 >> 2;
    for (size_t b = blockIdx.x * (size_t)blockDim.x + threadIdx.x; b < blocks; b += (size_t)gridDim.x * blockDim.x) {
        u64 u[8];
        chacha::block(K, chacha::block_counter(chacha::DOM_GAUSS, (blk0 + b) << 2), G.seed, u);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const u64 c = ((blk0 + b) << 2) + (u64)s;
            if (c < G.ctr0 || c - G.ctr0 >= (u64)total) continue;
            const size_t idx = (size_t)(c - G.ctr0);
            const double x = gauss::rn_mul((double)gauss::deviate(u[2 * s], u[2 * s + 1], T), G.scale);
            if (!FUSED) { xs[idx] = x; continue; }
            const int64_t z = gauss::round_coset(x, G.p, G.p ? coset[idx] : 0u);
            const size_t e = idx >> G.logn, i = idx & ((size_t)G.n - 1);
            W* o = dst + (e * G.L) * (size_t)G.n + i;
#pragma unroll
            for (int j = 0; j < MAXL; ++j)
                if ((u32)j < G.L) o[(size_t)j * G.n] = (W)gauss::reduce(z, G.q[j]);
        }
    }
}

struct GaussChol { double l[(gauss::MAX_ODD_PRIME - 1) * (gauss::MAX_ODD_PRIME - 1)]; };   // row-major (P-1) x (P-1), by value

// xs: `elems` elements of n doubles.  Axis of prime P: entries base + i mp stride, i < P - 1; one lane per column (j0 = 0 entry),
// cols = elems * n / (P - 1) < 2^31.  s = 0.0; s = s + Lc[i][k] * col[k], k ascending, every operation rounded on its own.
template <int P>
__global__ void __launch_bounds__(256) k_gauss_axis(GaussChol C, double* xs, u32 n, u32 mp, u32 stride, u32 cols) {
    constexpr int H = P - 1;
    const u32 per = n / H;                                     // columns per element
    for (u32 c = blockIdx.x * blockDim.x + threadIdx.x; c < cols; c += gridDim.x * blockDim.x) {
        const u32 e = c / per, r = c - e * per;
        const u32 lo = r % stride, t = r / stride, j1 = t % mp, hi = t / mp;
        double* x = xs + (size_t)e * n + (size_t)hi * H * mp * stride + (size_t)j1 * stride + lo;
        const size_t step = (size_t)mp * stride;
        double col[H], out[H];
#pragma unroll
        for (int i = 0; i < H; ++i) col[i] = x[i * step];
#pragma unroll
        for (int i = 0; i < H; ++i) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k <= i; ++k) s = gauss::rn_add(s, gauss::rn_mul(C.l[i * H + k], col[k]));
            out[i] = s;
        }
#pragma unroll
        for (int i = 0; i < H; ++i) x[i * step] = out[i];
    }
}

// xs: total = elems * n doubles (< 2^31).  dst: limb-major words of the first element, coset (nullable) as in k_gauss_sample.
template <typename W>
__global__ void __launch_bounds__(256) k_gauss_round(GaussPar G, const double* xs, W* dst, const u32* coset, u32 total) {
    for (u32 idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int64_t z = gauss::round_coset(xs[idx], G.p, G.p ? coset[idx] : 0u);
        const u32 e = idx / G.n, i = idx - e * G.n;
        W* o = dst + ((size_t)e * G.L) * G.n + i;
#pragma unroll
        for (int j = 0; j < MAXL; ++j)
            if ((u32)j < G.L) o[(size_t)j * G.n] = (W)gauss::reduce(z, G.q[j]);
    }
}

// ---- SymmSHE encrypt, ring arithmetic ---------------------------------------------------------------------------------------
// out[2b] = err[b] - c1 s, out[2b+1] = c1, c1 word (b, j, k) = splitmix64(seed + ((2 (ct0 + b) + 1) L + j) n + k) mod q_j: with
// ct0 = 0 the words alch_buf_fill_uniform(out, seed) leaves in the odd elements.  words = batch * L * n.  VW words per access as in
// k_ct_eval_sk.  The key element goes to Montgomery form on the way in (one product), read again by every ciphertext from L2.
template <typename W, int VW>
__global__ void k_ct_encrypt(DevRing<W> R, W* out, const W* err, const W* sk, size_t words, u64 seed, u64 ct0) {
    typedef Pack<W, VW> P;
    const u32 nv = R.n / VW;
    const size_t ev = (size_t)R.L * nv;                      // packs per ring element
    ALCH_WALK_INIT(nv, R.L);
    ALCH_WALK(w, words / VW, wk) {
        const ModP<W> m = R.mod[wk.mid];
        const P s = reinterpret_cast<const P*>(sk)[(size_t)wk.mid * nv + wk.k];
        const P e = reinterpret_cast<const P*>(err)[w];
        const u64 pos = ((2 * (ct0 + (u64)wk.outer) + 1) * (u64)R.L + wk.mid) * (u64)R.n + (u64)wk.k * VW;
        P c0, c1;
#pragma unroll
        for (int c = 0; c < VW; ++c) {
            const W u = (W)(splitmix64(seed + pos + (u64)c) % (u64)m.q);
            c1.v[c] = u;
            c0.v[c] = sub_mod(e.v[c], mont_mul(u, mont_mul(s.v[c], m.r2, m), m), m.q);
        }
        const size_t o = w + wk.outer * ev;                  // component 0 of ciphertext wk.outer, same limb and position
        reinterpret_cast<P*>(out)[o] = c0;
        reinterpret_cast<P*>(out)[o + ev] = c1;
    }
}

// PW uniform words of domain `dom` from position pos on, reduced into m.  PW = 4: pos is a multiple of 4 (n % 4 = 0), the four words
// are one block.  PW = 1: a block per word.
template <typename W, int PW>
__device__ __forceinline__ void keyed_uniform(const chacha::Key& K, u64 nonce, unsigned dom, u64 pos, const ModP<W>& m, W* out) {
    const chacha::Mod<W> cm = {m.q, m.qni, m.r1, m.r2};
    if constexpr (PW == 4) {
        u64 u[8];
        chacha::block(K, chacha::block_counter(dom, pos), nonce, u);
#pragma unroll
        for (int c = 0; c < 4; ++c) out[c] = chacha::reduce128(u[2 * c], u[2 * c + 1], cm);
    } else {
        u64 A, B;
        chacha::pair(K, nonce, dom, pos, A, B);
        out[0] = chacha::reduce128(A, B, cm);
    }
}

// Keyed form of k_ct_encrypt: c1 word (b, j, k) = (B 2^64 + A) mod q_j of position pos (the same rule, a plain integer below 2^58) of
// domain 2, nonce `seed`.  PW words per lane: 4 (n % 4 = 0: one block, 16 or 32 bytes per access) or 1.
template <typename W, int PW>
__global__ void k_ct_encrypt_keyed(DevRing<W> R, chacha::Key K, W* out, const W* err, const W* sk, size_t words, u64 seed, u64 ct0) {
    typedef Pack<W, PW> P;
    const u32 nv = R.n / PW;
    const size_t ev = (size_t)R.L * nv;                      // packs per ring element
    ALCH_WALK_INIT(nv, R.L);
    ALCH_WALK(w, words / PW, wk) {
        const ModP<W> m = R.mod[wk.mid];
        const P s = reinterpret_cast<const P*>(sk)[(size_t)wk.mid * nv + wk.k];
        const P e = reinterpret_cast<const P*>(err)[w];
        const u64 pos = ((2 * (ct0 + (u64)wk.outer) + 1) * (u64)R.L + wk.mid) * (u64)R.n + (u64)wk.k * PW;
        P c0, c1;
        keyed_uniform<W, PW>(K, seed, chacha::DOM_ENCRYPT, pos, m, c1.v);
#pragma unroll
        for (int c = 0; c < PW; ++c) c0.v[c] = sub_mod(e.v[c], mont_mul(c1.v[c], mont_mul(s.v[c], m.r2, m), m), m.q);
        const size_t o = w + wk.outer * ev;                  // component 0 of ciphertext wk.outer, same limb and position
        reinterpret_cast<P*>(out)[o] = c0;
        reinterpret_cast<P*>(out)[o + ev] = c1;
    }
}

// ---- key-switch and tunnel hints (ksHint, KeysHints.hs:101-129), ring arithmetic ---------------------------------------------
// For value i and gadget entry t < D, e = i D + t: out[2e + 1] = a, uniform words by k_ct_encrypt's rule; out[2e] = g_t v[i] + err[e] - a s.
// g_t is 2^(w d(t)) on limb i(t) and 0 elsewhere (hint_gadget.hpp; w = 1 for BaseBGad 2, d = 0 for TrivGad), so v is read on one limb of every entry only.  One launch serves the
// entries [e0, e0 + count): out, err and the counter ct0 are those of entry e0, v is value 0.  Walked as [i][t L + j][k] from the
// position of entry e0: t and j come from one 32-bit division, i never needs a 64-bit one.  words = count L n.
template <typename W, int VW>
__global__ void k_ct_ks_hint(DevRing<W> R, hintgad::Layout G, W* out, const W* v, const W* err, const W* sk, size_t words, u64 e0,
                             u64 seed, u64 ct0) {
    typedef Pack<W, VW> P;
    const u32 nv = R.n / VW, L = (u32)R.L;
    const size_t ev = (size_t)L * nv;                        // packs per ring element
    Walk3 wk(blockIdx.x * (size_t)blockDim.x + threadIdx.x + (size_t)e0 * ev, (size_t)gridDim.x * blockDim.x, nv, G.D * L);
    ALCH_WALK(w, words / VW, wk) {
        const u32 t = wk.mid / L, j = wk.mid - t * L;
        const ModP<W> m = R.mod[j];
        const u64 e = (u64)wk.outer * G.D + t - e0;          // entry of this launch
        const P s = reinterpret_cast<const P*>(sk)[(size_t)j * nv + wk.k];
        P h0 = reinterpret_cast<const P*>(err)[w], h1;
        u32 gl, gd;
        hintgad::entry(G, t, gl, gd);
        if (gl == j) {
            const W g = mont_mul((W)((W)1 << (gd * G.w)), m.r2, m);  // 2^(w d) < q_j, to Montgomery form
            const P x = reinterpret_cast<const P*>(v)[(wk.outer * L + j) * nv + wk.k];
#pragma unroll
            for (int c = 0; c < VW; ++c) h0.v[c] = add_mod(h0.v[c], mont_mul(x.v[c], g, m), m.q);
        }
        const u64 pos = hintgad::odd_word_pos(ct0 + e, L, j, R.n, wk.k * VW);
#pragma unroll
        for (int c = 0; c < VW; ++c) {
            const W u = (W)(splitmix64(seed + pos + (u64)c) % (u64)m.q);
            h1.v[c] = u;
            h0.v[c] = sub_mod(h0.v[c], mont_mul(u, mont_mul(s.v[c], m.r2, m), m), m.q);
        }
        const size_t o = w + (size_t)e * ev;                 // component 0 of pair e, same limb and position
        reinterpret_cast<P*>(out)[o] = h0;
        reinterpret_cast<P*>(out)[o + ev] = h1;
    }
}

// Keyed form of k_ct_ks_hint: the a words from domain 3, nonce `seed`, by k_ct_encrypt_keyed's rule with the entry for the ciphertext.
template <typename W, int PW>
__global__ void k_ct_ks_hint_keyed(DevRing<W> R, chacha::Key K, hintgad::Layout G, W* out, const W* v, const W* err, const W* sk,
                                   size_t words, u64 e0, u64 seed, u64 ct0) {
    typedef Pack<W, PW> P;
    const u32 nv = R.n / PW, L = (u32)R.L;
    const size_t ev = (size_t)L * nv;                        // packs per ring element
    Walk3 wk(blockIdx.x * (size_t)blockDim.x + threadIdx.x + (size_t)e0 * ev, (size_t)gridDim.x * blockDim.x, nv, G.D * L);
    ALCH_WALK(w, words / PW, wk) {
        const u32 t = wk.mid / L, j = wk.mid - t * L;
        const ModP<W> m = R.mod[j];
        const u64 e = (u64)wk.outer * G.D + t - e0;          // entry of this launch
        const P s = reinterpret_cast<const P*>(sk)[(size_t)j * nv + wk.k];
        P h0 = reinterpret_cast<const P*>(err)[w], h1;
        u32 gl, gd;
        hintgad::entry(G, t, gl, gd);
        if (gl == j) {
            const W g = mont_mul((W)((W)1 << (gd * G.w)), m.r2, m);  // 2^(w d) < q_j, to Montgomery form
            const P x = reinterpret_cast<const P*>(v)[(wk.outer * L + j) * nv + wk.k];
#pragma unroll
            for (int c = 0; c < PW; ++c) h0.v[c] = add_mod(h0.v[c], mont_mul(x.v[c], g, m), m.q);
        }
        keyed_uniform<W, PW>(K, seed, chacha::DOM_HINT, hintgad::odd_word_pos(ct0 + e, L, j, R.n, wk.k * PW), m, h1.v);
#pragma unroll
        for (int c = 0; c < PW; ++c) h0.v[c] = sub_mod(h0.v[c], mont_mul(h1.v[c], mont_mul(s.v[c], m.r2, m), m), m.q);
        const size_t o = w + (size_t)e * ev;                 // component 0 of pair e, same limb and position
        reinterpret_cast<P*>(out)[o] = h0;
        reinterpret_cast<P*>(out)[o + ev] = h1;
    }
}

}  // namespace alch
