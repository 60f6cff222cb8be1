// decrypt / errorRate_ on resident ciphertext batches (include/alchemy_hip.h, "since 1.8"): the two kernels behind
// alch_ct_error_term, alch_buf_lift and alch_ct_decrypt_lift.  Included from alchemy_hip.hip after the element-wise helpers
// (Walk3, Pack, ALCH_WALK) it uses.
//
//   k_ct_eval_sk   c(s) on the CRT basis: Horner in the secret key, one pass over the ciphertext components
//   k_lift         centred lift mod Q = prod q_j of Pow / Dec coefficients with word arithmetic only: Garner digits, sign from a
//                  digit-vector comparison, residue mod p, lexicographic maximum of |x| per element
#pragma once

namespace alch {

// ---- c(s) -----------------------------------------------------------------------------------------------------------------
// out[b] = s_pre (c_0 + s (c_1 + s c_2)) per limb: ciphertext b = elements (DEG + 1) b .. of `in`, all on the CRT basis.
//   s1[j] = s_pre R, s2[j] = s_pre R^2 (mod q_j), so  t = mont(s, s2) = s s_pre R  and
//   DEG 1: out = mont(c0, s1) + mont(c1, t)                          3 products per word
//   DEG 2: out = mont(c0, s1) + mont(c1 + mont(c2, mont(s, R^2)), t)  5 products per word
// VW words per access (16 bytes when n is a multiple of it, else 1: the split of k_pointwise / k_pointwise_scalar).  The key element
// is read again by every ciphertext: it is one element and stays in L2.
template <typename W, int VW, int DEG>
__global__ void k_ct_eval_sk(DevRing<W> R, W* out, const W* in, const W* sk, size_t words, Scal<W> s1, Scal<W> s2) {
    typedef Pack<W, VW> P;
    const u32 nv = R.n / VW;
    const size_t ev = (size_t)R.L * nv;                      // packs per ring element
    ALCH_WALK_INIT(nv, R.L);
    ALCH_WALK(w, words / VW, wk) {
        const ModP<W> m = R.mod[wk.mid];
        const size_t src = w + wk.outer * (size_t)DEG * ev;  // component 0 of ciphertext wk.outer, same limb and position
        const P s = reinterpret_cast<const P*>(sk)[(size_t)wk.mid * nv + wk.k];
        const P c0 = reinterpret_cast<const P*>(in)[src];
        const P c1 = reinterpret_cast<const P*>(in)[src + ev];
        P c2 = c1, z;
        if (DEG == 2) c2 = reinterpret_cast<const P*>(in)[src + 2 * ev];
#pragma unroll
        for (int c = 0; c < VW; ++c) {
            const W t = mont_mul(s.v[c], s2.v[wk.mid], m);
            W u = c1.v[c];
            if (DEG == 2) u = add_mod(u, mont_mul(c2.v[c], mont_mul(s.v[c], m.r2, m), m), m.q);
            z.v[c] = add_mod(mont_mul(c0.v[c], s1.v[wk.mid], m), mont_mul(u, t, m), m.q);
        }
        reinterpret_cast<P*>(out)[w] = z;
    }
}

// ---- centred lift -----------------------------------------------------------------------------------------------------------
template <typename W>
struct LiftPar {
    ModP<W> mod[MAXL];
    W inv_m[MAXL][MAXL];       // [j][i], i < j: q_i^-1 mod q_j in Montgomery form
    u32 qp[MAXL];              // q_j mod p
    u32 L, n;
    u32 bal;                   // every q_i < 2 q_j: a digit of limb i enters limb j with one conditional subtraction
    u32 p, Qp, lmul;           // destination modulus (p < 2^31, may be composite), Q mod p, l_scalar mod p
    u64 pinv;                  // floor((2^64 - 1) / p)
    u32 epw;                   // elements per workgroup: 1 = the workgroup strides one element, 4 = one wave per element
};

// v mod p for p < 2^31 and any 64-bit v: Barrett quotient from pinv (short by at most 2), then the few subtractions left.
__device__ __forceinline__ u32 lift_mod_p(u64 v, u32 p, u64 pinv) {
    u64 r = v - mul_hi64(v, pinv) * (u64)p;
    while (r >= p) r -= p;
    return (u32)r;
}

__device__ __forceinline__ u32 lift_shfl(u32 v, int off) { return (u32)__shfl_down((int)v, off, 64); }
__device__ __forceinline__ u64 lift_shfl(u64 v, int off) {
    const u32 lo = (u32)__shfl_down((int)(u32)v, off, 64), hi = (u32)__shfl_down((int)(u32)(v >> 32), off, 64);
    return ((u64)hi << 32) | lo;
}

// a > b as mixed-radix digit vectors (limb 0 least significant): decided at the highest limb where they differ.
// `a = b if greater` on all MAXL words; words at and above L are zero on both sides.
template <typename W>
__device__ __forceinline__ void lift_take_max(W (&best)[MAXL], const W (&a)[MAXL]) {
    bool gt = false, open = true;
#pragma unroll
    for (int j = MAXL - 1; j >= 0; --j) {
        const bool ne = a[j] != best[j];
        gt = (open && ne) ? a[j] > best[j] : gt;
        open = open && !ne;
    }
#pragma unroll
    for (int j = 0; j < MAXL; ++j) best[j] = gt ? a[j] : best[j];
}

// src: count elements [L][n] (Pow or Dec basis, residues in [0, q_j)).  dst (nullable): count elements [n] of 32-bit words,
// l (x mod p) mod p.  maxd (nullable): count * L words, digits of max_k |x|.
// Mapping: P.epw == 1 -- one workgroup per element, lanes stride k, so every limb row is read coalesced; the maximum goes
// lane-local -> cross-lane -> LDS across the four waves.  P.epw == 4 (small n) -- one wave per element, four elements per
// workgroup, no workgroup barrier; the last workgroup may be ragged.
template <typename W>
__global__ void __launch_bounds__(256) k_lift(LiftPar<W> P, const W* src, u32* dst, u64* maxd, size_t count) {
    const u32 L = P.L, n = P.n;
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const bool per_wave = P.epw != 1;
    const size_t e = per_wave ? (size_t)blockIdx.x * P.epw + wave : (size_t)blockIdx.x;
    const bool live = e < count;                               // false only for the spare waves of a ragged last workgroup
    const u32 k0 = per_wave ? lane : threadIdx.x, kstep = per_wave ? 64u : 256u;
    W best[MAXL];
#pragma unroll
    for (int j = 0; j < MAXL; ++j) best[j] = 0;
    if (live) {
        const W* x = src + e * (size_t)L * n;
        for (u32 k = k0; k < n; k += kstep) {
            // Garner: d_j = (x_j - (d_0 + q_0 (d_1 + ...))) / (q_0 .. q_{j-1})  mod q_j, one limb of the running value at a time
            W d[MAXL];
#pragma unroll
            for (int j = 0; j < MAXL; ++j) {
                d[j] = 0;
                if ((u32)j < L) {
                    const ModP<W> m = P.mod[j];
                    W t = x[(size_t)j * n + k];
#pragma unroll
                    for (int i = 0; i < j; ++i) {
                        if (P.bal) t = mont_mul(sub_mod(t, csub(d[i], m.q), m.q), P.inv_m[j][i], m);
                        else t = sub_mod(mont_mul(t, P.inv_m[j][i], m), mont_mul(d[i], P.inv_m[j][i], m), m.q);   // d_i is any word
                    }
                    d[j] = t;
                }
            }
            // x > (Q - 1) / 2 ?  (Q - 1) / 2 has the digits (q_j - 1) / 2: all moduli are odd, so there is no tie
            bool neg = false, open = true;
#pragma unroll
            for (int j = MAXL - 1; j >= 0; --j) {
                if ((u32)j < L) {
                    const W h = (P.mod[j].q - 1) >> 1;
                    const bool ne = d[j] != h;
                    neg = (open && ne) ? d[j] > h : neg;
                    open = open && !ne;
                }
            }
            if (dst) {
                // x mod p by Horner from the top digit; a negative lift is x - Q
                u64 acc = 0;
#pragma unroll
                for (int j = MAXL - 1; j >= 0; --j)
                    if ((u32)j < L) acc = lift_mod_p(acc * P.qp[j] + (u64)d[j], P.p, P.pinv);      // < 2^31 2^31 + 2^62
                u32 r = (u32)acc;
                if (neg) { r += P.p - P.Qp; r -= r >= P.p ? P.p : 0u; }
                dst[e * (size_t)n + k] = lift_mod_p((u64)r * P.lmul, P.p, P.pinv);
            }
            if (maxd) {
                // |x|: for a negative lift the digits of Q - x = (Q - 1 - x) + 1, i.e. the complement q_j - 1 - d_j plus one with carry
                W a[MAXL];
                u32 carry = neg ? 1u : 0u;
#pragma unroll
                for (int j = 0; j < MAXL; ++j) {
                    a[j] = 0;
                    if ((u32)j < L) {
                        const W q = P.mod[j].q;
                        W v = neg ? (W)(q - 1 - d[j]) : d[j];
                        v += carry;
                        carry = (neg && v == q) ? 1u : 0u;
                        a[j] = carry ? (W)0 : v;
                    }
                }
                lift_take_max(best, a);
            }
        }
    }
    if (!maxd) return;
    // cross-lane: every wave reduces its 64 lanes (spare waves carry zeros)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        W o[MAXL];
#pragma unroll
        for (int j = 0; j < MAXL; ++j) o[j] = ((u32)j < L) ? lift_shfl(best[j], off) : (W)0;
        lift_take_max(best, o);
    }
    if (per_wave) {
        if (live && lane == 0)
#pragma unroll
            for (int j = 0; j < MAXL; ++j)
                if ((u32)j < L) maxd[e * L + j] = (u64)best[j];
        return;
    }
    __shared__ W part[4][MAXL];
    if (lane == 0)
#pragma unroll
        for (int j = 0; j < MAXL; ++j) part[wave][j] = best[j];
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            W o[MAXL];
#pragma unroll
            for (int j = 0; j < MAXL; ++j) o[j] = part[w][j];
            lift_take_max(best, o);
        }
#pragma unroll
        for (int j = 0; j < MAXL; ++j)
            if ((u32)j < L) maxd[e * L + j] = (u64)best[j];
    }
}

}  // namespace alch
