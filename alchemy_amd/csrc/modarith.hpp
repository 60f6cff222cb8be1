// Word-size modular arithmetic for gfx950 (and the host-side table builder).
//
// Montgomery multiplication with R = 2^32 (32-bit residues, q < 2^31) or R = 2^64 (q < 2^62).
// Measured on MI355X (tools/ubench): v_mul_lo/v_mul_hi/v_mad_u64_u32 all issue at ~4.5 cycles per
// wave64, v_add/v_sub at ~2.6, v_min_u32 at ~4.1.  The 32-bit Montgomery product below compiles to
// exactly three multiplier instructions (v_mad_u64_u32, v_mul_lo_u32, v_mad_u64_u32) with no
// separate add, one fewer instruction than Shoup's and with one-word twiddles.  A product by a table constant in
// Plantard's form (plant_mul3 below) is three multiplier instructions as well and comes out in [0, q] with no
// conditional subtraction: the butterflies whose twiddle is shared by a whole wave use it (two-word twiddles).
//
// Ranges.  mont_mul_lazy(a, b): a any word, b < q  ->  a*b*R^-1 mod q in [0, 2q).
// Ring data are kept "lazy" in [0, 2q) between butterfly stages (2q < 2^32 / 2^63); csub() brings
// a [0,2q) value to [0,q).  4q does not fit a 32-bit word for ALCHEMY's 31-bit moduli
// (examples/HomomRLWR.hs:37-43), so Harvey's [0,4q) butterflies are not used; nor does 3q, so the SUM of a
// lazy and a reduced value needs a conditional subtraction first.  The DIFFERENCE of two lazy values does fit:
// sub_lazy(a, u, 2q): a, u in [0,2q)  ->  a - u mod q in [0,2q)  (a - u lies in (-2q, 2q); 2q is added back on a
// borrow, so nothing wraps and neither operand is reduced first).  A lazy accumulator therefore takes a
// product as  acc = sub_lazy(acc, mont_mul_lazy(-x, h))  in 6 instructions, against 8 for the sum of reduced values.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ALCH_HD __host__ __device__ __forceinline__
#else
#define ALCH_HD inline
#endif

namespace alch {

typedef uint32_t u32;
typedef uint64_t u64;

template <typename W>
struct ModP {
    W q;     // modulus
    W qni;   // -q^-1 mod R
    W r1;    // R mod q          (Montgomery form of 1)
    W r2;    // R^2 mod q        (to_mont multiplier)
};

ALCH_HD u32 mont_mul_lazy(u32 a, u32 b, u32 q, u32 qni) {
    u64 p = (u64)a * b;
    u32 m = (u32)p * qni;
    return (u32)((p + (u64)m * q) >> 32);
}

ALCH_HD u64 mul_hi64(u64 a, u64 b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (u64)(((unsigned __int128)a * b) >> 64);
#endif
}

ALCH_HD u64 mont_mul_lazy(u64 a, u64 b, u64 q, u64 qni) {
    // One 128-bit accumulation (p + m q < 2 q 2^64 < 2^127): on gfx950 this form compiles to 18 % fewer VALU
    // instructions than hi(a b) + hi(m q) + carry (28 against 34 per product, mostly register-pair moves).
    const unsigned __int128 p = (unsigned __int128)a * b;
    const u64 m = (u64)p * qni;
    return (u64)((p + (unsigned __int128)m * q) >> 64);
}

// [0,2q) -> [0,q).  x - q wraps to a huge value when x < q, so the unsigned min picks x.
ALCH_HD u32 csub(u32 x, u32 q) { u32 y = x - q; return y < x ? y : x; }
ALCH_HD u64 csub(u64 x, u64 q) { u64 y = x - q; return y < x ? y : x; }
// a, u in [0,q2), q2 = 2q  ->  a - u (mod q) in [0,q2).  gfx950: v_sub_co_u32, v_cndmask_b32, v_add_u32.
ALCH_HD u32 sub_lazy(u32 a, u32 u, u32 q2) { u32 d = a - u; return a < u ? d + q2 : d; }

template <typename W>
ALCH_HD W mont_mul(W a, W b, const ModP<W>& m) { return csub(mont_mul_lazy(a, b, m.q, m.qni), m.q); }
template <typename W>
ALCH_HD W add_mod(W a, W b, W q) { return csub((W)(a + b), q); }            // a,b in [0,q)
template <typename W>
ALCH_HD W sub_mod(W a, W b, W q) { W d = a - b; W e = d + q; return e < d ? e : d; }   // a,b in [0,q)

// The difference leg of a forward butterfly, xx + (c - t) with t <= c (c = q after a csub, c = 2q for Harvey's form where t < 2q):
// c - t = |c - t|, so the leg is an absolute difference plus xx -- the same word, not merely a congruent one -- and gfx950 has that
// as ONE instruction, v_sad_u32 D = |A - B| + C (A = c stays in its scalar register), where the plain form compiles to a subtract
// and an add.  hipcc forms it from the expression below; the host compiles the same line.
// ALCH_BFLY_SAD = 0: the subtract-and-add form (A/B builds, tools/build_variant.sh).
#ifndef ALCH_BFLY_SAD
#define ALCH_BFLY_SAD 1
#endif
ALCH_HD u32 diff_leg(u32 xx, u32 c, u32 t) {
#if ALCH_BFLY_SAD
    return (c > t ? c - t : t - c) + xx;
#else
    return xx + (c - t);
#endif
}

// Forward (Cooley-Tukey) butterfly on lazy values: x,y in [0,2q), w = twiddle in Montgomery form.
//   x' = x + w*y, y' = x - w*y   (mod q), outputs in [0,2q).  W = u32: 9 VALU instructions (three multiplier instructions, two
// conditional subtractions of two each, one add, one v_sad_u32); W = u64 keeps the subtract-and-add leg.
template <typename W>
ALCH_HD void bfly_fwd(W& x, W& y, W w, W q, W qni) {
    W xx = csub(x, q);
    W t = csub(mont_mul_lazy(y, w, q, qni), q);
    x = xx + t;
    y = xx + (q - t);
}
ALCH_HD void bfly_fwd(u32& x, u32& y, u32 w, u32 q, u32 qni) {
    const u32 xx = csub(x, q);
    const u32 t = csub(mont_mul_lazy(y, w, q, qni), q);
    x = xx + t;
    y = diff_leg(xx, q, t);
}

// q < 2^30 (4q fits a word): Harvey's lazy butterflies.  Forward: x, y in [0,4q) -> [0,4q); the product takes ANY word, so y is
// never reduced.  7 VALU instructions instead of 9 (the difference leg is |2q - t| + xx, t < 2q).  Inverse: x, y in [0,2q) -> [0,2q);
// 8 instead of 10.
ALCH_HD void bfly_fwd4(u32& x, u32& y, u32 w, u32 q, u32 qni) {
    const u32 q2 = 2u * q;
    const u32 xx = csub(x, q2);
    const u32 t = mont_mul_lazy(y, w, q, qni);
    x = xx + t;
    y = diff_leg(xx, q2, t);
}
ALCH_HD void bfly_inv4(u32& x, u32& y, u32 w, u32 q, u32 qni) {
    const u32 q2 = 2u * q;
    const u32 s = x + y, d = x + (q2 - y);
    x = csub(s, q2);
    y = mont_mul_lazy(d, w, q, qni);
}

// Montgomery reduction of a 64-bit value: p < q 2^32  ->  p R^-1 mod q in [0, 2q)   (then p + m q < 2^64).
ALCH_HD u32 mont_red_lazy(u64 p, u32 q, u32 qni) {
    u32 m = (u32)p * qni;
    return (u32)((p + (u64)m * q) >> 32);
}

// Lazy inner products on 32-bit words: how many products x y (x, y < q) one 64-bit accumulator takes between two Montgomery
// reductions.  With t in [0, 2q) the running sum carried as t (R mod q) < 2 q^2, a group of K products keeps
//   acc = t (R mod q) + sum_K x y < (K + 2) q^2 < q 2^32   as long as   (K + 2) q < 2^32,
// the bound of mont_red_lazy.  K = floor((2^32 - 1) / q) - 2, at most 8; 0 (one Montgomery product at a time) where a group of
// two does not fit.
ALCH_HD u32 lazy_group(u32 q) {
    const u32 kmax = 0xFFFFFFFFu / q;                       // (K + 2) q < 2^32
    return kmax >= 4 ? (kmax - 2 > 8 ? 8u : kmax - 2) : 0u;
}

// Weighted sums of reduced values (kernel_lincomb.hpp): acc += y w for y < q and a CANONICAL weight w < q, neither in Montgomery form,
// in groups of K = lazy_group(q) products under the bound above.  `carry` opens the next group: the running sum T comes back as
// t = T R^-1 in [0, 2q) and is carried as t (R mod q) = T (mod q), below 2 q^2.  lincomb_close returns T mod q in [0, q): the last
// reduction leaves T R^-1, and the product with R^2 mod q takes the factor out again (mont_mul_lazy takes any word on its left).
ALCH_HD u64 lincomb_step(u64 acc, bool carry, u32 y, u32 w, u32 q, u32 qni, u32 r1) {
    if (carry) acc = (u64)mont_red_lazy(acc, q, qni) * r1;
    return acc + (u64)y * w;
}
ALCH_HD u32 lincomb_close(u64 acc, u32 q, u32 qni, u32 r2) { return csub(mont_mul_lazy(mont_red_lazy(acc, q, qni), r2, q, qni), q); }

// The variant of dense_row a modulus allows: 2 below 2^32 / 6 (6 q < 2^32), 1 below 2^32 / sqrt(6) (6 q^2 < 2^64), else 0.
ALCH_HD int dense_level(u64 q) { return q < 715827882ull ? 2 : q < 1753413056ull ? 1 : 0; }

// c in [0,q) -> its centred representative in [-(q-1)/2, (q-1)/2]; negate: that of -c.
ALCH_HD int32_t centre_const(u32 c, u32 q, bool negate) {
    const int32_t s = c > ((q - 1) >> 1) ? (int32_t)c - (int32_t)q : (int32_t)c;
    return negate ? -s : s;
}

// Two Cooley-Tukey stages on SIGNED inputs as one multiply-add chain with a single reduction per output:
//   y0 = (x0 c0 + x2 c2 + x1 c1 + x3 c3) R^-1,   y2 = (x0 c0 + x2 c2 - x1 c1 - x3 c3) R^-1   (mod q), both in [0, 2q).
// With c0 = R, c2 = s w1 R, c1 = w2 R, c3 = s w1 w2 R (mod q, centred) these are stages 0 and 1 of the half s = +-1 of a forward
// transform:  u = x0 + s w1 x2, v = x1 + s w1 x3, y0 = u + w2 v, y2 = u - w2 v; with every constant negated, those of the negated input.
// Preconditions: q < 2^31, |x_k| < 2^30, |c_k| <= (q - 1) / 2.  Then each of x0 c0 + x2 c2 and x1 c1 + x3 c3 is below 2^30 (q - 1) in
// magnitude, so with C = q 2^31 (a multiple of q: the residues are exact) C + S +- T lies in (2^31, q 2^32 - 2^31): positive, below
// the reduction's bound, no 64-bit overflow.  gfx950: 4 v_mad_i64_i32, an add and a subtract of 64-bit pairs and two reductions
// (v_mul_lo_u32, v_mad_u64_u32) per pair of outputs -- 5.5 instructions per output, against 13 for a lazy stage 0 plus a butterfly.
ALCH_HD void stage01_signed(int32_t x0, int32_t x1, int32_t x2, int32_t x3, int32_t c0, int32_t c1, int32_t c2, int32_t c3,
                            u32 q, u32 qni, u32& y0, u32& y2) {
    const int64_t S = (int64_t)((u64)q << 31) + (int64_t)x0 * c0 + (int64_t)x2 * c2;
    const int64_t T = (int64_t)x1 * c1 + (int64_t)x3 * c3;
    y0 = mont_red_lazy((u64)(S + T), q, qni);
    y2 = mont_red_lazy((u64)(S - T), q, qni);
}

// Plantard multiplication by a precomputed constant (Plantard, "Efficient word size modular arithmetic",
// 2021).  For a constant c the table holds  br = (-c * 2^64 mod q) * q^-1 mod 2^64.  With T = a*br mod 2^64 and t1 = T >> 32,
//   result = floor((t1 + 1) * q / 2^32)  ==  a*c mod q   for ANY 32-bit a
// provided q < 2^31 (then a * (-c 2^64 mod q) < 2^63 and q 2^32 + that product < 2^64, which is the
// condition for the rounded quotient to be exact).  The price is a two-word constant.
// plant_mul3: the closing step as hi32(t1 q + q), ONE v_mad_u64_u32 -- three multiplier instructions in all (v_mul_hi_u32 and two
// v_mad_u64_u32), as many as a lazy Montgomery product, and the result needs no correction: it lies in [0, q].  The upper end is
// reached only at t1 = 2^32 - 1 (a c = 0 mod q), where (t1 + 1) q / 2^32 is q itself; every consumer of these butterflies takes q
// for 0 (the next butterfly, csub, a Montgomery product).
// plant_mul: the same with t1 + 1 formed in 32 bits first (four instructions; at t1 = 2^32 - 1 it wraps to 0 where plant_mul3 gives
// q, otherwise the same word).  Kept for A/B builds (ALCH_USE_PLANTARD, kernels_ntt.hpp).
ALCH_HD u32 plant_close(u32 t1, u32 q) { return (u32)(((u64)t1 * q + q) >> 32); }     // (2^32 - 1) q + q = q 2^32: no overflow
ALCH_HD u32 plant_t1(u32 a, u64 br) {
    const u64 lo = (u64)a * (u32)br;
    return (u32)((u64)a * (u32)(br >> 32) + (lo >> 32));
}
ALCH_HD u32 plant_mul3(u32 a, u64 br, u32 q) { return plant_close(plant_t1(a, br), q); }
ALCH_HD u32 plant_mul(u32 a, u64 br, u32 q) {
    const u32 t1 = plant_t1(a, br);
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(t1 + 1u, q);
#else
    return (u32)(((u64)(u32)(t1 + 1u) * q) >> 32);
#endif
}
// the product the Plantard butterflies use: plant_mul3 unless an A/B build asks for the four-instruction form
#ifndef ALCH_USE_PLANTARD
#define ALCH_USE_PLANTARD 0
#endif
ALCH_HD u32 plant_tw(u32 a, u64 br, u32 q) {
#if ALCH_USE_PLANTARD
    return plant_mul(a, br, q);
#else
    return plant_mul3(a, br, q);
#endif
}

// Forward butterfly with a Plantard twiddle: 7 VALU instructions (csub 2, product 3, add, v_sad_u32).  x in [0,2q), y ANY word
// -> xx < q, t <= q:  x' = xx + t <= 2q - 1,  y' = |q - t| + xx <= 2q - 1: both below 2q, what a Montgomery pass, another
// Plantard butterfly or the hint product takes.
// (its two legs from the twiddle product t in [0, q], apart so that the host test can put t = q through them)
ALCH_HD void bfly_fwd_from_t(u32& x, u32& y, u32 t, u32 q) {
    const u32 xx = csub(x, q);
    x = xx + t;
    y = diff_leg(xx, q, t);
}
ALCH_HD void bfly_fwd(u32& x, u32& y, u64 br, u32 q, u32 /*qni*/) { bfly_fwd_from_t(x, y, plant_tw(y, br, q), q); }

// Inverse (Gentleman-Sande) butterfly with a Plantard twiddle on values kept in [0, q] (q itself stands for 0): 8 VALU instructions.
//   d = x + (q - y) in [0, 2q] (any word suits the product),  x' = csub(x + y, q) in [0, q]  (x + y <= 2q),  y' = d w in [0, q].
ALCH_HD void bfly_inv(u32& x, u32& y, u64 br, u32 q, u32 /*qni*/) {
    const u32 s = x + y, d = x + (q - y);
    x = csub(s, q);
    y = plant_tw(d, br, q);
}
// its entry form: x, y lazy in [0,2q) are reduced first (12 instructions); outputs in [0, q] as above.
ALCH_HD void bfly_inv_entry(u32& x, u32& y, u64 br, u32 q, u32 qni) {
    x = csub(x, q);
    y = csub(y, q);
    bfly_inv(x, y, br, q, qni);
}

// Inverse (Gentleman-Sande) butterfly: x' = x + y, y' = (x - y) * w.  in/out in [0,2q).
template <typename W>
ALCH_HD void bfly_inv(W& x, W& y, W w, W q, W qni) {
    W a = csub(x, q), b = csub(y, q);
    x = a + b;
    y = mont_mul_lazy((W)(a - b + q), w, q, qni);
}

// ---- 64-bit rings: Shoup twiddles ----------------------------------------------------------------------
// A 64-bit Montgomery product is 11 multiplier instructions and, with the register-pair moves hipcc needs for the
// zero-extended addends, 27 VALU instructions.  A product by a CONSTANT w (a twiddle) with the precomputed quotient
// w' = floor(w 2^64 / q) (Shoup / Harvey, "Faster arithmetic for number-theoretic transforms", 2014):
//     Q = hi64(a w'),   r = a w - Q q  (mod 2^64)   in [0, 2q)   for ANY 64-bit a
// needs the high half of one product and the low halves of two: 17 VALU instructions (the subtraction rides on the
// multiply-add chain as + Q (2^64 - q)).  4q < 2^64 for every supported modulus (q < 2^62), so the forward butterflies
// are Harvey's: values in [0,4q) inside a register-resident pass, one conditional subtraction per butterfly, and
// [0,2q) again at the pass boundary (what every loader and epilogue of the engine expects).  w is a plain residue
// (ring data are never in Montgomery form), two words per twiddle.
struct alignas(16) Sh64 { u64 w, wp; };

ALCH_HD u64 shoup_mul_lazy(u64 a, Sh64 t, u64 q) {
    const u32 a0 = (u32)a, a1 = (u32)(a >> 32), p0 = (u32)t.wp, p1 = (u32)(t.wp >> 32);
#if defined(__HIP_DEVICE_COMPILE__)
    const u64 m1 = (u64)a1 * p0 + __umulhi(a0, p0);
#else
    const u64 m1 = (u64)a1 * p0 + (((u64)a0 * p0) >> 32);
#endif
    const u64 m2 = (u64)a0 * p1 + (u32)m1;
    const u64 Q = (u64)a1 * p1 + ((m1 >> 32) + (m2 >> 32));     // hi64(a w'), exact
    return a * t.w + Q * ((u64)0 - q);
}

// Forward butterfly of stage r of a register-resident pass (FIRST: inputs in [0,2q), else [0,4q); LAST: outputs
// reduced to [0,2q), else left in [0,4q)).
// (first / last are compile-time constants after the stage loops are unrolled)
ALCH_HD void bfly_fwd_st(u64& x, u64& y, Sh64 w, u64 q, u64 /*qni*/, bool FIRST, bool LAST) {
    const u64 q2 = 2 * q;
    const u64 xx = FIRST ? x : csub(x, q2);
    const u64 t = shoup_mul_lazy(y, w, q);
    x = xx + t;
    y = xx + (q2 - t);
    if (LAST) { x = csub(x, q2); y = csub(y, q2); }
}
// Inverse (Gentleman-Sande) butterfly, [0,2q) in and out: one conditional subtraction.
ALCH_HD void bfly_inv(u64& x, u64& y, Sh64 w, u64 q, u64 /*qni*/) {
    const u64 q2 = 2 * q;
    const u64 s = x + y, d = x + (q2 - y);
    x = csub(s, q2);
    y = shoup_mul_lazy(d, w, q);
}
// every other twiddle type: the stage position does not matter
template <typename W, typename TW>
ALCH_HD void bfly_fwd_st(W& x, W& y, TW w, W q, W qni, bool, bool) { bfly_fwd(x, y, w, q, qni); }

// sum_t x[t] * M[t] (Montgomery: M holds M R) for canonical x, M < q < 2^31.
// 32-bit words: four products are summed in 64 bits before one reduction -- 4 q^2 < 2^64, the sum's high word is < 2q, one
// conditional subtraction brings the sum below q 2^32, then a single Montgomery reduction: 10 instructions per four terms
// instead of 20.  64-bit words: one product at a time.
// LVL 1 (every modulus of the ring below 2^32 / sqrt(6) = 1 753 413 056: all of the reference's): up to SIX products are summed
// before one reduction -- 6 q^2 < 2^64, the sum's high word is < 2.2 q and takes two conditional subtractions (2q, q).  One
// Montgomery reduction per row of a CRT_13 / DFT_13 half-matrix instead of two: 14 instructions per row instead of 21.
// LVL 2 (every modulus below 2^32 / 6 = 715 827 882: all of examples/Tunnel.hs's): six q^2 stay below q 2^32, the sum's high word is
// already below q -- no conditional subtraction in front of the reduction (10 instructions per six-term row instead of 14).  Any level:
// a chunk of one or two products needs none either (2 q^2 < q 2^32 for every q < 2^31).
template <int R, int LVL = 0, typename MP>
ALCH_HD u32 dense_row(const u32* x, MP M, u32 q, u32 qni) {
    constexpr int CH = LVL ? 6 : 4;
    u32 acc = 0;
#pragma unroll
    for (int t0 = 0; t0 < R; t0 += CH) {
        const int terms = (R - t0 < CH) ? R - t0 : CH;
        u64 p = (u64)x[t0] * M[t0];
#pragma unroll
        for (int t = t0 + 1; t < t0 + CH && t < R; ++t) p += (u64)x[t] * M[t];
        u32 hi = (u32)(p >> 32);
        if (LVL == 1 && terms > 4) hi = csub(hi, 2u * q);                       // more than four terms: high word < 2.2 q
        if (terms > 2 && LVL != 2) hi = csub(hi, q);                             // high word < 2q -> < q
        const u64 pr = ((u64)hi << 32) | (u32)p;
        const u32 m = (u32)pr * qni;
        const u32 v = csub((u32)((pr + (u64)m * q) >> 32), q);
        acc = t0 ? csub(acc + v, q) : v;
    }
    return acc;
}
template <int R, int LVL = 0, typename MP>
ALCH_HD u64 dense_row(const u64* x, MP M, u64 q, u64 qni) {
    u64 acc = csub(mont_mul_lazy(x[0], M[0], q, qni), q);
#pragma unroll
    for (int t = 1; t < R; ++t) acc = csub(acc + csub(mont_mul_lazy(x[t], M[t], q, qni), q), q);
    return acc;
}

// ---- host-side helpers (table building) ------------------------------------------------------
inline u64 h_mulmod(u64 a, u64 b, u64 q) { return (u64)(((unsigned __int128)a * b) % q); }
inline u64 h_powmod(u64 b, u64 e, u64 q) {
    u64 r = 1 % q;
    b %= q;
    while (e) {
        if (e & 1) r = h_mulmod(r, b, q);
        b = h_mulmod(b, b, q);
        e >>= 1;
    }
    return r;
}

inline Sh64 h_shoup_const(u64 c, u64 q) {
    Sh64 t;
    t.w = c;
    t.wp = (u64)((((unsigned __int128)c) << 64) / q);
    return t;
}

// Plantard constant of c (< q) for modulus q < 2^31.
inline u64 h_plant_const(u64 c, u64 q) {
    u64 inv = 1;                                 // q^-1 mod 2^64
    for (int i = 0; i < 7; ++i) inv *= 2 - q * inv;
    const u64 r64 = h_powmod(2, 64, q);
    const u64 b = h_mulmod((q - c % q) % q, r64, q);      // -c * 2^64 mod q
    return b * inv;
}

template <typename W>
inline ModP<W> make_modp(u64 q) {
    ModP<W> m;
    m.q = (W)q;
    W inv = 1;                                  // Newton: inv = q^-1 mod 2^bits
    for (int i = 0; i < 7; ++i) inv *= (W)2 - (W)q * inv;
    m.qni = (W)0 - inv;
    const int bits = 8 * (int)sizeof(W);
    u64 r1 = h_powmod(2, (u64)bits, q);
    m.r1 = (W)r1;
    m.r2 = (W)h_mulmod(r1, r1, q);
    return m;
}

}  // namespace alch
