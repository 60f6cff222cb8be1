// k_tensor_intt_split: kernel A (c2 = a1 b1 s, crtInv, centred lift -> TrivGad digit) with the inverse transform run
// as TWO sequential half-size sub-transforms in 64 (+4) KiB of LDS, so that two independent 8-wave workgroups share
// a CU (k_tensor_intt holds the whole polynomial in LDS: one 16-wave workgroup per CU whose waves move through the
// load / transform / store phases in lock step).
//
// Gentleman-Sande order: the stages 14..1 of the n-point inverse act inside each half of the slots (sub-transform of
// size n/2 with the big ring's twiddles, prefix = 2 + half, no n^-1); stage 0 pairs coefficient k of the two
// halves.
//
// Three LDS trips per half for the 14 local stages (ALCH_TI_SPLIT_PASSES == 4, the product):
//   on load   a lane holds the products of four ADJACENT slots (one 16-byte piece of a1 and b1).  Local stages 13 and
//             12 pair slots at distance 1 and 2, inside the piece, so they run in registers before the piece is
//             written to LDS; their three twiddles (a pair and a single word, lane-contiguous in the table) are
//             fetched with the piece's operands.
//   LB = 2    stages [8, 12): groups {64 h + lo + 4 k}, per-lane twiddles (four lanes share a group index)
//   LB = 6    stages [4, 8):  wave-uniform twiddles.  ALCH_PLANT3_INV (!Q30): Plantard constants (R.twpi), the pass enters with the
//             12-instruction butterfly on the lazy [0,2q) values of the LB = 2 pass and goes on with the 8-instruction one on values
//             kept in [0, q] (modarith.hpp); so does the LB = 10 pass, and the closing stage takes keep[] and x[] as they are:
//             u + y <= 2q and u - y + q <= 2q are plain words for the Montgomery products that carry n^-1 s.
//   LB = 10   stages [0, 4):  wave-uniform twiddles, KEEP: nothing is written back.  A lane owns the coefficients
//             tid + 512 g + 1024 k of its half -- the same set for both halves -- so half 0's 32 values wait in
//             registers while half 1 is transformed, and stage 0, the n^-1 s scaling, the centred lift and the digit
//             stores are lane-local straight out of half 1's last pass.  For fixed (g, k) a wave stores 64
//             consecutive coefficients (256 contiguous bytes) with dword buffer stores.
// ALCH_TI_CLOSE_LDS = 1 writes the last pass back and reads both halves once more in the lane-contiguous layout for
// 16-byte digit stores (four trips); ALCH_TI_SPLIT_PASSES == 5 is the earlier sequence (4 + 4 + 4 + 2 stages in LDS
// and that closing trip: five), == 3 its radix-32 form.  DESIGN.md section 11 has the measurements.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include "ntt_engine.hpp"

#ifndef ALCH_TI_SPLIT_PASSES
#define ALCH_TI_SPLIT_PASSES 4
#endif
#ifndef ALCH_TI_CLOSE_LDS
#define ALCH_TI_CLOSE_LDS 0
#endif
// stages 13 and 12 in registers on load; the closing epilogue straight out of the last pass
#define ALCH_TI_ONLOAD (ALCH_TI_SPLIT_PASSES == 4)
#define ALCH_TI_EPI_REGS (ALCH_TI_ONLOAD && !ALCH_TI_CLOSE_LDS)

// experiment switch: cache policy of the operand loads (2 = non-temporal: read once by this kernel)
#ifndef ALCH_TI_NT_IN
#define ALCH_TI_NT_IN 0
#endif

// experiment (tools/build_variant.sh partials -DALCH_A_PARTIALS=1): this kernel also forms the key-switch
// kernel's starting values c0 = a0 b0 s + c2 h0_i, c1 = (a0 b1 + a1 b0) s + c2 h1_i for its limb (it holds a1, b1 and c2 anyway) and
// writes them to the result rows, so that the key-switch kernel reads two finished polynomials instead of four cold operands and
// two hint rows at the head of every item.  Measured, see DESIGN.md "dead ends"; off in the product.
#ifndef ALCH_A_PARTIALS
#define ALCH_A_PARTIALS 0
#endif

namespace alch {

// Q30: every modulus below 2^30 -- 8-instruction inverse butterflies (bfly_inv4); values stay in [0,2q) as otherwise
template <int LOGN, bool Q30 = false>
__global__ void __launch_bounds__(1 << (LOGN - 6), 4)
k_tensor_intt_split(DevRing<u32> R, const u32* __restrict__ a, const u32* __restrict__ b, int32_t* __restrict__ digits,
                    unsigned nitems, Scal<u32> spre
#if ALCH_A_PARTIALS
                    , const u32* __restrict__ hint, u32* __restrict__ out
#endif
                    ) {
    typedef u32 W;
    constexpr int LOGM = LOGN - 1, M = 1 << LOGM, LT = LOGN - 6, T = 1 << LT;
    typedef Geo<LOGM, LT> G;
    static_assert(G::E == 32 && (LOGM - 2) % 4 == 0, "32 coefficients per lane, stages 2 (on load) + 4 + 4 + 4");
    typedef u32 V __attribute__((ext_vector_type(4)));
#if !ALCH_TI_EPI_REGS
    typedef int32_t SV __attribute__((ext_vector_type(4)));
#endif
    constexpr int NV = G::E / 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    W* lds = reinterpret_cast<W*>(smem);
    const int L = R.L;
    const u32 nct = nitems / (unsigned)L;
    const auto ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<W*>(a), 0, (u32)((size_t)nct * 2 * L * (2 * M) * 4), 0x00020000);
    const auto rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<W*>(b), 0, (u32)((size_t)nct * 2 * L * (2 * M) * 4), 0x00020000);
    const auto rd = __builtin_amdgcn_make_buffer_rsrc(digits, 0, (u32)((size_t)nct * L * (2 * M) * 4), 0x00020000);
    const u32 lane16 = threadIdx.x * 16u;
#if ALCH_TI_EPI_REGS
    const u32 lane4 = threadIdx.x * 4u;
#endif
    constexpr u32 ROW = (u32)(2 * M) * 4u, SLICE = (u32)T * 16u, HALF = (u32)M * 4u;
#if ALCH_A_PARTIALS
    const auto rh = __builtin_amdgcn_make_buffer_rsrc(const_cast<W*>(hint), 0, (u32)((size_t)2 * L * L * (2 * M) * 4), 0x00020000);
    const auto ro = __builtin_amdgcn_make_buffer_rsrc(out, 0, (u32)((size_t)nct * 2 * L * (2 * M) * 4), 0x00020000);
#endif

    for (unsigned item = blockIdx.x; item < nitems; item += gridDim.x) {
        // the quotient comes out of the vector unit (the division runs on a float reciprocal): hand it back to scalar registers here,
        // or every offset derived from it may stay in vector registers (buffer offsets then cost a loop per access)
        const u32 ct = __builtin_amdgcn_readfirstlane(item / (unsigned)L), i = item - ct * (unsigned)L;
        const ModP<W> m = R.mod[i];
        const W q = m.q, qni = m.qni;
        const W ninv_s = mont_mul(R.ninv_m[i], spre.v[i], m), w1ninv_s = mont_mul(R.w1ninv_m[i], spre.v[i], m);
        const u32 row = ((2 * ct + 1) * (u32)L + i) * ROW;           // a1 / b1 of this ciphertext and limb
        const u32 drow = (ct * (u32)L + i) * ROW;
        const int rot = (int)((item ^ (item >> 3)) & (NV - 1));      // slice order rotated per item (HBM channels)
        const W* twi = R.twi[i];
        // the two wave-uniform passes: Plantard constants, values in [0, q] (the closing stage then skips its reductions)
        constexpr bool PINV = ALCH_PLANT3_INV && ALCH_TI_EPI_REGS && !Q30;
        const auto twu = pick_tw<PINV>(R.twpi[i], R.twi[i]);
        typedef typename std::remove_cv<typename std::remove_pointer<decltype(twu)>::type>::type TWU;
        W keep[G::E];
#pragma unroll 1
        for (int half = 0; half < 2; ++half) {
            int tid = threadIdx.x;
            asm volatile("" : "+v"(tid));
            const int prefix = 2 + half;
            // c2 = a1 b1 R^-1 (lazy) for this half of the slots -> LDS
#pragma unroll
            for (int r = 0; r < NV; ++r) {
                const u32 so = row + (u32)half * HALF + SLICE * (u32)((r + rot) & (NV - 1));
#if ALCH_TI_ONLOAD
                // the piece starts at slot b = 4 p: stage 13 groups b/2 and b/2 + 1, stage 12 group b/4
                const int p = tid + T * ((r + rot) & (NV - 1));
                typedef W W2 __attribute__((ext_vector_type(2)));
                const W2 w13 = *reinterpret_cast<const W2*>(twi + (prefix << (LOGM - 1)) + 2 * p);
                const W w12 = twi[(prefix << (LOGM - 2)) + p];
#endif
                const V va = __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(ra, lane16, so, ALCH_TI_NT_IN));
                const V vb = __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(rb, lane16, so, ALCH_TI_NT_IN));
#if ALCH_A_PARTIALS
                if (out) {   // the key-switch kernel's tensor part for this limb, with its very formulas (kernel_ks_half.hpp)
                    const u32 so0 = so - (u32)L * ROW;                                  // a0 / b0: the element in front of a1 / b1
                    const u32 piece = (u32)half * HALF + SLICE * (u32)((r + rot) & (NV - 1));
                    const u32 hrow = ((2 * i) * (u32)L + i) * ROW + piece;               // hint row (digit i, component 0, limb i)
                    const V a0v = __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(ra, lane16, so0, ALCH_TI_NT_IN));
                    const V b0v = __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(rb, lane16, so0, ALCH_TI_NT_IN));
                    const V h0v = __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(rh, lane16, hrow, 0));
                    const V h1v = __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(rh, lane16, hrow + (u32)L * ROW, 0));
                    const W sr2 = spre.v[i];
                    V o0v, o1v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const W x0 = csub(mont_mul_lazy(a0v[e], sr2, q, qni), q);
                        const W x1 = csub(mont_mul_lazy(va[e], sr2, q, qni), q);
                        const W c2 = csub(mont_mul_lazy(vb[e], x1, q, qni), q);
                        const u64 p0 = (u64)x0 * b0v[e] + (u64)c2 * h0v[e];
                        const u32 m0 = (u32)p0 * qni;
                        o0v[e] = csub((u32)((p0 + (u64)m0 * q) >> 32), q);
                        const u64 p1 = (u64)x0 * vb[e] + (u64)x1 * b0v[e] + (u64)c2 * h1v[e];
                        const u64 p1r = ((u64)csub((W)(p1 >> 32), q) << 32) | (u32)p1;
                        const u32 m1 = (u32)p1r * qni;
                        o1v[e] = csub((u32)((p1r + (u64)m1 * q) >> 32), q);
                    }
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(decltype(__builtin_amdgcn_raw_buffer_load_b128(ro, 0, 0, 0)), o0v), ro, lane16, so0, 0);
                    ALCH_STORE_GUARD(o0v);
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(decltype(__builtin_amdgcn_raw_buffer_load_b128(ro, 0, 0, 0)), o1v), ro, lane16, so, 0);
                    ALCH_STORE_GUARD(o1v);
                }
#endif
                W c[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) c[e] = mont_mul_lazy(va[e], vb[e], q, qni);
#if ALCH_TI_ONLOAD
                if constexpr (Q30) {
                    bfly_inv4(c[0], c[1], w13[0], q, qni); bfly_inv4(c[2], c[3], w13[1], q, qni);
                    bfly_inv4(c[0], c[2], w12, q, qni);    bfly_inv4(c[1], c[3], w12, q, qni);
                } else {
                    bfly_inv(c[0], c[1], (W)w13[0], q, qni);  bfly_inv(c[2], c[3], (W)w13[1], q, qni);
                    bfly_inv(c[0], c[2], w12, q, qni);        bfly_inv(c[1], c[3], w12, q, qni);
                }
#endif
                const V v = {c[0], c[1], c[2], c[3]};
                *reinterpret_cast<V*>(&lds[swz<LOGM>((tid + T * ((r + rot) & (NV - 1))) * 4)]) = v;
            }
            lds_barrier();
            NoEpilogue none;
            const W hq = (q - 1) >> 1;
#if ALCH_TI_ONLOAD
            ntt_pass<LOGM, LT, W, 8, 4, true, false, false, W, NoEpilogue&, false, Q30>(lds, twi, q, qni, (W)0, (W)0, tid, prefix, none);
            lds_barrier();
            ntt_pass<LOGM, LT, W, 4, 4, true, false, false, TWU, NoEpilogue&, false, Q30, PINV>(lds, twu, q, qni, (W)0, (W)0, tid, prefix, none);
            lds_barrier();
#if ALCH_TI_CLOSE_LDS
            ntt_pass<LOGM, LT, W, 0, 4, true, false, false, W, NoEpilogue&, false, Q30>(lds, twi, q, qni, (W)0, (W)0, tid, prefix, none);
            lds_barrier();
#else
            // x[k] = coefficient tid + T g + 1024 k of this half; half 0 waits in `keep`, half 1 closes: stage 0 with n^-1 s
            // folded in, centred lift, digit stores (for fixed g, k a wave writes 256 contiguous bytes)
            auto close = [&](int g, int, W* x) {
                if (half == 0) {
#pragma unroll
                    for (int k = 0; k < 16; ++k) keep[16 * g + k] = x[k];
                } else {
#pragma unroll
                    for (int k = 0; k < 16; ++k) {
                        // PINV: both in [0, q] already; the sums below stay words (<= 2q) and the products take any word
                        const W u = PINV ? keep[16 * g + k] : csub(keep[16 * g + k], q), y = PINV ? x[k] : csub(x[k], q);
                        const W c0 = csub(mont_mul_lazy((W)(u + y), ninv_s, q, qni), q);
                        const W c1 = csub(mont_mul_lazy((W)(u - y + q), w1ninv_s, q, qni), q);
                        const int32_t z0 = c0 > hq ? (int32_t)c0 - (int32_t)q : (int32_t)c0;
                        const int32_t z1 = c1 > hq ? (int32_t)c1 - (int32_t)q : (int32_t)c1;
                        const u32 so = drow + 4u * (u32)(T * g + (k << (LOGM - 4)));
                        __builtin_amdgcn_raw_buffer_store_b32(z0, rd, lane4, so, 0);
                        __builtin_amdgcn_raw_buffer_store_b32(z1, rd, lane4, so + HALF, 0);
                    }
                }
            };
            ntt_pass<LOGM, LT, W, 0, 4, true, true, false, TWU, decltype(close)&, false, Q30>(lds, twu, q, qni, (W)0, (W)0, tid, prefix, close);
#endif
#elif ALCH_TI_SPLIT_PASSES == 3
            // 14 stages as 5 + 5 + 4: three LDS round trips per half instead of four (radix-32 groups: 32 coefficients and
            // up to 31 per-lane twiddles in registers -- affordable here, there are no accumulators to keep)
            ntt_pass<LOGM, LT, W, 9, 5, true, false, false, W, NoEpilogue&, false, Q30>(lds, twi, q, qni, (W)0, (W)0, tid, prefix, none);
            lds_barrier();
            ntt_pass<LOGM, LT, W, 4, 5, true, false, false, W, NoEpilogue&, false, Q30>(lds, twi, q, qni, (W)0, (W)0, tid, prefix, none);
            lds_barrier();
            ntt_pass<LOGM, LT, W, 0, 4, true, false, false, W, NoEpilogue&, false, Q30>(lds, twi, q, qni, (W)0, (W)0, tid, prefix, none);
            lds_barrier();
#else
            ntt_pass<LOGM, LT, W, 10, 4, true, false, false, W, NoEpilogue&, false, Q30>(lds, twi, q, qni, (W)0, (W)0, tid, prefix, none);
            pair_sync<LOGM>();
            ntt_pass<LOGM, LT, W, 6, 4, true, false, false, W, NoEpilogue&, false, Q30>(lds, twi, q, qni, (W)0, (W)0, tid, prefix, none);
            lds_barrier();
            ntt_pass<LOGM, LT, W, 2, 4, true, false, false, W, NoEpilogue&, false, Q30>(lds, twi, q, qni, (W)0, (W)0, tid, prefix, none);
            lds_barrier();
            ntt_pass<LOGM, LT, W, 0, 2, true, false, false, W, NoEpilogue&, false, Q30>(lds, twi, q, qni, (W)0, (W)0, tid, prefix, none);
            lds_barrier();
#endif
#if !ALCH_TI_EPI_REGS
            if (half == 0) {
#pragma unroll
                for (int r = 0; r < NV; ++r) {
                    const V lo = *reinterpret_cast<const V*>(&lds[swz<LOGM>((tid + T * r) * 4)]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) keep[4 * r + e] = lo[e];
                }
            } else {
                // stage 0 with n^-1 s folded in, centred lift, digit stores (lane-contiguous, 16 bytes per lane)
#pragma unroll
                for (int r = 0; r < NV; ++r) {
                    const V hi = *reinterpret_cast<const V*>(&lds[swz<LOGM>((tid + T * r) * 4)]);
                    SV z0, z1;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const W x = csub(keep[4 * r + e], q), y = csub(hi[e], q);
                        const W c0 = csub(mont_mul_lazy((W)(x + y), ninv_s, q, qni), q);
                        const W c1 = csub(mont_mul_lazy((W)(x - y + q), w1ninv_s, q, qni), q);
                        z0[e] = c0 > hq ? (int32_t)c0 - (int32_t)q : (int32_t)c0;
                        z1[e] = c1 > hq ? (int32_t)c1 - (int32_t)q : (int32_t)c1;
                    }
                    const u32 so = drow + SLICE * (u32)r;
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(decltype(__builtin_amdgcn_raw_buffer_load_b128(rd, 0, 0, 0)), z0), rd, lane16, so, 0);
                    ALCH_STORE_GUARD(z0);
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(decltype(__builtin_amdgcn_raw_buffer_load_b128(rd, 0, 0, 0)), z1), rd, lane16, so + HALF, 0);
                    ALCH_STORE_GUARD(z1);
                }
            }
#endif
            lds_barrier();                      // LDS is refilled next
        }
    }
}

}  // namespace alch
