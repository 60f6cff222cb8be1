/*
 * alchemy_hip.h -- C ABI of the MI355X (gfx950) ciphertext-arithmetic backend for ALCHEMY's evaluator.
 *
 * This is the boundary a new Lol `Tensor` instance binds to.  The reference
 * never names a backend: every ALCHEMY signature is polymorphic in the tensor type `t`
 * (Crypto/Alchemy/Language/SHE.hs:21-45, Crypto/Alchemy/Interpreter/PT2CT.hs:78-96) and the backend is
 * chosen only by the tensor type in an example's `PT` alias (examples/Arithmetic.hs:19,23).  The
 * entry points below are what `instance Tensor GT` would `foreign import ccall`; each cites the
 * reference call site (or the Lol Tensor method behind it) that it serves.  INTEGRATION.md shows
 * the Haskell-side stub.
 *
 * Conventions
 *   - plain C: no C++ types, no exceptions across the ABI (every entry point catches: std::bad_alloc -> ALCH_E_NOMEM,
 *     anything else -> ALCH_E_INTERNAL).  Every function returns an int status
 *     (ALCH_OK == 0, negative == error); alch_last_error() gives a thread-local message.
 *   - ring R'_q = Z_q[zeta_m], ANY cyclotomic index m whose odd prime factors are <= 13 (the reference's
 *     ciphertext indices are H0' = F11648 .. H5' = F20475 = 2^a 3^b 5^c 7 13, examples/Common.hs:38-54) with
 *     n = phi(m) <= 40960; for m = 2n a power of two that is Z_q[X]/(X^n+1).  RNS limbs q_0..q_{L-1}, limb 0 =
 *     outermost component of Lol's nested pair (Crypto/Alchemy/Interpreter/PT2CT/Noise.hs:82-89,130).
 *   - HOST buffers use Lol's layout: int64_t, tuple-interleaved ("AoS"): coefficient k of limb j of
 *     one ring element at data[k*L + j], residues in [0, q_j)   (ZqBasic q Int64, examples/Common.hs:35).
 *     Host buffers are caller-owned, modified in place, never retained.
 *   - DEVICE buffers (alch_buf) are library-owned handles holding ring elements limb-major in HBM:
 *     element e, limb j, coefficient k at word (e*L + j)*n + k; 32-bit words when every q_j < 2^31
 *     (all of ALCHEMY's moduli, PT2CT.hs:137-139,283-285), 64-bit words otherwise (q < 2^62).
 *   - bases (toolkit / Lol definitions; m = prod_l p_l^e_l, primes ascending, m_l = p_l^e_l, m'_l = m_l/p_l):
 *       Pow  p_j = prod_l zeta_{m_l}^{j_l}, j_l in [phi(m_l)], zeta_{m_l} = zeta_m^(m/m_l); linear index mixed radix,
 *            first factor outermost (for a two-power index: the coefficient vector)
 *       Dec  d^T = p^T L, L = kron_l (L_{p_l} (x) I_{m'_l}), L_p = lower-triangular all-ones; == Pow for a two-power index
 *       CRT  slot (s_1..s_k) holds sigma_u(x), sigma_u: zeta_m -> omega_m^u, omega_m = gen^((q-1)/m), gen = smallest
 *            generator of Z_q^*, u = i0 + p i1 (mod m_l) where s_l = (i0 - 1) m'_l + digitrev_p(i1);
 *            for a two-power index: slot k holds a(psi^(2*brev(k)+1)), psi = omega_m.
 *       g    = prod_{odd p | m} (1 - zeta_p)   (1 for a two-power index)
 *   - all work is queued on the ring's HIP stream; alch_sync() waits for it.  Entry points are thread-safe: a call that
 *     touches a ring holds the lock of that ring's DEVICE until it returns (calls on one GPU are serialised -- they only queue
 *     work --, calls on different GPUs run side by side), so a host may force tensors from any number of threads (a -threaded
 *     Haskell RTS).  The *_free functions do not take it (finalizer threads): free a handle only when no call is using it.
 *     A ring is bound to the HIP device that was current when it was created; every entry point makes that device current for
 *     the calling thread first, so rings may be used from any OS thread (Haskell `safe` calls).
 *   - there is NO CPU fallback: without a gfx950 device every compute entry point fails with
 *     ALCH_E_NO_DEVICE.
 */
#ifndef ALCHEMY_HIP_H
#define ALCHEMY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ALCH_OK 0
#define ALCH_E_INVALID (-1)        /* bad argument (null, size, basis) */
#define ALCH_E_NOT_PRIME (-2)      /* alch_host_root only: q is not an odd prime */
#define ALCH_E_NO_CRT (-3)         /* no CRT basis over Z_q: q composite, q = 2, or q != 1 mod m -- Lol's crtFuncs returns Nothing */
#define ALCH_E_UNSUPPORTED (-4)    /* a CRT basis exists but this backend does not serve the ring: index with a prime factor > 13,
                                      limb-polynomial larger than the LDS, q >= 2^62 */
#define ALCH_E_NO_DEVICE (-5)      /* no gfx950 device / HIP runtime error at init */
#define ALCH_E_HIP (-6)            /* HIP runtime error (message in alch_last_error) */
#define ALCH_E_NOMEM (-7)          /* device or host allocation failed */
#define ALCH_E_INTERNAL (-8)       /* a C++ exception was caught at the ABI (never crosses it); message in alch_last_error */
#define ALCH_NOT_DIVISIBLE 1       /* divG family: Lol's Nothing */

/* bases of alch_buf_mulg / alch_buf_divg */
#define ALCH_BASIS_POW 0
#define ALCH_BASIS_DEC 1
#define ALCH_BASIS_CRT 2

typedef struct alch_ring alch_ring;
typedef struct alch_buf alch_buf;
typedef struct alch_hint alch_hint;
typedef struct alch_tunnel alch_tunnel;

/* flags of alch_ct_mul_relin */
#define ALCH_POW_IN 1u             /* inputs are in the Pow basis (crt applied first)          */
#define ALCH_POW_OUT 2u            /* outputs wanted in the Pow basis (crtInv applied last)     */
#define ALCH_AUTO_SUM 4u           /* alch_ct_automorph_hoisted: one output batch, the sum over the set's rotations */

/* gadgets (Crypto/Alchemy/Interpreter/PT2CT.hs:139-140) */
#define ALCH_GAD_TRIV 0            /* TrivGad: one digit per limb, centred lift                 */
#define ALCH_GAD_BASE2 1           /* BaseBGad 2: sum_i ceil(log2 q_i) digits; unfused device path */
/* BaseBGad 2^w, 1 <= w <= 16 (added within 1.8): limb i has k_i = ceil(ceil(log2 q_i) / w) digits, the smallest k with 2^(w k) >= q_i;
 * limb 0's digits first, least significant first; non-top digits in [-2^(w-1), 2^(w-1)), the top digit absorbs the rest (Lol's
 * divModCent); gadget entry t of limb i is 2^(w t) on limb i and 0 elsewhere.  About 1/w of BaseBGad 2's digit transforms for w - 1
 * more bits of hint noise.  Accepted wherever a gadget code is taken (alch_hint_load, alch_hint_from_buf, alch_tunnel_create,
 * alch_ct_ks_hint, alch_ct_ks_hint_part, alch_select_limbs, alch_gadget_digits, alch_decompose_baseb); such a hint or tunnel runs the
 * composed (unfused) device path of BaseBGad 2.  ALCH_GAD_BASEPOW2(1) means exactly ALCH_GAD_BASE2: same digit count, same words.
 * w = 0, w > 16 and every other code: ALCH_E_INVALID.  The cap at 16 is a decision, not a limit of the arithmetic: above it a digit
 * is within 2^15 of TrivGad's on a 31-bit limb. */
#define ALCH_GAD_BASEPOW2(w) (0x100 | (w))

const char *alch_last_error(void);
/* Library/ABI version: (major<<16)|minor; the minor number goes up with every added capability (1.7: tunnels between two-power rings; 1.8: decrypt / error rates on resident batches).).
 * The step entry points of mul_ (alch_ct_mul, alch_ct_key_switch_quad, alch_ct_mod_switch_deg) were added WITHIN 1.8 -- the number did
 * not move; a host that wants them probes for the symbols (dlsym / ctypes hasattr).  So were the plaintext-side entry points
 * (alch_pt_mul, alch_pt_linear_create / _free, alch_pt_eval_lin, alch_pt_rescale, alch_buf_add_bcast, alch_pt_bound) and
 * alch_ct_add. */
uint32_t alch_version(void);

/* ---- ring context ------------------------------------------------------------------------------
 * Replaces the per-call twiddle/modulus arguments lol-cpp receives from Haskell; built once per
 * (index, modulus-list) type, i.e. once per `Cyc t m' zq` instance (PT2CT.hs:251-254).
 * m = cyclotomic index (2n).  Builds device-resident twiddle tables with the root rule above.
 * STATUS ORDER (part of the ABI; haskell/.../GT.hs `ringFor` dispatches on it, tests/test_host_logic.py and
 * tests/test_gpu_example_rings.py pin it):
 *   ALCH_E_INVALID      malformed arguments (null, L out of 1..8, a modulus < 2, repeated moduli)
 *   ALCH_E_NO_CRT       some modulus is composite, 2, or a prime that is not 1 mod m -- exactly the cases in which Lol's
 *                       `crtFuncs` is Nothing for ZqBasic (CRTrans Maybe needs a prime q with m | q - 1; a pair needs both
 *                       components).  Decided BEFORE the index is looked at: it is a property of (m, q), not of this backend.
 *                       The plaintext rings of the reference land here (Z_{2^e}, examples/Common.hs:32; Zq 7 over F4,
 *                       examples/Arithmetic.hs:23); the caller then creates the ring with alch_ring_create_nocrt.
 *   ALCH_E_UNSUPPORTED  a CRT basis exists but the backend does not serve (m, q): a Lol host keeps that (index, element type)
 *                       on lol-cpp as a whole (every basis-order-dependent method).
 *   ALCH_E_NO_DEVICE / ALCH_E_HIP / ALCH_E_NOMEM   run-time failures, checked last.
 * Two-power m: 32 <= m <= 2^17 (n <= 2^16) when every q < 2^31, m <= 2^16 (n <= 2^15) otherwise.  The largest size
 * of each word runs its transforms as two LDS-resident halves and the key switch unfused; the fused
 * kernels of alch_ct_mul_relin / alch_ct_mul_full cover n <= 2^15 (32-bit) / 2^14 (64-bit); at the largest size both
 * entry points run the same operations composed from element-wise kernels and batched transforms.
 * Any other m (composite, or two-power below 32): the pass engine of kernel_gen.hpp -- every transform LDS-resident
 * (phi(m) * word <= 160 KiB), the key switch composed from the element-wise tensor product (with mulG), batched
 * crtInv, digit transforms with decompose + reduce in their loader, and the hint inner product. */
int alch_ring_create(uint32_t m, int L, const uint64_t *q, alch_ring **out);
/* A ring WITHOUT CRT basis: Lol's Tensor over a modulus whose crtFuncs is Nothing -- a plaintext ring Z_p (any
 * 2 <= q < 2^31, e.g. the Z_{2^e} of examples/Common.hs:32) or, with q = 0, the integers (Tensor t m Int64: what
 * Lol lifts to in decrypt, PT2CT.hs:91-99).  Serves the Pow / Dec operations: l, lInv, mulG, divG (Pow, Dec), add,
 * sub, upload / download; everything that needs the CRT basis returns ALCH_E_NO_CRT. */
int alch_ring_create_nocrt(uint32_t m, int L, const uint64_t *q, alch_ring **out);
int alch_ring_destroy(alch_ring *ring);
/* Host-only: PT2CT's limb-count selection (the type-level rules of Crypto/Alchemy/Interpreter/PT2CT/Noise.hs:107-170 and
 * PT2CT.hs:132-140,234-249,281-296).  `moduli` is the circuit's modulus list in the order of the `Zqs` type list
 * (examples/Arithmetic.hs:29-34, examples/HomomRLWR.hs:37-43); a ring uses the shortest PREFIX of it with enough 6.1-bit
 * noise units, nested last-taken-outermost, i.e. the alch_ring of L limbs is created on moduli[L-1], ..., moduli[0].
 * Given the pNoise of an operation's OUTPUT, returns how many moduli its input, its key-switch hint and its output use,
 * and the pNoise its input must have (feed that to the operation before it: PT2CT resolves a circuit backwards).
 *   op ALCH_OP_MUL     mul_        (PT2CT.hs:160-177):  modSwitch . keySwitchQuad hint . modSwitch $ x * y
 *   op ALCH_OP_TUNNEL  linearCyc_  (PT2CT.hs:207-229):  modSwitch . tunnel hint . modSwitch
 * ALCH_E_INVALID when the list does not hold enough units (PT2CT's type error "You need more/bigger moduli!").
 * The hint's units: KSPNoise = p + KSAccumPNoise + 5 (Max32BitUnits) for TrivGad and + 0 for BaseBGad 2 are the reference's
 * (PT2CT.hs:139-140), which defines no other gadget.  For ALCH_GAD_BASEPOW2(w) the rule is THIS LIBRARY'S OWN:
 * + ceil((w - 1) / 6.1), the digit's extra w - 1 bits in 6.1-bit units.  It reproduces both: + 0 at w = 1, and a 30.5-bit digit
 * gives Max32BitUnits = 5. */
#define ALCH_OP_MUL 0
#define ALCH_OP_TUNNEL 1
int alch_select_limbs(const uint64_t *moduli, int n_moduli, int op, int gadget, int p_noise_out, int *L_in, int *L_hint,
                      int *L_out, int *p_noise_in);
/* Noise units a modulus holds: floor(log2 q / 6.1)  (mkModulus, Noise.hs:154-170). */
int alch_modulus_units(uint64_t q);
/* Host-only (no GPU needed): the root-rule constants of one modulus, for cross-checking against the
 * oracle: psi (primitive m-th root), and the smallest generator. */
int alch_host_root(uint32_t m, uint64_t q, uint64_t *psi, uint64_t *generator);
int alch_ring_n(const alch_ring *ring, uint32_t *n, int *L, int *word_bytes);
/* Use an externally created hipStream_t (e.g. torch's current stream) for all work of this ring.
 * Guarantee: the call first waits for everything the ring has queued on its previous stream, so no work is lost; from then on every
 * kernel and copy of this ring's entry points -- including the ones another ring's call queues "as part of this ring's pipeline"
 * (tunnel, modSwitch, mul_ across rings) -- is queued on `hip_stream` or on internal streams that fork from it and join it again
 * before the call returns.  Work the caller queued on `hip_stream` before a call is therefore seen by the call, and work queued on
 * it after the call sees the call's results; buffers of other rings are ordered against it with events exactly as for a stream the
 * library created.  Every value of `hip_stream` names a stream: the null stream (0, what torch.cuda.current_stream() is
 * unless the caller switched streams) is accepted and is used as such.  The stream stays the caller's: the library never destroys
 * it (alch_ring_destroy waits for the work queued on it and destroys only the ring's internal streams), and the caller keeps it
 * alive while the ring, or a ring that took it over through alch_ring_share_stream, still uses it. */
int alch_ring_set_stream(alch_ring *ring, void *hip_stream);
/* Launch-structure options of the fused hot-path kernels (results never depend on them; tests sweep them).  The
 * library reads no environment variable.  Names: "chunk" (ciphertexts per launch group, >= 8, default 1024),
 * "one_stream" (0/1: do not alternate chunks over two streams), "pipe" (1 = tensor kernels on one stream, one chunk ahead of the
 * key-switch kernels on the other; measured slower, default 0), "nstreams" (1 .. 4 independent pipelines the chunks rotate over; default 2,
 * 3 and 4 measured 2-4 % slower), "ks_map" (1 = limb-per-XCD item numbering of the key-switch kernel when L divides 8; no measurable
 * difference, default 0), "ks_rev" (1 = the key-switch kernel walks a chunk's ciphertexts last to first; no measurable difference, default 0),
 * "q30" (0 = rings whose moduli are all below 2^30 use the general kernels), "ks_grid" (persistent workgroups of the key-switch
 * kernel, default 4096), "ti_split" / "ti_grid" (form and grid of the tensor + crtInv kernel), "crt_half" (0 = whole-polynomial crt at 128 KiB), "rs_half" (1 = the closing rescale at n = 2^15 always as two launches of half-size workgroups), "tunnel_ep" (read by alch_tunnel_create on ring_s: 0 = transform
 * the embedded E'-coefficients at dimension phi(s') instead of phi(e')), "tunnel_fused" (alch_ct_tunnel with TrivGad hints: 2 or 4 = digit transforms and hint products in one kernel with that many digits side by side, 0 = through HBM), "tunnel_mac" (0 = the tunnel's hint inner product one Montgomery product at a time behind a separate evalLin pass; default 1: lazy 64-bit groups, k_tunnel_mac_e), "gen_nt" (threads per workgroup of the general-index transform kernels: 128, 256, 512; 0 = by ring size), "rs_lin" / "gen_fused" (0 = the
 * composed forms of the closing rescale / the general-index key switch), "scratch_mib", "rs_slots" (resident
 * workgroups of the closing rescale kernel; for alch_ct_mul_full the options of the hint's ring apply), "stream_dedicated" (1: the ring
 * gets a NEW stream with a hardware queue of its own -- set it before other rings borrow the stream.  Ordinary streams share the HIP
 * runtime's few hardware queues, and two streams that land on one queue run their kernels one after the other; a host that runs
 * independent sub-batches side by side gives each a dedicated stream (at most 32 alive per process: ALCH_E_UNSUPPORTED beyond, the ring
 * keeps its ordinary stream), see alchemy_amd/ringround.py). */
int alch_ring_set_option(alch_ring *ring, const char *name, long value);
int alch_sync(alch_ring *ring);
/* HIP-event timer on the ring's stream (what bench.py brackets the timed region with). */
int alch_timer_start(alch_ring *ring);
int alch_timer_stop(alch_ring *ring, float *elapsed_ms);

/* ---- Tensor methods on host buffers (one ring element, Lol layout, in place) --------------------
 * crt/crtInv: Tensor `crtFuncs` -> crt, crtInv; reached from every Cyc ring product under
 * (*) on CT (Crypto/Alchemy/Interpreter/Eval.hs:65-67) and keySwitchQuadCirc (Eval.hs:133). */
int alch_crt(alch_ring *ring, int64_t *data);
int alch_crtinv(alch_ring *ring, int64_t *data);
/* zipWithT (*), (+), (-) in one basis (CRT for mul): the pointwise half of a Cyc product. */
int alch_mul(alch_ring *ring, int64_t *a, const int64_t *b);
int alch_add(alch_ring *ring, int64_t *a, const int64_t *b);
int alch_sub(alch_ring *ring, int64_t *a, const int64_t *b);
/* Multiply limb j by scalar s[j] (scalarPow/scalarCRT product: toLSD/toMSD of SymmSHE). */
int alch_scale(alch_ring *ring, int64_t *a, const uint64_t *s);
/* mulG and divG families (Tensor mulGPow/mulGDec/mulGCRT, divGPow/divGDec/divGCRT; used by (*) on CT, which
 * applies mulG to every product coefficient, Eval.hs:65-67, and by decrypt, PT2CT.hs:91-99).  g = prod over the odd
 * primes p of m of (1 - zeta_p); identity for a two-power index.  divG returns ALCH_OK (Lol's Just) or
 * ALCH_NOT_DIVISIBLE (Lol's Nothing; the data are left untouched): as in lol-cpp, a Z_q limb fails when the odd
 * radical of m is not a unit mod q, an integer ring (alch_ring_create_nocrt with q = 0) when some coefficient of
 * (rad/g) a is not divisible by the radical.  divGCRT never fails. */
int alch_mulg_pow(alch_ring *ring, int64_t *a);
int alch_mulg_dec(alch_ring *ring, int64_t *a);
int alch_mulg_crt(alch_ring *ring, int64_t *a);
int alch_divg_pow(alch_ring *ring, int64_t *a);
int alch_divg_dec(alch_ring *ring, int64_t *a);
int alch_divg_crt(alch_ring *ring, int64_t *a);
/* Tensor l / lInv: decoding-basis coefficients -> powerful-basis coefficients and back (prefix sums / differences
 * along every odd-prime axis); what Cyc's toPow / toDec run, e.g. under modSwitch's rescaleDec (Eval.hs:130) and
 * decrypt's liftDec.  Identity for a two-power index. */
int alch_l(alch_ring *ring, int64_t *a);
int alch_linv(alch_ring *ring, int64_t *a);
/* Lol `decompose` for TrivGad followed by `reduce` of every digit (the first half of `switch` in
 * keySwitchQuadCirc, Eval.hs:133): c in the Pow basis; digits = L consecutive ring elements (each
 * n*L int64, Pow basis), digit i = centred lift of limb i reduced into every limb. */
int alch_decompose_triv(alch_ring *ring, const int64_t *c_pow, int64_t *digits);
/* The same for BaseBGad 2 (PT2CT.hs:140): per limb i, ceil(log2 q_i) balanced binary digits of the centred lift,
 * least significant first, the top digit absorbing the remainder; digits of limb 0 first.  *n_digits receives
 * their number D = sum_i ceil(log2 q_i); `digits` must hold D ring elements (pass NULL to query D only). */
int alch_decompose_base2(alch_ring *ring, const int64_t *c_pow, int64_t *digits, int *n_digits);
/* The same for any BaseBGad code (ALCH_GAD_BASE2, ALCH_GAD_BASEPOW2(w)): D = sum_i ceil(ceil(log2 q_i) / w) digits by the rule next to
 * the gadget defines.  ALCH_GAD_TRIV and unknown codes: ALCH_E_INVALID.  Added within 1.8; probe for the symbol. */
int alch_decompose_baseb(alch_ring *ring, int gadget, const int64_t *c_pow, int64_t *digits, int *n_digits);
/* Host-only: the number of gadget entries D of any gadget code on this ring (L for ALCH_GAD_TRIV).  ALCH_E_INVALID: null argument,
 * unknown code.  Added within 1.8; probe for the symbol. */
int alch_gadget_digits(const alch_ring *ring, int gadget, int *D);

/* ---- device-resident ring-element arrays --------------------------------------------------------
 * What a Haskell `ForeignPtr`-wrapped tensor would hold; upload/download do the AoS <-> limb-major
 * transpose (and the 64 -> 32 bit narrowing when the ring uses 32-bit words). */
int alch_buf_alloc(alch_ring *ring, size_t n_elems, alch_buf **out);
int alch_buf_free(alch_buf *buf);
/* A non-owning alias of elements [first, first + count) of `parent` (same ring): lets the d_rel results of `coeffs` or the L digits
 * of `decompose` be handed on as single-element Tensor values without copies.  alch_buf_free of a view releases only the handle;
 * the parent must outlive its views (the Haskell side keeps the parent's ForeignPtr alive from the view's finalizer). */
int alch_buf_view(const alch_buf *parent, size_t first, size_t count, alch_buf **out);
/* Footprint.  A call stores nothing outside the ranges it is documented to write -- the words next to a view belong to the caller --
 * and leaves its inputs as they were; a count or an offset that leads past the end of a handle is ALCH_E_INVALID even where the
 * handle's parent has the room (DESIGN section 19 lists the span every entry point writes).
 * Overlapping ranges.  Views make two handles cover the same bytes, so every entry point that takes several ranges of one ring
 * compares BYTE ranges, not handles.  The rule: the range a call writes must share no byte with a range it reads -- touching
 * ranges (adjacent views of one parent) are fine -- and a violation is ALCH_E_INVALID with the function's name in
 * alch_last_error() and nothing launched.  Ranges that are only read may overlap freely (a == b is legal everywhere).  Where
 * an entry point differs:
 *   alch_buf_mul / _add / _sub / _scale   dst may START where a, b or src starts (any subset of them): in place
 *   alch_buf_mul_public, alch_ct_add_public   the same for dst / src; pub[pub_index] must lie outside the count (2 * batch)
 *                                         elements of dst, and may lie inside src
 *   alch_buf_add_public                   in place by definition; pub[pub_index] must lie outside all 2 * batch elements of cts,
 *                                         the c1 components (odd elements) included although only c0 is written
 *   alch_buf_decompose_triv               element src_index must lie outside dst[dst_first, dst_first + L)
 *   alch_buf_add_bcast, alch_pt_mul, alch_pt_rescale, alch_buf_lift, alch_buf_tensor_op, alch_buf_copy
 *                                         dst may start where its source starts (alch_buf_copy: a no-op); one[index] as pub above
 *   alch_ct_add                           out may start where an operand of the result's degree starts
 *   alch_hint_from_buf, alch_tunnel_create, alch_pt_linear_create   copy their sources: the sources may be overwritten afterwards
 * Entry points between two rings whose limb counts differ (alch_ct_mod_switch(_deg), alch_buf_rescale_drop0 / _add0) cannot be
 * given overlapping ranges: a view keeps its parent's ring.  Those that accept one ring on both sides (alch_buf_embed / _twace /
 * _coeffs with equal indices, alch_ct_tunnel from a ring to itself, alch_ct_mul_full with operands and result on one ring,
 * alch_buf_automorph, alch_ct_automorph, alch_ct_automorph_hoisted, alch_ct_automorph_lincomb) follow the rule without exception. */
int alch_buf_elems(const alch_buf *buf, size_t *n_elems);
/* Device address and size of the buffer (limb-major words, see above) for zero-copy hand-off to other device
 * code on the same GPU -- RCCL collectives that gather result batches, a caller's own kernels.
 * Work queued on the ring's stream must be ordered against the consumer by the caller (alch_sync or events). */
int alch_buf_device_ptr(const alch_buf *buf, void **ptr, size_t *bytes);
/* The ring a buffer belongs to, and the HIP device / stream a ring queues its work on: what other device code on the same GPU
 * needs to order itself against the library (include/alchemy_rccl.h queues its collectives on that stream). */
int alch_buf_ring(const alch_buf *buf, alch_ring **ring);
int alch_ring_device(const alch_ring *ring, int *device, void **hip_stream);
int alch_buf_upload(alch_buf *buf, size_t first, size_t count, const int64_t *host);
int alch_buf_download(const alch_buf *buf, size_t first, size_t count, int64_t *host);
/* Synthetic residues: word (e,j,k) = splitmix64(seed + ((e*L + j)*n + k)) mod q_j  (oracle:
 * orc_fill_uniform uses the same rule).  It fills TEST DATA, not secrets: it stays splitmix64 whatever the ring's key
 * (alch_ring_set_rng_key), and under a key the odd elements it writes are no longer the c1 of alch_ct_encrypt. */
int alch_buf_fill_uniform(alch_buf *buf, uint64_t seed);
/* Batched Tensor crt / crtInv / pointwise ops on elements [first, first+count). */
int alch_buf_crt(alch_buf *buf, size_t first, size_t count);
int alch_buf_crtinv(alch_buf *buf, size_t first, size_t count);
int alch_buf_mul(alch_buf *dst, const alch_buf *a, const alch_buf *b, size_t count);
int alch_buf_add(alch_buf *dst, const alch_buf *a, const alch_buf *b, size_t count);
int alch_buf_sub(alch_buf *dst, const alch_buf *a, const alch_buf *b, size_t count);
/* dst = src * s_j per limb (toLSD / toMSD scalars of SymmSHE, any basis); dst may equal src; a shifted overlap is refused
 * ("Overlapping ranges" above, as for the three calls before this one). */
int alch_buf_scale(alch_buf *dst, const alch_buf *src, size_t count, const uint64_t *s);
/* Batched l / lInv / mulG / divG on elements [first, first+count); basis = ALCH_BASIS_*.  alch_buf_divg returns
 * ALCH_NOT_DIVISIBLE when any element of the range is not divisible (the range is then unspecified). */
int alch_buf_l(alch_buf *buf, size_t first, size_t count);
int alch_buf_linv(alch_buf *buf, size_t first, size_t count);
int alch_buf_mulg(alch_buf *buf, size_t first, size_t count, int basis);
int alch_buf_divg(alch_buf *buf, size_t first, size_t count, int basis);
/* SymmSHE mulPublic (Crypto/Alchemy/Interpreter/Eval.hs:132; the first op of homomRLWR, examples/HomomRLWR.hs:52-59):
 * dst[e] = src[e] * pub[pub_index] for e < count, CRT basis (every component of every ciphertext times one public
 * ring element, already embedded / reduced into this ring by the host). */
int alch_buf_mul_public(alch_buf *dst, const alch_buf *src, const alch_buf *pub, size_t pub_index, size_t count);
/* SymmSHE addPublic (Eval.hs:131; PT2CT.hs:114-118 uses it for constants): cts[2b] += pub[pub_index] for b < batch
 * (c0 of every linear ciphertext; `pub` = the public element times l^-1 g^k, embedded, in the basis of cts). */
int alch_buf_add_public(alch_buf *cts, const alch_buf *pub, size_t pub_index, size_t batch);
/* SymmSHE addPublic with its encoding change as ONE pass (Eval.hs:131: addPublic works on the LSD form, i.e. toLSD's per-limb scalar
 * comes first): dst[e] = src[e] * s_j for every element e < 2*batch, then c0 components (even e) += pub[pub_index].  s = NULL: no
 * scalar.  dst may equal src.  Same results as alch_buf_scale followed by alch_buf_add_public. */
int alch_ct_add_public(alch_buf *dst, const alch_buf *src, size_t batch, const uint64_t *s, const alch_buf *pub, size_t pub_index);
/* Device-resident Lol `decompose` (TrivGad) + `reduce`: element `src_index` of src (Pow basis) -> L digit
 * elements written to dst[dst_first .. dst_first+L) (Pow basis). */
int alch_buf_decompose_triv(const alch_buf *src, size_t src_index, alch_buf *dst, size_t dst_first);
/* 64-bit order-independent checksum of elements [first, first+count): sum over words of
 * splitmix64(position ^ value<<20) -- used by the full-size parity tests. */
int alch_buf_checksum(const alch_buf *buf, size_t first, size_t count, uint64_t *sum);
/* The same sum with the words counted from element `position` of a larger array: the checksum of a batch that lives in several
 * buffers (sub-batches on their own streams, shards on their own GPUs) is the sum of its parts' checksums, each taken at the
 * position of the part's first element in the whole batch. */
int alch_buf_checksum_at(const alch_buf *buf, size_t first, size_t count, uint64_t position, uint64_t *sum);

/* ---- device-resident Tensor values -------------------------------------------------
 * E issues one Lol call per op (Crypto/Alchemy/Interpreter/Eval.hs:120-134) and Lol one Tensor call per basis change, so through
 * `instance Tensor GT` a ciphertext operation arrives as a chain of single-element calls.  A `GT` value may therefore hold an
 * alch_buf of ONE ring element instead of a host vector (haskell/.../GT.hs: constructor GTDev); these entry points are what its
 * methods call.  alch_buf_alloc / alch_buf_free of small buffers are served from a per-ring free list (no hipMalloc / hipFree, no
 * synchronisation; reuse is ordered on the ring's stream), and uploads / downloads of a few elements go through pinned staging
 * (no synchronisation on upload, one on download).
 *   alch_ring_share_stream   `ring` queues its work on the stream of `with` from now on: operations between the two rings
 *                            (embed / twace / coeffs, modSwitch, tunnel) then need no events.  A host that issues one Tensor call
 *                            at a time shares one stream between all its rings.
 *   alch_buf_copy            dst[dst_first + i] = src[src_first + i]
 *   alch_buf_tensor_op       dst[dst_first + i] = op(src[src_first + i]) for the unary Tensor methods, out of place (the ranges
 *                            may coincide: in place): crt / crtInv read src and write dst in one kernel, l / lInv / mulG / divG on
 *                            Pow and Dec likewise.  ALCH_T_DIVG_* return ALCH_NOT_DIVISIBLE for Lol's Nothing (dst unspecified). */
#define ALCH_T_CRT 0
#define ALCH_T_CRTINV 1
#define ALCH_T_L 2
#define ALCH_T_LINV 3
#define ALCH_T_MULG_POW 4
#define ALCH_T_MULG_DEC 5
#define ALCH_T_MULG_CRT 6
#define ALCH_T_DIVG_POW 7
#define ALCH_T_DIVG_DEC 8
#define ALCH_T_DIVG_CRT 9
int alch_ring_share_stream(alch_ring *ring, alch_ring *with);
int alch_buf_copy(alch_buf *dst, size_t dst_first, const alch_buf *src, size_t src_first, size_t count);
int alch_buf_tensor_op(alch_buf *dst, size_t dst_first, const alch_buf *src, size_t src_first, size_t count, int op);

/* ---- Tensor methods between two indices m | m'  ----------------------------------------------------
 * Lol's embedPow / embedDec / twacePowDec / coeffs and crtExtFuncs = (twaceCRT, embedCRT): what Cyc `embed`, `twace` and `coeffsCyc`
 * run, e.g. under SymmSHE encrypt / decrypt (Crypto/Alchemy/Interpreter/PT2CT.hs:84-99), mulPublic / addPublic (Eval.hs:131-132) and
 * tunnel (Eval.hs:134).  twaceCRT and embedCRT act on CRT SLOTS, so they must come from the same instance as crt / crtInv /
 * mulGCRT: they are computed from the slot rule at the top of this file (embedCRT: slot s of the big ring <- the slot of the small
 * ring whose unit is the unit of s reduced mod m; twaceCRT[t] = (mhat/mhat') g(t)^-1 sum over that fibre of g'(s) y[s], the
 * tweaked trace Tw(y) = (mhat/mhat') Tr(y g'/g)).  `small` has index m, `big` index m' (m | m'), same moduli (or both rings
 * without CRT over the same moduli: Pow / Dec forms only).
 *   embed   basis Pow: coefficient j of the small ring lands at its position in the big ring's powerful basis, zeros elsewhere;
 *           Dec: lInv_big . embedPow . l_small;  CRT: slot replication
 *   twace   basis Pow or Dec (Tensor twacePowDec: the same positions read back on either basis), or CRT
 *   coeffs  Tensor `coeffs`: the d_rel = phi(m')/phi(m) coefficient vectors over the small ring w.r.t. the relative powerful (or
 *           decoding: same positions) basis, relative indices in mixed radix, first prime outermost; dst holds d_rel * count elements,
 *           element e's coefficients at [e * d_rel, (e + 1) * d_rel).
 * Work is queued on the destination ring's stream, ordered after the source ring's. */
int alch_buf_embed(alch_buf *dst_big, const alch_buf *src_small, size_t count, int basis);
int alch_buf_twace(alch_buf *dst_small, const alch_buf *src_big, size_t count, int basis);
int alch_buf_coeffs(alch_buf *dst_small, const alch_buf *src_big, size_t count);
/* The same on host buffers (one ring element, Lol layout; `out` is distinct from `in`). */
int alch_embed_pow(alch_ring *small, alch_ring *big, const int64_t *in_small, int64_t *out_big);
int alch_embed_dec(alch_ring *small, alch_ring *big, const int64_t *in_small, int64_t *out_big);
int alch_embed_crt(alch_ring *small, alch_ring *big, const int64_t *in_small, int64_t *out_big);
int alch_twace_pow_dec(alch_ring *small, alch_ring *big, const int64_t *in_big, int64_t *out_small);
int alch_twace_crt(alch_ring *small, alch_ring *big, const int64_t *in_big, int64_t *out_small);
int alch_coeffs(alch_ring *small, alch_ring *big, const int64_t *in_big, int64_t *out_small_d_rel);
/* Host-only index tables of an index pair (no GPU needed; Lol computes the corresponding `baseIndicesPow` / `extIndicesCoeffs` in
 * Haskell): *len in = capacity of out (entries), out = entries written; out == NULL queries the length.
 *   ALCH_EXT_POW_POS   phi(m) entries: position in the big ring of the small ring's powerful-basis element j (Tensor powBasisPow:
 *                      the relative powerful basis element i is the unit vector at entry [i][0] of ALCH_EXT_COEFFS)
 *   ALCH_EXT_COEFFS    d_rel * phi(m) entries, [i][j]: position in the big ring of coefficient j of E-coefficient i
 *   ALCH_EXT_CRT_SLOT  phi(m') entries: the small ring's CRT slot behind every CRT slot of the big ring */
#define ALCH_EXT_POW_POS 0
#define ALCH_EXT_COEFFS 1
#define ALCH_EXT_CRT_SLOT 2
int alch_ext_table(uint32_t m_small, uint32_t m_big, int which, int32_t *out, size_t *len);
/* Tensor crtSetDec (host-only table construction, like the twiddle tables): the relative mod-p CRT set of O_m' / O_m for a prime p
 * not dividing m', as coefficient vectors over F_p on the decoding basis of index m' -- what Cyc's `crtSet` lifts to Z_{p^e} and
 * embeds, and `decToCRT` (examples/Common.hs:65-75) turns into the linear functions of the ring switches.  out: *count vectors of
 * phi(m') residues each, consecutive; *count in = capacity (vectors); out == NULL queries the number of CRT-set elements
 * (#<p>-cosets of Z_m'^* / #<p>-cosets of Z_m^*).  c_k is the idempotent that is 1 exactly at the primes above p indexed by I_k;
 * the I_k take one <p>-coset of Z_m'^* above every <p>-coset of Z_m^* (groups ordered by the smallest element of the coset below,
 * cosets inside a group by their smallest element, I_k = every group's k-th coset).  The set is canonical; its ORDER is this
 * library's rule (Lol's is not observable in the reference). */
int alch_crt_set_dec(uint32_t m_small, uint32_t m_big, uint32_t p, int64_t *out, size_t *count);

/* ---- key-switch hint ----------------------------------------------------------------------------
 * KSQuadCircHint gad (Cyc t m' zq) as produced by ksQuadCircHint
 * (Crypto/Alchemy/Interpreter/KeysHints.hs:101-113): one degree-1 polynomial (h0_i, h1_i) per gadget
 * digit.  host: 2*D consecutive ring elements in the CRT basis, order h0_0, h1_0, h0_1, h1_1, ... ;
 * D = L for TrivGad, sum_i ceil(log2 q_i) for BaseBGad 2 (digits of limb 0 first, least significant first;
 * alch_decompose_base2 reports D).
 * Kept device-resident (Montgomery form) for every later call. */
int alch_hint_load(alch_ring *ring, int gadget, const int64_t *host_crt, alch_hint **out);
/* Same, taking 2*L CRT-basis elements already on the device (e.g. synthetic). */
int alch_hint_from_buf(alch_ring *ring, int gadget, const alch_buf *src, alch_hint **out);
int alch_hint_free(alch_hint *hint);

/* ---- the hot path -------------------------------------------------------------------------------
 * out[b] = keySwitchQuadCirc hint (a[b] * b[b])  for b < batch: SymmSHE (*) (Eval.hs:65-67) followed
 * by keySwitchQuadCirc (Eval.hs:133) as PT2CT's mul_ sequences them (PT2CT.hs:172-177), on linear
 * ciphertexts.  a, b, out hold 2*batch ring elements: ciphertext b = elements (2b, 2b+1) = (c0, c1).
 * s_pre[j] = per-limb scalar folded into the tensor product: the product of both operands' toLSD
 * scalars and of keySwitchQuadCirc's toMSD scalar (p^-1 mod q_j when both operands are LSD); NULL = 1.
 * The (enc, k, l) metadata of SymmSHE's CT stays on the host (k1+k2+1, l1*l2 -- see
 * alchemy_amd/host/symmshe.hpp).  flags: ALCH_POW_IN / ALCH_POW_OUT; default is CRT basis in and out,
 * the representation Lol's Cyc keeps fresh ciphertexts and ring products in. */
int alch_ct_mul_relin(alch_ring *ring, const alch_hint *hint, const alch_buf *a, const alch_buf *b,
                      alch_buf *out, size_t batch, const uint64_t *s_pre, unsigned flags);

/* The complete PT2CT mul_ (PT2CT.hs:160-177):  out[b] = modSwitch (keySwitchQuadCirc hint (modSwitch (a[b] * b[b])))
 * -- SymmSHE (*) (Eval.hs:65-67), modSwitch to the hint's modulus (Eval.hs:130; PT2CTMulCtx'' "ModSwitchCtx_ ctin ->
 * hintzq", PT2CT.hs:142-158), keySwitchQuadCirc (Eval.hs:133), modSwitch to the output modulus.  Three rings with
 * the limb nesting of Noise.hs:82-89 (outermost = first): `hint` belongs to ring_h = (q_0 .. q_{Lh-1}); a and b
 * to ring_in = its last L_in limbs (L_in < Lh: KSPNoise gives a TrivGad hint one extra limb, PT2CT.hs:139);
 * out to ring_out = its last L_out limbs (L_out < Lh, at most 3 limbs dropped).  The rings are taken from the
 * handles; work is queued on ring_h's stream after everything queued so far on the other two, which in turn wait
 * for it.  s_pre[j] (j < L_in): toLSD scalars of both operands times the first modSwitch's toMSD scalar
 * (p^-1 mod q when both operands are LSD), NULL = 1; the library itself multiplies in the added moduli
 * (Rescale b -> (a,b): x -> (0, q_a x)) and performs both later toMSD as the identities they are.
 * flags: ALCH_POW_OUT leaves the result in the Pow basis (what Lol's rescale produces); operands are CRT basis.
 * BaseBGad 2 hints (composed from the entry points' own kernels): when the hint's ring has at least as many limbs as the operands',
 * both operands are switched up, then the BaseBGad key switch of alch_ct_mul_relin and the closing modSwitch.  When KSPNoise
 * (BaseBGad 2) leaves the hint on FEWER limbs than the product (PT2CT.hs:140 against :164; ring_h = the last limbs of ring_in) the
 * leading modSwitch goes down on the QUADRATIC ciphertext: tensor product on ring_in, c0 rescaled on the decoding basis, c1 and c2 on
 * the powerful basis, BaseBGad 2 digits of c2 on ring_h, hint products, closing modSwitch to ring_out. */
int alch_ct_mul_full(const alch_hint *hint, const alch_buf *a, const alch_buf *b, alch_buf *out, size_t batch,
                     const uint64_t *s_pre, unsigned flags);

/* ---- ring tunnelling ----------------------------------------------------------------
 * SymmSHE `tunnel hint` as E runs it (Eval.hs:134) between PT2CT's two modSwitch_ (PT2CT.hs:224-229), with the hint of
 * `tunnelHint f skout skin` (Crypto/Alchemy/Interpreter/KeysHints.hs:120-129); the linear functions of the reference are
 * `linearDec` lists (examples/Common.hs:65-75), the hops switch1..5 (examples/Common.hs:78-95).
 * ring_r = R'_q (input ciphertexts), ring_s = S'_q (hint and output), same moduli; E' = R' cap S' (index gcd), which must
 * satisfy Lol's tunnel conditions (alch_tunnel_info reports E' and d_rel = dim R'/E', or ALCH_E_INVALID).
 *   lin_crt : d_rel elements of ring_s, CRT basis: the values f'(d_i) of the E'-linear function on the relative decoding
 *             basis of R'/E' (Lol: `extendLin (lift f)` reduced mod q), i in the order of Tensor `coeffs`
 *   gadget  : ALCH_GAD_TRIV (examples/HomomRLWR.hs:46) or ALCH_GAD_BASE2 (examples/Tunnel.hs:24); D digits (alch_decompose_base2
 *             reports D for BaseBGad 2; D = L for TrivGad)
 *   ks_crt  : 2 * d_rel * D elements of ring_s, CRT basis: for relative index i and gadget digit t the linear hint
 *             (b, a) with b + a s_out = g_t f'(s_in p_i) + e   (p_i = relative powerful basis of R'/E'); order i, t, (b, a)
 * alch_ct_tunnel: out[b] = (f'(c0), 0) + sum_i switch(hint_i, embed(coeffsPow(c1)_i)) for linear ciphertexts with k = 0
 * (elements (2b, 2b+1)); s_pre = toMSD's per-limb scalar (NULL = 1).  CRT basis in and out unless ALCH_POW_IN /
 * ALCH_POW_OUT.  Runs on ring_s's stream; the input is not modified.
 * k > 0 (a ciphertext that has been multiplied): SymmSHE's `tunnel` runs absorbGFactors first -- every component times the element
 * reduce(liftPow(g^-k in R'_p)), a public multiplication (alch_buf_mul_public) that leaves k = 0 -- and then this call; the host mirror
 * (alchemy_amd/host/symmshe_gen.hpp, `tunnel`) and tests/test_gpu_tunnel.py do exactly that.
 * `in` may also belong to a ring holding only the LAST limbs of ring_r (same index): PT2CT emits
 * modSwitch_ .: tunnel_ hint .: modSwitch_ (PT2CT.hs:224-229) and the leading modSwitch up, x -> (0, q_a x), is then part of
 * this call -- the added limbs are zero, so their transforms, digits and hint products are skipped (same results as
 * alch_ct_mod_switch followed by alch_ct_tunnel; s_pre is indexed by ring_s's limbs either way).
 * TWO-POWER RINGS (since 1.7).  The same three entry points, with the same contract word for word (lin_crt, ks_crt order i, t, (b, a),
 * both gadgets, both word sizes, input on ring_r or on its last limbs, ALCH_POW_IN / ALCH_POW_OUT, input untouched, ring_s's stream),
 * serve a pair of two-power rings that are BOTH on the radix-16 engine (32 <= m; every size alch_ring_create accepts, the split sizes
 * included).  Every such pair is a tunnel; E' is the smaller ring.  Two shapes:
 *   up    r' | s' (r' = s' counts as down): R' = E' inside S', d_rel = 1, `coeffs` is the identity.  By the embedCRT rule and the bit-reversed
 *         slot order, crt_S'(embedPow x)[k] = crt_R'(x)[k >> sh] with n_s = 2^sh n_r: every transform runs at dimension n_r and the
 *         products with lin_crt / ks_crt read slot k >> sh; with CRT input c0 is not transformed at all.
 *   down  s' | r': S' = E', d_rel = n_r / n_s; E'-coefficient i of a Pow-basis element is the stride-d_rel subsequence of its coefficient
 *         vector that starts at i.  One crtInv at R', then d_rel (1 + D) transforms at n_s.
 * g = 1 and l = identity on a two-power index, so there is no lInv / l step.  The index maps are closed forms: no tables are built, and
 * the ring options "tunnel_ep", "tunnel_fused" and "tunnel_mac" are read by the general-index path only ("scratch_mib" applies to both).
 * NOT served: a pair with one ring on the radix-16 engine and the other on the general engine (a two-power partner below 32, or a
 * composite partner): alch_tunnel_create returns ALCH_E_UNSUPPORTED and says so.  Two rings of the general engine (two-power indices
 * below 32 among them) run the general-index path as before. */
int alch_tunnel_info(const alch_ring *ring_r, const alch_ring *ring_s, uint32_t *e_prime, uint32_t *d_rel);
int alch_tunnel_create(alch_ring *ring_r, alch_ring *ring_s, int gadget, const alch_buf *lin_crt, const alch_buf *ks_crt,
                       alch_tunnel **out);
int alch_tunnel_free(alch_tunnel *t);
int alch_ct_tunnel(const alch_tunnel *t, const alch_buf *in, alch_buf *out, size_t batch, const uint64_t *s_pre, unsigned flags);

/* ---- Galois automorphisms (added within 1.8; probe for the symbols) ---------------------------------------------------------------
 * sigma_j : zeta_m -> zeta_m^j for gcd(j, m) = 1, the third primitive of ciphertext arithmetic next to (+) and (*): on a plaintext a
 * rotation / permutation of its CRT slots, conjugation for j = -1.  The reference's evaluator has no such operation (its rotations are
 * ring tunnels); a ring-to-itself alch_ct_tunnel computes sigma_j only where it is E'-linear for a subring of index e' with j = 1 mod e',
 * at d_rel = phi(m') / phi(e') key switches.  These entry points cost ONE key switch for every unit j.
 * DEFINITION.  sigma_j fixes Z_q, so on the CRT basis it moves slots and nothing else.  By the slot rule at the top of this file slot(u)
 * holds a(omega_m^u), hence
 *       crt(sigma_j a)[slot(u)] = crt(a)[slot(u j mod m)]
 *   two-power index: slot k holds the unit 2 brev(k) + 1;  general index: slot (s_1..s_k) holds u = i0 + p i1 on every prime-power axis.
 * The permutation is the same for every limb and factorises over the prime-power axes.  j is reduced mod m everywhere.
 * ON CIPHERTEXTS.  (sigma_j c0, sigma_j c1) decrypts under sigma_j(s); one LINEAR key switch takes it back under s:
 *       out = (s_pre sigma_j c0, 0) + sum_t D_t (b_t, a_t),   D_t = the transformed gadget digits of s_pre sigma_j c1,
 * with a hint b_t + a_t s = g_t sigma_j(s) + e_t -- what alch_ct_ks_hint writes for n_v = 1 and v = sigma_j(s).  That key switch is
 * exactly the tunnel from the ring to itself with lin_crt = crt(1) (d_rel = 1). */
/* Host-only (no GPU needed), like alch_ext_table: out[k] = the SOURCE slot of destination slot k, k < phi(m).  *len in = capacity of
 * out (entries), out = phi(m); out == NULL queries the length.  ALCH_E_INVALID: null len, capacity too small, gcd(j, m) != 1, m = 0.
 * ALCH_E_UNSUPPORTED: an index neither engine serves (alch_ring_create's rule without its word-size test: an odd prime above 13,
 * phi(m) > 65535, a two-power m > 2^17). */
int alch_automorph_table(uint32_t m, uint32_t j, uint32_t *out, size_t *len);
/* dst[dst_first + e] = sigma_j(src[src_first + e]), e < count: both buffers on one ring with a CRT basis, elements in the CRT basis.
 * Queued on the ring's stream; the source is left as it was.  A gather cannot run in place: the written range must share no byte with
 * the read range ("Overlapping ranges" above; adjacent views are fine), else ALCH_E_INVALID naming this function, nothing launched.
 * Two-power m >= 32 (the split sizes included): the source slot is a closed form per lane, no table; any other index: a phi(m)-entry
 * device table cached in the ring per j.  count = 0: ALCH_OK, nothing queued.  Statuses, in this order: ALCH_E_INVALID (null buffer;
 * different rings; a range outside its buffer), ALCH_E_NO_CRT (a ring from alch_ring_create_nocrt), ALCH_E_INVALID (j not a unit;
 * overlap), device errors last. */
int alch_buf_automorph(alch_buf *dst, size_t dst_first, const alch_buf *src, size_t src_first, size_t count, uint32_t j);
/* The ciphertext operation.  The handle is the library's `alch_automorph`, declared as an untyped `void *` for the reason given at
 * alch_pt_linear_create (the FFI check's type table has no entry for a new handle type); alchemy_amd.Automorph wraps it.
 *   gadget  any gadget code, ALCH_GAD_BASEPOW2(w) included; D = its digit count on `ring` (alch_gadget_digits)
 *   ks_crt  2 * D elements of `ring`, CRT basis, the layout of alch_hint_from_buf: b_0, a_0, b_1, a_1, ... with
 *           b_t + a_t s = g_t sigma_j(s) + e_t.  Copied (Montgomery form) at create time: the source may be overwritten afterwards.
 * alch_ct_automorph serves linear ciphertexts with k = 0 (elements (2b, 2b+1)), `in` and `out` on `ring`, CRT basis in and out;
 * s_pre = toMSD's per-limb scalar (NULL = 1).  The result is WORD FOR WORD what alch_buf_automorph on the batch followed by
 * alch_ct_tunnel from the ring to itself (lin_crt = crt(1), the same ks_crt) returns: the gather goes into a scratch area of the ring,
 * the tunnel's key-switch stage runs on it; both walk the batch in chunks of at most "scratch_mib".  The input is not modified; `out`
 * must not overlap `in`.  ALCH_POW_IN / ALCH_POW_OUT: ALCH_E_UNSUPPORTED (on the powerful basis sigma_j is not a permutation; callers
 * transform).  k > 0: absorbGFactors first, exactly as documented for alch_ct_tunnel.  batch = 0: ALCH_OK, nothing queued.
 * Free the handle with alch_automorph_free when no call is using it (it does not take the device lock, like the other *_free). */
int alch_automorph_create(alch_ring *ring, uint32_t j, int gadget, const alch_buf *ks_crt, void **out);
int alch_automorph_free(void *a);
int alch_ct_automorph(const void *a, const alch_buf *in, alch_buf *out, size_t batch, const uint64_t *s_pre, unsigned flags);

/* ---- Hoisted automorphisms (added within 1.8; probe for the symbols) ---------------------------------------------------------------
 * Several sigma_j of the SAME ciphertexts at ONE gadget decomposition.  Almost all of alch_ct_automorph's key switch is the
 * decomposition of c1 and the forward transforms of its D digits; sigma_j fixes Z_q, the gadget entries g_t are constants of Z_q, so
 * with s_pre c1 = sum_t g_t d_t also sigma_j(s_pre c1) = sum_t g_t sigma_j(d_t), the sigma_j(d_t) as short as the d_t.  On the CRT
 * basis sigma_j is the slot permutation src_j (alch_automorph_table), hence
 *       out_j.c0[k] = s_pre c0[src_j[k]] + sum_t crt(d_t)[src_j[k]] b_{j,t}[k]
 *       out_j.c1[k] =                      sum_t crt(d_t)[src_j[k]] a_{j,t}[k]
 * is a key switch of sigma_j(ct) under the hint alch_automorph_create takes for j: one decomposition and D transforms for all the
 * rotations, one gathered inner product per rotation.  WORD FOR WORD, with j' the inverse of j mod m and h' = alch_buf_automorph by j'
 * of the hint, out_j = alch_buf_automorph_j(alch_ct_tunnel(identity tunnel from crt(1) and h')(ct, s_pre)).  It equals
 * alch_ct_automorph's words for j = 1, and for TrivGad on two-power rings; elsewhere the digits differ (decompose-then-permute against
 * permute-then-decompose), both are valid key switches with the same noise bound.
 *   alch_automorph_set_create   n_j units (1 <= n_j <= 32; each reduced mod m, repeats allowed), one gadget; ks_crt holds the n_j
 *           hints one after the other, 2 * D elements each in the layout and meaning of alch_automorph_create.  Copied (Montgomery
 *           form) at create time.  The handle is the library's `alch_automorph_set`, an untyped `void *` like alch_automorph's.
 *           Statuses, in this order: ALCH_E_INVALID (null argument; unknown gadget; the hint on another ring), ALCH_E_NO_CRT,
 *           ALCH_E_INVALID (n_j outside 1..32; a j that is no unit; fewer than n_j * 2 * D hint elements), device errors last.
 *   alch_ct_automorph_hoisted   linear ciphertexts with k = 0, CRT basis in and out, `in` (batch ciphertexts) and `out` on the set's
 *           ring.  out holds n_j * batch ciphertexts: rotation r of ciphertext b at elements 2 (r batch + b) and 2 (r batch + b) + 1.
 *           ALCH_AUTO_SUM: out holds batch ciphertexts, sum_r out_(j_r)[b] (rotate-and-sum, traces), from one launch per chunk.
 *           s_pre = toMSD's per-limb scalar (NULL = 1).  Runs on the ring's stream in chunks of at most "scratch_mib"; the input is
 *           not modified; out shares no byte with in.  batch = 0: ALCH_OK, nothing queued.
 *           Statuses, in this order: ALCH_E_INVALID (null argument; buffers of another ring; an unknown flag), ALCH_E_UNSUPPORTED
 *           (ALCH_POW_IN / ALCH_POW_OUT), ALCH_E_INVALID (a buffer shorter than its ciphertexts; out overlapping in), device errors.
 * Free the set with alch_automorph_set_free when no call is using it. */
int alch_automorph_set_create(alch_ring *ring, uint32_t n_j, const uint32_t *j, int gadget, const alch_buf *ks_crt, void **out);
int alch_automorph_set_free(void *set);
int alch_ct_automorph_hoisted(const void *set, const alch_buf *in, alch_buf *out, size_t batch, const uint64_t *s_pre, unsigned flags);

/* ---- Weighted sums of hoisted rotations (added within 1.8; probe for the symbol) ------------------------------------------------------
 * The diagonals of a slot-wise linear map: every rotation of the set times its own public CRT-basis element, summed, for n_out
 * weightings (rows) of the same rotations at ONE gadget decomposition and without the rotations ever reaching memory.  With y_r[b]
 * rotation r of ciphertext b as alch_ct_automorph_hoisted(set, in, ., batch, s_pre, 0) stores it, WORD FOR WORD
 *       out[g batch + b].c_i[k] = sum_(r < n_j) w[w_first + g n_j + r][k] * y_r[b].c_i[k]   (mod q_limb),   i = 0, 1
 * every stored word in [0, q): the words of that call followed by alch_buf_mul_public per (g, r) and alch_buf_add.  n_out = 1 with
 * every weight crt(1) gives ALCH_AUTO_SUM's words; a row with crt(1) at r0 and zero elsewhere gives rotation r0.
 *   w_crt   n_out * n_j CRT-basis elements of the set's ring from element w_first on, element w_first + g n_j + r the weight of
 *           rotation r in row g: canonical residues, NOT in Montgomery form.  Read at call time in stream order, not copied.
 *   in      batch linear ciphertexts with k = 0, CRT basis; s_pre as for alch_ct_automorph_hoisted.
 *   out     n_out * batch ciphertexts, row g of ciphertext b at elements 2 (g batch + b) and 2 (g batch + b) + 1.
 * Runs on the ring's stream in chunks of at most "scratch_mib", the rows in blocks of four per launch (a call with more rows redoes
 * the inner products per block).  The input and the weights are not modified; out shares no byte with in or with the weight range.
 * batch = 0 or n_out = 0: ALCH_OK, nothing queued.  Statuses, in this order: ALCH_E_INVALID (null argument; buffers of another ring;
 * an unknown flag -- ALCH_AUTO_SUM is unknown here), ALCH_E_UNSUPPORTED (ALCH_POW_IN / ALCH_POW_OUT), ALCH_E_INVALID (a buffer shorter
 * than its ciphertexts or weights; out overlapping in or the weights), device errors. */
int alch_ct_automorph_lincomb(const void *set, const alch_buf *w_crt, size_t w_first, size_t n_out, const alch_buf *in, alch_buf *out, size_t batch,
                              const uint64_t *s_pre, unsigned flags);

/* ---- SymmSHE modSwitch on batches of linear ciphertexts (Eval.hs:130; the two modSwitch_ of PT2CT.hs:177 and :224-229) ----
 * The rings come from the handles; the smaller ring's moduli are the LAST limbs of the bigger ring's (Noise.hs:82-89).  The
 * ciphertexts are in MSD form already (apply toMSD's per-limb scalar with alch_buf_scale first).
 *   out has more limbs: Rescale b -> (a, b) -- added limbs 0, the others times the added moduli; any basis, flags ignored.
 *   out has fewer limbs: Rescale (a, b) -> b per dropped limb (any number), c0 rescaled on the Dec basis and c1 on the Pow basis
 *   (Lol: rescaleDec / rescalePow); CRT basis in and out unless ALCH_POW_IN / ALCH_POW_OUT.  The input is not modified. */
int alch_ct_mod_switch(const alch_buf *in, alch_buf *out, size_t batch, unsigned flags);

/* ---- mul_ one SHE operation at a time on resident ciphertext batches (added within 1.8; probe for the symbols) ------------
 * PT2CT emits a multiplication as four object-language operations, modSwitch_ . keySwitchQuad_ hint . modSwitch_ $ x *: y
 * (PT2CT.hs:160-177), E binds each on its own (Eval.hs:65-67,130,133) and the ErrorRateWriter logs a rate after each
 * (ErrorRateWriter.hs:122,194,197).  These three entry points, with alch_ct_mod_switch, are those four operations: the quadratic
 * ciphertext exists in a caller's buffer and alch_ct_decrypt_lift (degree 2) can look at it.  They are the inspection path -- composed
 * from element-wise kernels and batched transforms at every size; alch_ct_mul_relin / alch_ct_mul_full stay the fast one and give the
 * same words.
 * A quadratic ciphertext b is elements (3b, 3b+1, 3b+2) = (c0, c1, c2): the layout alch_ct_error_term documents for degree = 2.
 * CRT basis in and out unless ALCH_POW_IN / ALCH_POW_OUT.  batch = 0: ALCH_OK, nothing done.  The input is never modified and `out`
 * must not alias it.  Statuses, in this order: ALCH_E_INVALID (null handle; handles of different rings; buffer too small; unknown
 * flag; degree not 1 or 2; the smaller ring's moduli not the last limbs of the bigger ring's), ALCH_E_NO_CRT (a ring created with
 * alch_ring_create_nocrt), device errors last. */
/* SymmSHE (*) on linear ciphertexts (Eval.hs:65-67): out[b] = s_pre * mulG(a[b] (x) b[b]),
 * (c0,c1,c2) = (a0 b0, a0 b1 + a1 b0, a1 b1), mulG on every component (identity on a two-power index).
 * s_pre[j] = product of both operands' toLSD scalars (NULL = 1).  a, b: 2*batch elements, out: 3*batch, one ring. */
int alch_ct_mul(alch_ring *ring, const alch_buf *a, const alch_buf *b, alch_buf *out, size_t batch,
                const uint64_t *s_pre, unsigned flags);

/* keySwitchQuadCirc hint (Eval.hs:133) on resident quadratic ciphertexts of the hint's ring:
 * out[b] = s_pre*(c0, c1) + sum_d crt(digit_d(s_pre*c2)) * hint_d.   s_pre = toMSD's per-limb scalar (NULL = 1).
 * TrivGad and BaseBGad 2; every ring alch_ring_create accepts, the split sizes included.  in: 3*batch, out: 2*batch.
 * The ring's launch options select among equivalent forms of the digit stage and never change a result. */
int alch_ct_key_switch_quad(const alch_hint *hint, const alch_buf *in, alch_buf *out, size_t batch,
                            const uint64_t *s_pre, unsigned flags);

/* alch_ct_mod_switch for ciphertexts of degree 1 or 2 ((degree+1)*batch elements on both sides): up = every component
 * times the added moduli; down = c0 rescaled on the decoding basis, every higher component on the powerful basis
 * (SymmSHE modSwitch; for degree 2 the same recollection alch_ct_mul_full's BaseBGad-2 "fewer limbs" path already rests on).
 * degree 1 gives alch_ct_mod_switch's results word for word.  Two rings on different streams are ordered as alch_ct_mod_switch
 * orders them. */
int alch_ct_mod_switch_deg(const alch_buf *in, alch_buf *out, size_t batch, int degree, unsigned flags);

/* ---- SymmSHE (+), (-), negate on resident batches, operands unaligned (added within 1.8; probe for the symbol) --------------
 * add_ = pureE (+) and neg_ = pureE negate on ciphertexts (Eval.hs:59-60, PT2CT.hs:117-118).  SymmSHE's (+) aligns its operands
 * first: the g-power k (mulG on the operand with the smaller k), the Z_p scalar l, the MSD / LSD encoding, and the degree (a
 * quadratic ciphertext before its key switch plus a linear one).  Every one of these is a per-limb scalar or a power of g, so a
 * whole unaligned sum is ONE element-wise pass:
 *       out[ct] = s_a * g^g_a * a[ct]  +  s_b * g^g_b * b[ct]        component by component, mod q_j
 * The (enc, k, l, degree) metadata stays on the host, as for alch_ct_mul; alchemy_amd/ctadd.py (`align`) turns two metadata
 * records into (s_a, g_a, s_b, g_b) by the rule of DESIGN section 16 -- subtraction and negate are the scalar's sign.
 *   layouts  a ciphertext of degree d is elements (d + 1) ct .. (d + 1) ct + d (alch_ct_mul's layout for d = 2); deg_a, deg_b in
 *            {1, 2}; out has degree max(deg_a, deg_b).  A c2 that only one operand has is scaled and stored as it is.
 *   s_x      L plain residues (reduced mod q_j like alch_buf_scale's), NULL = 1.   g_x <= 16; ignored where g = 1 (two-power index).
 *   b NULL   the unary form out = s_a * g^g_a * a (deg_b, s_b, g_b ignored): negate, mulG or toMSD / toLSD of whole ciphertexts.
 *   flags    0: CRT basis in and out (g^d is a pointwise factor read from the ring's table).  ALCH_POW_IN | ALCH_POW_OUT: Pow basis
 *            in and out; on a general index an operand with a non-zero g-power first goes through the batched mulG of the Pow basis
 *            into the ring's scratch, in chunks of at most "scratch_mib".  One flag alone: ALCH_E_UNSUPPORTED (alch_buf_crt exists).
 *   aliasing out may BE a or b when that operand has the result's degree; any other overlap is ALCH_E_INVALID.  a may be b.
 * Statuses, in this order: ALCH_E_INVALID (null out or a; buffers of different rings; a degree outside {1, 2}; unknown flag;
 * g_x > 16; a buffer smaller than (degree + 1) * batch; overlap), ALCH_E_UNSUPPORTED (one basis flag alone), ALCH_E_NO_CRT (a ring
 * from alch_ring_create_nocrt asked for a g-power on the CRT basis; such a ring is ALCH_E_UNSUPPORTED otherwise, as for
 * alch_buf_scale), device errors last.  batch = 0: ALCH_OK, nothing launched.  All three buffers belong to one ring, so the work
 * is ordered by that ring's stream alone. */
int alch_ct_add(alch_buf *out, size_t batch, const alch_buf *a, int deg_a, const uint64_t *s_a, unsigned g_a,
                const alch_buf *b, int deg_b, const uint64_t *s_b, unsigned g_b, unsigned flags);

/* ---- decrypt and errorRate_ on resident ciphertext batches (since 1.8) -------------------------------------------------
 * SymmSHE decrypt (Crypto/Alchemy/Interpreter/PT2CT.hs:91-99) and errorTermUnrestricted as the ErrorRateWriter interpreter logs it
 * (Eval.hs:150-160) both start from c(s), the ciphertext polynomial evaluated at the secret key, on the decoding basis, and lift
 * it, centred, from Z_q to the integers.  The lift never leaves word arithmetic: the mixed-radix (Garner) digits
 * x = d_0 + q_0 (d_1 + q_1 (d_2 + ...)), d_j in [0, q_j), are compared with ((q_j - 1)/2)_j from the top limb down (all moduli are
 * odd, so there is no tie), and |x| is again a digit vector.  What is left of decrypt stays composed from alch_buf_divg (k times,
 * on the Z_p ring), alch_buf_twace and alch_buf_l; `l_scalar` commutes with all of them and is folded into the lift.
 * Work is queued on the source ring's stream; a destination ring on another stream is ordered before and after it, as
 * alch_ct_mul_full orders its three rings.  batch = 0 / count = 0: ALCH_OK, nothing done.  max_digits is a HOST array, filled when
 * the call returns (one synchronisation of the stream; none without it). */
/* out[out_first + b] = c_b(s) for b < batch: ciphertext b = elements ((degree+1) b ..) of `in`; degree 1 or 2; sk = element
 * sk_index of sk_crt (CRT basis, same ring); s_pre = toLSD's per-limb scalar (NULL = 1).  CRT basis in (ALCH_POW_IN: Pow);
 * result on the DECODING basis (crtInv, then lInv on a general index) -- the object errorTermUnrestricted lifts.  Input untouched. */
int alch_ct_error_term(const alch_buf *in, size_t batch, int degree, const alch_buf *sk_crt, size_t sk_index,
                       const uint64_t *s_pre, alch_buf *out, size_t out_first, unsigned flags);

/* Centred lift mod Q = prod q_j of every coefficient of src[first .. first+count) (Pow or Dec basis; the basis is the caller's).
 *   dst_zp (nullable): a ring of the SAME index with ONE modulus p (alch_ring_create_nocrt or a CRT ring): element dst_first + i
 *                      = l_scalar * (lift mod p) mod p.
 *   max_digits (nullable): count * L words; the mixed-radix digits (limb 0 least significant) of max_k |lift| of each element. */
int alch_buf_lift(const alch_buf *src, size_t first, size_t count, alch_buf *dst_zp, size_t dst_first, uint64_t l_scalar,
                  uint64_t *max_digits);

/* Both in one call for a batch of ciphertexts -- what decrypt and errorRate_ need.  c(s) stays in a scratch area the ring keeps
 * (at most 1 GiB; larger batches are walked in chunks of that size), so nothing but the residues and the digits is written. */
int alch_ct_decrypt_lift(const alch_buf *in, size_t batch, int degree, const alch_buf *sk_crt, size_t sk_index,
                         const uint64_t *s_pre, alch_buf *dst_zp, size_t dst_first, uint64_t l_scalar, uint64_t *max_digits,
                         unsigned flags);

/* ---- plaintext ring elements on resident batches (added within 1.8; probe for the symbols) ----------------------------------
 * The reference runs every example twice, on plaintexts and homomorphically, and compares (examples/HomomRLWR.hs, examples/Arithmetic.hs):
 * E evaluates the same mul_, div2_ and linearCyc_ on `Cyc t m zp` (Eval.hs:65-67, 72-88, 136-148) that PT2CT turns into ciphertext
 * operations.  These entry points are that half on resident batches of rings WITHOUT a CRT basis (alch_ring_create_nocrt: Z_{2^e}, Z_7).
 * Products run over a LIFTING RING, as Lol multiplies over an extension ring when Z_p has no CRT basis: any ring from alch_ring_create
 * with the plaintext ring's index; Q = the product of its moduli.  Residues are lifted centred to the integers (|z| <= p/2), reduced
 * into every limb, the ring operation runs exactly mod Q, and the result is lifted centred mod Q and reduced mod p.
 * EXACTNESS.  On the powerful basis of index m the product of two elements with integer coefficients bounded by A has coefficients
 * bounded by phi(m) * 2^w * A^2, w = the number of ODD primes of m: coefficient k of a*b is sum_{i,j} s(i,j,k) a_i b_j with s in
 * {0, +1, -1}; the powerful basis is a tensor product over the prime powers m_l of m, and on each axis the exponent i_l + j_l mod m_l
 * either is k_l itself or, past phi(m_l), reduces modulo Phi_{m_l} to minus a sum that contains k_l -- so for given (i, k) at most two
 * j_l contribute, and for a power of two exactly one (the two candidates differ by m_l / 2 = phi(m_l)).  A sum of t such products:
 *       bound(t, m, p) = t * phi(m) * 2^w * floor(p/2)^2          (alch_pt_bound computes it)
 * Every entry point below that multiplies computes the bound and returns ALCH_E_INVALID, with a message, unless Q/2 > bound: a
 * product that could wrap is never silently wrong.  (Two 31-bit primes, Q/2 ~ 2^61, hold phi(m) = 2^12, w = 3, t = 8 up to
 * p = 2^22: far beyond the reference's Z_{2^e}, e <= 5.)
 * RESTRICTIONS.  Every *_zp buffer belongs to a ring with exactly one modulus 2 <= p < 2^31 (32-bit words); the lifting ring has the
 * SAME index as the plaintext ring it serves; alch_pt_rescale needs p' | p.  Powerful basis in and out everywhere.
 * Common rules: count = 0 is ALCH_OK with nothing launched; ranges that would wrap are refused; inputs are never modified; work is
 * queued on the lifting ring's stream (alch_pt_rescale: the destination ring's), and buffers of rings on other streams are ordered
 * before and after it, as alch_ct_decrypt_lift orders its rings.  Products stay in the lifting ring's scratch, walked in chunks of at
 * most "scratch_mib".  Statuses, in this order: ALCH_E_INVALID (null handle; buffers of different rings; unknown flag; a plaintext
 * ring with several moduli or p >= 2^31; a lifting ring of another index), ALCH_E_NO_CRT (a lifting ring from
 * alch_ring_create_nocrt), ALCH_E_INVALID (count out of bounds; Q too small for the bound; shifted overlaps), device errors last. */
/* Host-only: the bound above for a t-term sum (1 <= terms <= 65536) as a 128-bit number (lo, hi). */
int alch_pt_bound(uint32_t m, uint64_t p, uint32_t terms, uint64_t *lo, uint64_t *hi);
/* Cyc (*) on plaintexts (Eval.hs:65-67 on `Cyc t m zp`): dst[e] = a[e] * b[e] in Z_p[zeta_m], e < count.  No mulG (that belongs to
 * SymmSHE's product, not Cyc's).  One plaintext ring for the three buffers; dst may BE an operand.  flags: none defined (0). */
int alch_pt_mul(alch_ring *lift, alch_buf *dst_zp, const alch_buf *a_zp, const alch_buf *b_zp, size_t count, unsigned flags);
/* A `Linear t zp e r s` as linearDec builds it (examples/Common.hs:65-75), e = gcd(r, s): ys_zp holds EXACTLY d_rel = phi(r)/phi(e)
 * elements of S_p (index s = lift_s's index) on the Pow basis, in the order of Tensor `coeffs` (ALCH_E_INVALID otherwise); they are
 * kept resident, lifted, in the CRT basis of lift_s.  m_r = r.  Only lift_s needs a CRT basis; r and e may be any indices (two-power or
 * not: only index tables touch them -- H0 = F128 -> H1 = F448 is served).  The handle is the library's `alch_ptlin`, declared here as
 * an untyped `void *`: the mechanical check of the Haskell FFI module (tests/test_haskell_shim.py) maps every C parameter type of this
 * header to an FFI type through a fixed table, and that table has no entry for a new handle type -- a typed `alch_ptlin *` would break it.
 * Callers that want the type back wrap the pointer (alchemy_amd/host/cycgen.hpp: `Linear`; alchemy_amd.PtLinear).  Free it with
 * alch_pt_linear_free when no call is using it.  The bound is taken with t = d_rel. */
int alch_pt_linear_create(alch_ring *lift_s, const alch_buf *ys_zp, uint32_t m_r, void **out);
int alch_pt_linear_free(void *f);
/* evalLin (Eval.hs:141): dst[b] = sum_i y_i * embed(coeffsDec(src[b])_i), b < count.  src over index r, dst over index s, both on the
 * Pow basis with the function's p: the l / lInv steps are inside the call (folded into the resident y_i, so the Z_p intermediates
 * never exist in memory).  dst must not overlap src.  flags: none defined (0). */
int alch_pt_eval_lin(const void *f, const alch_buf *src_zp, alch_buf *dst_zp, size_t count, unsigned flags);
/* div2_ = rescalePow (Eval.hs:72-78) from Z_p to Z_p', p' | p, same index: dst = src / (p/p') coefficient-wise.  ALCH_NOT_DIVISIBLE
 * when some coefficient of the range is not divisible; dst then holds the floor quotients.  The flag is reduced on the device: the
 * call downloads one word and synchronises the destination ring's stream once. */
int alch_pt_rescale(const alch_buf *src_zp, alch_buf *dst_zp, size_t count);
/* addLit_ on a batch: dst[e] = src[e] + one[index], e < count; any ring with moduli (not the integers), any basis, one ring for the
 * three buffers; dst may be src.  The x * (1 + x) of the rescale tree uses it. */
int alch_buf_add_bcast(alch_buf *dst, const alch_buf *src, const alch_buf *one, size_t index, size_t count);

/* ---- encrypt on resident batches (added within 1.8; probe for the symbols) ------------------------------------------------------
 * SymmSHE encrypt (PT2CT.hs:84-87): an error term from the coset pt + p R on the decoding basis, a uniform c1, c0 = err - c1 s.  The
 * mirror image of alch_ct_decrypt_lift.  The error sampler is COUNTER-BASED: every stored word is an integer-exact function of
 * (seed, position), so a batch cut into chunks, the host mirror (alchemy_amd/host/cycgen.hpp: gaussDecCounter) and the Python model
 * of the tests give the same words.  Definition (arithmetic on seeds and counters mod 2^64):
 *   table      T[t] = floor(2^63 P(|K| <= t)), K ~ D_{Z,64}; 582 entries, the last one 2^63 - 1 (alch_gauss_table)
 *   deviate    coefficient i of element e, n = phi(m): c = (elem0 + e) n + i; w0 = splitmix64(seed + 2c), w1 = splitmix64(seed + 2c + 1);
 *              t = #{ j : T[j] <= w0 >> 1 }; k = (w0 & 1) ? -t : t; f = k 2^32 + (w1 >> 32) - 2^31; x = (double)f * scale
 *   scale      sigma / (sqrt(4096 + 1/12) * 2^32), sigma = sqrt(svar * (m / rad m) / (2 pi)) (alch_gauss_plan)
 *   correlate  for every odd prime p of m, ascending, the lower Cholesky factor of p I - J along the axis (the loop of tGaussianDec in
 *              cycgen.hpp), s = 0.0; s = s + Lc[i][k] * col[k] for k = 0 .. i, every product and every sum rounded on its own
 *   round      R(x) = sign(x) floor(|x| + 0.5); errorRounded: z = R(x); errorCoset with coset word v mod p: c = v centred,
 *              z = c + p R((x - c) / p); the stored word of limb j is z mod q_j, on the DECODING basis
 * splitmix64 is a STATISTICAL generator, not a cryptographic one -- like the mt19937_64 of the host path it stands beside.  A ring
 * with a key (alch_ring_set_rng_key, "keyed streams" below) takes w0, w1 from a ChaCha20 keystream instead.
 * Doubles cross the ABI as their IEEE-754 bit patterns in uint64_t. */
/* Host only (no device needed).  cdt = NULL: *len = the table's length; else *len >= that on entry, the table is copied. */
int alch_gauss_table(uint64_t *cdt, size_t *len);
/* Host only.  scale (nullable) and the Cholesky factors of the ODD primes of m, ascending, each row-major and full (p-1) x (p-1) with
 * zeros above the diagonal.  chol_bits = NULL: *chol_len = their total length; else *chol_len >= that on entry.
 * ALCH_E_INVALID: m < 1; svar not finite or <= 0. */
int alch_gauss_plan(uint32_t m, uint64_t svar_bits, uint64_t *scale_bits, uint64_t *chol_bits, size_t *chol_len);
/* dst[first + e], e < count: errorRounded (coset_zp = NULL) or errorCoset of scaled variance svar (the caller's: encrypt passes
 * svar * p^2) on the decoding basis, reduced into every modulus of dst's ring -- any ring of alch_ring_create or
 * alch_ring_create_nocrt (modulus 0, the integers: z itself).  coset_zp: a buffer of a ONE-modulus ring of the same index, modulus
 * 2 <= p < 2^31; element coset_first + e is the coset of element e.  elem0 only shifts the counters: calls over consecutive chunks
 * with elem0 advanced give the words of one call.  Work is queued on dst's ring; a coset ring on another stream is ordered before and
 * after it.  count = 0: ALCH_OK, nothing queued.  ALCH_E_INVALID: svar not finite or <= 0, or so large that |z| < 2^62 cannot be
 * guaranteed (from scale, the table length and the row sums of the Cholesky factors); index, modulus-count or device mismatch of the
 * coset ring; a range outside a buffer; overlapping ranges other than coset == destination.  ALCH_E_UNSUPPORTED: an odd prime of
 * the index above 13. */
int alch_buf_gauss_dec(alch_buf *dst, size_t first, size_t count, uint64_t svar_bits, const alch_buf *coset_zp, size_t coset_first,
                       uint64_t seed, uint64_t elem0);
/* out[2b] = err_crt[err_first + b] - c1 * sk_crt[sk_index], out[2b + 1] = c1, b < batch: `CT LSD 0 1 [c0, c1]`, everything on the CRT
 * basis of one ring.  Word (b, limb j, slot k) of c1 is splitmix64(seed + ((2 (ct0 + b) + 1) L + j) n + k) mod q_j: with ct0 = 0 the
 * words alch_buf_fill_uniform(out, seed) puts into the odd elements; ct0 shifts the ciphertext counter as elem0 does above.  A ring
 * with a key (alch_ring_set_rng_key) draws c1 from a ChaCha20 keystream, and then also refuses positions that would reach 2^58.
 * batch = 0: ALCH_OK, nothing queued.  ALCH_E_INVALID: null buffer; buffers of different rings; out smaller than 2 * batch; a range or
 * the key index outside its buffer; out overlapping err_crt's range or the key.  ALCH_E_NO_CRT: a ring without CRT basis. */
int alch_ct_encrypt(alch_buf *out, size_t batch, const alch_buf *err_crt, size_t err_first, const alch_buf *sk_crt, size_t sk_index,
                    uint64_t seed, uint64_t ct0);

/* ---- key-switch and tunnel hints on resident buffers (added within 1.8; probe for the symbol) --------------------------------------
 * ksHint (KeysHints.hs:101-129): for every value v_i and every gadget entry t an RLWE sample under the key with g_t v_i added.  The
 * gadget has D entries: D = L for ALCH_GAD_TRIV, D = sum_i ceil(log2 q_i) for ALCH_GAD_BASE2, the digits of limb 0 first, least
 * significant first (the order of alch_hint_load and alch_decompose_base2).  Entry t belongs to limb i(t) with exponent d(t) (0 for
 * TrivGad): g_t is 2^d(t) on limb i(t) and 0 on every other limb.  ALCH_GAD_BASEPOW2(w): D = sum_i ceil(ceil(log2 q_i) / w) in the
 * same order and g_t = 2^(w d(t)), which stays below q_i(t).  For i < n_v, t < D and e = i D + t, everything on the CRT basis of
 * one ring:
 *   out[out_first + 2e + 1] = a, word (limb j, slot k) = splitmix64(seed + ((2 (ct0 + e) + 1) L + j) n + k) mod q_j  (alch_ct_encrypt's
 *                             rule: ct0 cuts a long hint into chunks the same way)
 *   out[out_first + 2e]     = g_t v_crt[v_first + i] + err_crt[err_first + e] - a * sk_crt[sk_index]
 * n_v = 1 gives the layout of alch_hint_from_buf (h0_0, h1_0, h0_1, ...), n_v = d_rel the ks_crt of alch_tunnel_create.  The error
 * terms are the caller's (alch_buf_gauss_dec, l, crt).  splitmix64 is a STATISTICAL generator, not a cryptographic one; a ring with a
 * key (alch_ring_set_rng_key) draws a from a ChaCha20 keystream, and then also refuses positions that would reach 2^58.
 * n_v = 0: ALCH_OK, nothing queued.  ALCH_E_INVALID: null buffer; buffers of different rings; unknown gadget; a range or the key index
 * outside its buffer; the output range overlapping an input.  ALCH_E_NO_CRT: a ring without CRT basis. */
int alch_ct_ks_hint(alch_buf *out, size_t out_first, int gadget, size_t n_v, const alch_buf *v_crt, size_t v_first,
                    const alch_buf *err_crt, size_t err_first, const alch_buf *sk_crt, size_t sk_index, uint64_t seed, uint64_t ct0);
/* A part of the same hint, for callers that cannot hold every error term at once: the entries e_first <= e < e_first + e_count of the
 * hint of the values v_crt[v_first ..] (entry e belongs to value e / D and gadget entry e mod D; any cut, not only a multiple of D).
 * out_first, err_first and ct0 are those of entry e_first: out[out_first + 2 (e - e_first)], err_crt[err_first + e - e_first],
 * counter ct0 + e - e_first.  Consecutive parts with out_first, err_first and ct0 advanced by the entries done give the words of one
 * alch_ct_ks_hint call.  Statuses as above; v_crt must hold the values of every entry of the part. */
int alch_ct_ks_hint_part(alch_buf *out, size_t out_first, int gadget, size_t e_first, size_t e_count, const alch_buf *v_crt,
                         size_t v_first, const alch_buf *err_crt, size_t err_first, const alch_buf *sk_crt, size_t sk_index,
                         uint64_t seed, uint64_t ct0);

/* ---- keyed streams for the samplers (added within 1.8; probe for the symbols) ------------------------------------------------------
 * An opt-in 256-bit key per ring.  With a key set, the three samplers above draw their random words from ChaCha20 keystreams addressed
 * by (key, seed, domain, position) instead of splitmix64 on a counter; with no key set nothing changes, bit for bit.  The key of the
 * ring that is WRITTEN applies: dst of alch_buf_gauss_dec, out of alch_ct_encrypt, alch_ct_ks_hint and alch_ct_ks_hint_part.
 * alch_buf_fill_uniform never looks at it.  Definition (alchemy_amd/csrc/chacha_stream.hpp):
 *   block      ChaCha20, original layout, 20 rounds: state words 0-3 the constants 0x61707865 0x3320646e 0x79622d32 0x6b206574, words
 *              4-11 the key as eight little-endian 32-bit words, words 12, 13 a 64-bit block counter (low, high), words 14, 15 a
 *              64-bit nonce (low, high); output = working state + input state; u64[t] = word[2t] | word[2t+1] << 32, t < 8
 *   address    nonce = the call's `seed` as given; position 0 <= x < 2^58 (a plain integer) of domain 0 <= d < 256 has block counter
 *              (d << 56) | (x >> 2) and owns the pair (A, B) = (u64[2s], u64[2s+1]), s = x & 3
 *   domain 1   alch_buf_gauss_dec: x = c = (elem0 + e) n + i; w0 = A, w1 = B -- deviate, scale, correlation and rounding as above
 *   domain 2   alch_ct_encrypt: x = ((2 (ct0 + b) + 1) L + j) n + k; the c1 word is (B 2^64 + A) mod q_j
 *   domain 3   alch_ct_ks_hint / _part: the same x with e for b; the a word is (B 2^64 + A) mod q_j
 *   other domains are reserved.  One seed in two domains never shares keystream.
 * A uniform word taken from 128 bits is within 2^-66 of uniform (q < 2^62).  elem0 / ct0 still only shift x: a batch cut anywhere,
 * inside a block included, gives the words of one call.  A keystream must not wrap: a keyed call whose largest x would reach 2^58
 * -- (elem0 + count) n > 2^58, 2 (ct0 + batch) L n > 2^58, computed without wrap-around -- returns ALCH_E_INVALID with nothing
 * queued; unkeyed calls keep their arithmetic mod 2^64.
 * CLAIMED: the words are a ChaCha20 keystream under the caller's key; uniform words are within 2^-66 of uniform.  THE CALLER'S DUTY: a
 * (key, seed) pair is used for ONE batch per entry point, as any nonce is.  NOT CLAIMED: constant time (the table search and the
 * reductions depend on the words); a better Gaussian than the staircase above; anything about the host path's mt19937_64. */
#define ALCH_RNG_SPLITMIX 0
#define ALCH_RNG_CHACHA20 1
/* key: 32 bytes, copied into the ring under the device lock; NULL goes back to splitmix64.  The library keeps the key on the host only
 * (zeroed on reset and in alch_ring_destroy) and passes it to kernels by value: no device memory is allocated for it.  Any ring,
 * alch_ring_create_nocrt's included (the Gaussian writes into those). */
int alch_ring_set_rng_key(alch_ring *ring, const void *key);
/* ALCH_RNG_SPLITMIX or ALCH_RNG_CHACHA20; ALCH_E_INVALID: null ring. */
int alch_ring_rng(const alch_ring *ring);
/* Host only (no device needed): out[2i], out[2i + 1] = the pair (A, B) of position x0 + i, i < count, of (key, nonce, domain) -- the
 * definition made callable.  key: 32 bytes.  ALCH_E_INVALID: null pointer; domain > 255; x0 + count > 2^58. */
int alch_rng_words(const void *key, uint64_t nonce, unsigned domain, uint64_t x0, size_t count, uint64_t *out);

/* ---- modSwitch building block (Eval.hs:130) ---------------------------------------
 * Rescale (a,b) -> b on Pow-basis elements: src lives in ring_src (L limbs), dst in ring_dst whose
 * limbs are ring_src's limbs 1..L-1:  dst_j = q_0^-1 * (src_j - reduce(lift src_0)). */
int alch_buf_rescale_drop0(const alch_buf *src, alch_buf *dst, size_t count);
/* Rescale b -> (a,b) (modSwitch up, PT2CT.hs:177 first modSwitch_): dst lives in a ring whose limbs 1..L are
 * src's limbs and whose limb 0 is the added modulus q_a:  dst_0 = 0,  dst_{j+1} = q_a * src_j.  Any basis. */
int alch_buf_rescale_add0(const alch_buf *src, alch_buf *dst, size_t count);

#ifdef __cplusplus
}
#endif
#endif /* ALCHEMY_HIP_H */
