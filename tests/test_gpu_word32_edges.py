"""GPU: the 4-byte two-power kernels on extreme words at the edges of their modulus range.

A two-power ring runs on 4-byte words while every modulus is below 2^31.  The rest of the suite runs these kernels on uniform words,
and on extreme words only through k_ks_accum_half at n = 2^11 / 2^15 on the four largest primes; here they run
  * on the largest primes below 2^31 (2q fits a word with 2^17 to spare, 3q does not), on the first primes above 2^30 (the smallest
    that take the non-Harvey kernels) and on the largest below 2^30 (r->q30: Harvey's [0, 4q) butterflies with no headroom left),
  * on either side of r->balanced = (qmax - 1) / 2 < qmin, for a 31-bit and for a 30-bit qmax (EDGE_*), with a 31-bit limb next to a
    17-bit and a 20-bit one (MIXED), and with one limb on each side of 2^30 (STRADDLE30),
  * on words drawn from {0, 1, q-2, q-1, (q-1)/2, (q+1)/2} (helpers.extreme_words), with s_pre in {None, [q-1 ...]}.
Every case asserts 4-byte words on every ring it creates (a refused ring raises), compares every output word with the C restatement
(pinned to the by-definition model at these moduli by tests/test_oracle_word32.py, which also checks the classes of the moduli on
the CPU) and asserts that every stored word is below its modulus.

Kernels per case group, read off `dispatch` (run_call in kernels_ntt.hpp) and the host layer:
  1. test_crt_crtinv_and_products: k_crt<4 .. 15, u32, false / true>; at log n = 15 k_crt_half<15, u32, false / true> (option
     crt_half = 1) and k_crt<15, u32> (crt_half = 0); at log n = 16 k_crt_split; k_pointwise for the products.
  2. test_ct_mul_relin_off_the_half_sizes: k_tensor_intt<LOGN, u32> into k_ks_accum<LOGN, u32, true> (TOP4, ABOVE30, BELOW4,
     EDGE_BAL31, EIGHT_TOP) or k_ks_accum<LOGN, u32, false> (MIXED, MIXED_LAST, EDGE_UNBAL31), LOGN in {4, 8, 10, 13, 14};
     test_ct_mul_relin_every_product_at_its_maximum: the same and the k_ks_accum_half / k_ks_accum_split forms, L products (q-1)^2
     per slot; test_ct_mul_relin_n65536: k_tensor_crtinv_split + k_ks_accum_split (split_fused = 2 and 1), k_crt_split_digits (0).
  3. test_ct_mul_relin_digits_at_the_ends, at n = 2^15 (at n = 2^11 the tensor kernel is k_tensor_intt<11, u32> for every ring):
       ABOVE30, STRADDLE30, EDGE_BAL31     k_tensor_intt_split<15, false> into k_ks_accum_half<15, true>
       EDGE_UNBAL31                        k_tensor_intt_split<15, false> into k_ks_accum_half<15, false>
       EDGE_BAL30                          k_tensor_intt_split<15, true>  into k_ks_accum_half<15, true, 32, false, true>
       EDGE_BAL30, option q30 = 0          k_tensor_intt_split<15, false> into k_ks_accum_half<15, true>
       EDGE_UNBAL30                        k_tensor_intt_split<15, true>  into k_ks_accum_half<15, false>
       EDGE_UNBAL30, option q30 = 0        k_tensor_intt_split<15, false> into k_ks_accum_half<15, false>
  4. test_ct_mul_relin_base2_hint: k_tensor_ew, k_crt<LOGN, u32, true>, k_crt_base2_digits<LOGN, u32> (31 + 31, 31 + 17 and 30 + 30
     digits), k_hint_mac.
  5. test_ct_mul_full (LOGN in {8, 11, 15}): the tensor kernels of 2. / 3.; the key switch with dup > 0 -- k_ks_accum<8, u32, bal> and,
     at LOGN = 11 / 15, k_ks_accum_half<LOGN, true, 32, true> (TOP5), <LOGN, true, 32, true, true> (BELOW30),
     <LOGN, false, 32, true> (MIXED_FULL); the closing modSwitch
       4-5-3, 3-4-2, 2-3-1        k_rescale_out_lin<LOGN, u32, 2, true>
       3-4-3                      k_rescale_out_lin<LOGN, u32, 1, true>
       4-5-3-pow                  k_rescale_out<LOGN, u32>
       2-5-2                      k_rescale_out<LOGN, u32>; at LOGN = 15 k_rescale_drop_half + k_rescale_keep_half
       mixed-4-5-3                k_rescale_out<LOGN, u32>; at LOGN = 15 k_rescale_drop_half + k_rescale_keep_half
       mixed-4-5-4                k_rescale_out_lin<LOGN, u32, 1, false>
     test_ct_mul_full_n32768_options: 4-5-3 with rs_half = 1 (k_rescale_drop_half + k_rescale_keep_half) and with rs_lin = 0
     (k_rescale_out<15, u32>).
  6. test_ct_mul_full_rescale_at_the_ends (LOGN in {8, 15}): the kernels of 5. on lifts at the ends of the centred range --
     k_rescale_out_lin<LOGN, u32, 2, true> (top, edge_bal*-2-3-1), k_rescale_out<LOGN, u32> / the half-size pair at LOGN = 15
     (edge_unbal*-2-3-1, mixed), k_rescale_out_lin<LOGN, u32, 1, true> (*-2-3-2), and k_rescale_out<LOGN, u32> for Pow output.
  7. test_mul_steps_chain: alch_ct_mul (k_ct_tensor3), alch_ct_mod_switch_deg up and down, alch_ct_key_switch_quad one at a time, at
     n = 2^8 and 2^11, and the chain against alch_ct_mul_full.
  8. test_elementwise_decompose_and_rescale: k_pointwise (add, sub, mul), scale by q-1, (q+1)/2 and q-2, k_mul_bcast (mulPublic), k_add_bcast (addPublic),
     k_decompose_triv<u32> balanced and not, k_decompose_base2<u32>, k_rescale_drop0<u32>.
Two-power tunnels, evalLin, decrypt and the general-index engine on 4-byte extreme words: tests/test_gpu_word32_thresholds.py."""
import numpy as np
import pytest

from helpers import (assert_reduced, centred_extreme_words, extreme_words, oracle_full_mul, oracle_mul_relin_base2, primes_1_mod,
                     primes_below)
from test_gpu_full_mul import SIX_QS
from test_gpu_parity import EIGHT_QS

pytestmark = pytest.mark.gpu

M16 = 1 << 16                                                   # moduli = 1 mod 2^16 serve every n <= 2^15
TOP6 = primes_below(M16, 6, 1 << 31)
TOP5 = TOP6[:5]
ABOVE30 = primes_1_mod(M16, 2, 1 << 30)                         # the smallest ring with q30 == false
BELOW30 = primes_below(M16, 5, 1 << 30)
STRADDLE30 = [BELOW30[0], ABOVE30[0]]                           # one limb on each side of 2^30: not q30, balanced
_HALF31 = (TOP5[0] - 1) // 2
EDGE_BAL31 = [TOP5[0], primes_1_mod(M16, 1, _HALF31)[0]]        # the first prime above (qmax - 1) / 2: still balanced
EDGE_UNBAL31 = [TOP5[0], primes_below(M16, 1, _HALF31 + 1)[0]]  # the last one at or below it: not any more
_HALF30 = (BELOW30[0] - 1) // 2
EDGE_BAL30 = [BELOW30[0], primes_1_mod(M16, 1, _HALF30)[0]]     # q30 and balanced
EDGE_UNBAL30 = [BELOW30[0], primes_below(M16, 1, _HALF30 + 1)[0]]   # q30 and not
SMALL2 = primes_1_mod(M16, 2, 0)                                # the two smallest primes = 1 mod 2^16: 17 and 20 bits
MIXED = [TOP5[0]] + SMALL2                                      # the largest spread
MIXED_LAST = SMALL2 + [TOP5[0]]                                 # the same limbs in another drop order
MIXED_FULL = MIXED + TOP5[1:3]                                  # MIXED plus two more 31-bit limbs
EIGHT_TOP = EIGHT_QS                                            # = 1 mod 2^12
TOP17 = SIX_QS                                                  # = 1 mod 2^17: n = 2^16
BELOW30_17 = primes_below(1 << 17, 1, 1 << 30)[0]
EDGE31_FULL = {"bal": [TOP5[1]] + EDGE_BAL31, "unbal": [TOP5[1]] + EDGE_UNBAL31}        # one limb added in front of an EDGE pair
EDGE30_FULL = {"bal": [BELOW30[1]] + EDGE_BAL30, "unbal": [BELOW30[1]] + EDGE_UNBAL30}

RINGS = {"TOP5": TOP5, "TOP4": TOP5[:4], "TOP3": TOP5[:3], "TOP2": TOP5[:2], "TOP1": TOP5[:1], "ABOVE30": ABOVE30, "ABOVE1": ABOVE30[:1],
         "BELOW30": BELOW30, "BELOW4": BELOW30[:4], "BELOW3": BELOW30[:3], "BELOW2": BELOW30[:2], "BELOW1": BELOW30[:1],
         "STRADDLE30": STRADDLE30, "EDGE_BAL31": EDGE_BAL31, "EDGE_UNBAL31": EDGE_UNBAL31, "EDGE_BAL30": EDGE_BAL30,
         "EDGE_UNBAL30": EDGE_UNBAL30, "MIXED": MIXED, "MIXED_LAST": MIXED_LAST, "MIXED_FULL": MIXED_FULL, "EIGHT_TOP": EIGHT_TOP,
         "TOP17": TOP17, "TOP17_1": TOP17[:1], "BELOW30_17": [BELOW30_17], "TOP_AND_17_BIT": [TOP5[0], 65537],
         "EDGE31_FULL_BAL": EDGE31_FULL["bal"], "EDGE31_FULL_UNBAL": EDGE31_FULL["unbal"],
         "EDGE30_FULL_BAL": EDGE30_FULL["bal"], "EDGE30_FULL_UNBAL": EDGE30_FULL["unbal"]}

ALL_MODULI = sorted({q for qs in RINGS.values() for q in qs} | {TOP6[5]})


def is_balanced(qs):
    """r->balanced of ring_create_impl."""
    return (max(qs) - 1) // 2 < min(qs)


def is_q30(qs):
    """r->q30 of ring_create_impl (4-byte rings)."""
    return max(qs) < (1 << 30)


# name -> (balanced, q30): what ring_create_impl derives, and with it the instantiations `dispatch` picks
CLASSES = {"TOP5": (True, False), "ABOVE30": (True, False), "BELOW30": (True, True), "STRADDLE30": (True, False),
           "EDGE_BAL31": (True, False), "EDGE_UNBAL31": (False, False), "EDGE_BAL30": (True, True), "EDGE_UNBAL30": (False, True),
           "MIXED": (False, False), "MIXED_LAST": (False, False), "MIXED_FULL": (False, False), "EIGHT_TOP": (True, False),
           "TOP17": (True, False), "BELOW30_17": (True, True), "TOP_AND_17_BIT": (False, False),
           "EDGE31_FULL_BAL": (True, False), "EDGE31_FULL_UNBAL": (False, False), "EDGE30_FULL_BAL": (True, True),
           "EDGE30_FULL_UNBAL": (False, True)}


def test_the_moduli_are_where_the_cases_need_them():
    assert TOP6 == [2147352577, 2146959361, 2146041857, 2145976321, 2144796673, 2144468993]
    assert ABOVE30 == [1073872897, 1074266113]
    assert BELOW30 == [1073479681, 1072496641, 1071513601, 1070727169, 1069219841]
    assert STRADDLE30 == [1073479681, 1073872897]
    assert _HALF31 == 1073676288 and EDGE_BAL31 == [2147352577, 1073872897] and EDGE_UNBAL31 == [2147352577, 1073479681]
    assert _HALF30 == 536739840 and EDGE_BAL30 == [1073479681, 537133057] and EDGE_UNBAL30 == [1073479681, 536608769]
    assert MIXED == [2147352577, 65537, 786433] and MIXED_LAST == [65537, 786433, 2147352577]
    assert EIGHT_TOP == primes_below(1 << 12, 8, 1 << 31) and TOP17 == primes_below(1 << 17, 6, 1 << 31)
    assert BELOW30_17 == 1073479681 and TOP17[0] == TOP5[0]
    assert all(q < (1 << 31) for q in ALL_MODULI)                 # 4-byte words throughout
    assert all((1 << 31) - (1 << 22) < q for q in TOP6 + EIGHT_TOP) and all((1 << 31) - (1 << 24) < q for q in TOP17)
    assert all((1 << 30) < q < (1 << 30) + (1 << 20) for q in ABOVE30)
    assert all((1 << 30) - (1 << 23) < q < (1 << 30) for q in BELOW30)
    for name, (bal, q30) in CLASSES.items():
        assert is_balanced(RINGS[name]) == bal and is_q30(RINGS[name]) == q30, name
    # the EDGE partners sit next to the boundary, and next to each other
    for bal, unbal, half in ((EDGE_BAL31, EDGE_UNBAL31, _HALF31), (EDGE_BAL30, EDGE_UNBAL30, _HALF30)):
        assert unbal[1] <= half < bal[1] and bal[1] - unbal[1] < 1 << 20
    # DropTab::balanced of the 2-3-1 shapes of case group 6: only the drop of qmax above its EDGE partner decides
    for full, edge in ((EDGE31_FULL, EDGE_UNBAL31), (EDGE30_FULL, EDGE_UNBAL30)):
        for qs in full.values():
            assert (qs[0] - 1) // 2 < min(qs[1:])
        assert (full["bal"][1] - 1) // 2 < full["bal"][2] and not (full["unbal"][1] - 1) // 2 < full["unbal"][2]


def _ring(oracle_lib, n, qs):
    import alchemy_amd as A
    g = A.Ring(2 * n, qs)                                        # a refusal raises: the test fails
    assert g.word_bytes == 4
    return g, oracle_lib.Ring(n, qs)


def _rings_full(n, qs_h, l_in, l_out, opts=None):
    import alchemy_amd as A
    L = len(qs_h)
    rings = A.Ring(2 * n, qs_h[L - l_in:]), A.Ring(2 * n, qs_h), A.Ring(2 * n, qs_h[L - l_out:])
    for r in rings:
        assert r.word_bytes == 4
        for k, v in (opts or {}).items():
            r.set_option(k, v)
    return rings


def _minus_one(qs):
    return [q - 1 for q in qs]


def constant_elements(n, qs):
    """(2, n, L): every word q-1, and q-1 in the lower half with 0 above -- every first-stage butterfly sees q-1 on both inputs."""
    qv = np.array(qs, dtype=np.int64)
    out = np.zeros((2, n, len(qs)), dtype=np.int64)
    out[0, :, :] = qv - 1
    out[1, :n // 2, :] = qv - 1
    return out


def lifts_beyond(x, qs):
    """How many centred lifts of the (..., L) residues x reach or pass another limb's modulus: |z| >= q_j is where the BALANCED = true
    reduce (one add) and the general one part."""
    x = np.asarray(x)
    count = 0
    for i, q in enumerate(qs):
        z = np.where(2 * x[..., i] < q, x[..., i], q - x[..., i])              # |centred lift|
        count += int(np.count_nonzero(z >= min(qs[:i] + qs[i + 1:]))) if len(qs) > 1 else 0
    return count


# ---- 1. transforms -------------------------------------------------------------------------------------------------------------------
CRT_CASES = ([(logn, name, half) for logn in range(4, 16) for name in ("TOP1", "ABOVE1", "BELOW1", "MIXED")
              for half in ((0, 1) if logn == 15 else (None,)) if name != "MIXED" or logn <= 11]
             + [(16, "TOP17_1", None), (16, "BELOW30_17", None)])


@pytest.mark.parametrize("logn,name,half", CRT_CASES, ids=[f"logn{c[0]}-{c[1]}" + ("" if c[2] is None else f"-half{c[2]}") for c in CRT_CASES])
def test_crt_crtinv_and_products(oracle_lib, logn, name, half):
    """k_crt<LOGN, u32>, k_crt_half<15, u32> (option crt_half), k_crt_split (n = 2^16), forward and inverse: crt in place, crtInv of it,
    crtInv on CRT-basis input, the products of two transforms -- on two extreme elements and the two constant ones."""
    n, qs = 1 << logn, RINGS[name]
    g, o = _ring(oracle_lib, n, qs)
    if half is not None:
        g.set_option("crt_half", half)
    rng = np.random.default_rng(3200 + logn)
    x = np.concatenate([extreme_words(rng, 2, n, qs), constant_elements(n, qs)])
    want = [o.crt(e) for e in x]
    buf = g.upload(x)
    buf.crt()
    got = buf.download()
    assert_reduced(got, qs)
    for e in range(4):
        assert np.array_equal(got[e], want[e]), f"crt mismatch elem {e}"
    prod = g.alloc(2)
    prod.mul(buf.view(0, 2), buf.view(2, 2), 2)                  # extreme * constant, twice
    wprod = [o.mul(want[0], want[2]), o.mul(want[1], want[3])]
    got = prod.download()
    assert_reduced(got, qs)
    for e in range(2):
        assert np.array_equal(got[e], wprod[e]), f"product of two transforms {e}"
    buf.crtinv()
    assert np.array_equal(buf.download(), x), "crtInv . crt != id"
    prod.crtinv()
    got = prod.download()
    assert_reduced(got, qs)
    for e in range(2):
        assert np.array_equal(got[e], o.crtinv(wprod[e])), f"crtInv of the product {e}"
    b2 = g.upload(x)                                             # the same words AS CRT-basis input
    b2.crtinv()
    got = b2.download()
    assert_reduced(got, qs)
    for e in range(4):
        assert np.array_equal(got[e], o.crtinv(x[e])), f"crtInv mismatch elem {e}"


# ---- 2. keySwitchQuadCirc hint (a * b) off the two-workgroup sizes ------------------------------------------------------------------------
def _relin_case(oracle_lib, n, qs, batch, seed, minus_one, pow_basis=False, options=({},)):
    from alchemy_amd import capi
    g, o = _ring(oracle_lib, n, qs)
    L = len(qs)
    rng = np.random.default_rng(seed)
    hint = extreme_words(rng, 2 * L, n, qs)
    a, b = extreme_words(rng, 2 * batch, n, qs), extreme_words(rng, 2 * batch, n, qs)
    s_pre = _minus_one(qs) if minus_one else None
    want = [o.ct_mul_relin(list(hint), a[2 * ct], a[2 * ct + 1], b[2 * ct], b[2 * ct + 1], s_pre=s_pre, pow_basis=pow_basis)
            for ct in range(batch)]
    ghint, ga, gb = g.hint_load(hint), g.upload(a), g.upload(b)
    for opts in options:
        for k, v in opts.items():
            g.set_option(k, v)
        gout = g.alloc(2 * batch)
        g.ct_mul_relin(ghint, ga, gb, gout, batch, s_pre=s_pre, flags=(capi.ALCH_POW_IN | capi.ALCH_POW_OUT) if pow_basis else 0)
        got = gout.download()
        assert_reduced(got, qs)
        for ct in range(batch):
            assert np.array_equal(got[2 * ct], want[ct][0]), f"c0 mismatch ct {ct} {opts}"
            assert np.array_equal(got[2 * ct + 1], want[ct][1]), f"c1 mismatch ct {ct} {opts}"


RELIN_RINGS = ["TOP4", "ABOVE30", "BELOW4", "MIXED", "MIXED_LAST", "EDGE_BAL31", "EDGE_UNBAL31"]
RELIN_SIZES = [(4, 3), (8, 3), (8, 9), (10, 3), (13, 2), (14, 2)]


@pytest.mark.parametrize("minus_one", [False, True], ids=["s_default", "s_minus_one"])
@pytest.mark.parametrize("name", RELIN_RINGS)
@pytest.mark.parametrize("logn,batch", RELIN_SIZES)
def test_ct_mul_relin_off_the_half_sizes(oracle_lib, logn, batch, name, minus_one):
    """k_tensor_intt<LOGN, u32> and k_ks_accum<LOGN, u32, true / false>: extreme hint rows and operands; batch 9 is ragged against the
    group of eight ciphertexts."""
    _relin_case(oracle_lib, 1 << logn, RINGS[name], batch, 3300 + 16 * logn + batch + minus_one, minus_one)


@pytest.mark.parametrize("minus_one", [False, True], ids=["s_default", "s_minus_one"])
def test_ct_mul_relin_eight_31_bit_limbs(oracle_lib, minus_one):
    _relin_case(oracle_lib, 1 << 8, EIGHT_TOP, 2, 3400 + minus_one, minus_one)


@pytest.mark.parametrize("minus_one", [False, True], ids=["s_default", "s_minus_one"])
def test_ct_mul_relin_pow_basis(oracle_lib, minus_one):
    _relin_case(oracle_lib, 1 << 8, TOP5[:4], 3, 3420 + minus_one, minus_one, pow_basis=True)


def test_ct_mul_relin_n65536(oracle_lib):
    """n = 2^16: k_tensor_crtinv_split + k_ks_accum_split<FROM_OPS> (the default), then the composed forms -- k_tensor_ew, k_crt_split
    and k_ks_accum_split (split_fused = 1), k_crt_split_digits and the hint products on their own (split_fused = 0)."""
    _relin_case(oracle_lib, 1 << 16, TOP17[:3], 2, 3430, minus_one=True, options=({}, {"split_fused": 1}, {"split_fused": 0}))


WORST_RINGS = {"TOP4": TOP5[:4], "ABOVE30": ABOVE30, "BELOW4": BELOW30[:4], "EIGHT_TOP": EIGHT_TOP, "TOP17_3": TOP17[:3]}
WORST_CASES = ([(logn, name) for logn in (4, 8, 10, 11, 13, 14, 15) for name in ("TOP4", "ABOVE30", "BELOW4")]
               + [(8, "EIGHT_TOP"), (11, "EIGHT_TOP"), (16, "TOP17_3")])


@pytest.mark.parametrize("minus_one", [False, True], ids=["s_default", "s_minus_one"])
@pytest.mark.parametrize("logn,name", WORST_CASES, ids=[f"logn{c[0]}-{c[1]}" for c in WORST_CASES])
def test_ct_mul_relin_every_product_at_its_maximum(oracle_lib, logn, name, minus_one):
    """The largest sum a key-switch accumulator can see: every hint word is q-1 and c2 is the constant -1 (a1 = crt(1), b1 = crt(-1),
    or crt(1) under s_pre = -1), so every digit is -1, its CRT image is q-1 in every slot, and every slot sums L products (q-1)^2 --
    on top of a0 b0 = (q-1)^2 in the first ciphertext and extreme words in the second.  Random extreme words reach this in no
    slot; k_ks_accum, every k_ks_accum_half form without added limbs and k_ks_accum_split all run it here."""
    n, qs, batch = 1 << logn, WORST_RINGS[name], 2
    g, o = _ring(oracle_lib, n, qs)
    L = len(qs)
    qv = np.array(qs, dtype=np.int64)
    top = np.ascontiguousarray(np.broadcast_to(qv - 1, (n, L)))
    ones = np.ones((n, L), dtype=np.int64)
    rng = np.random.default_rng(3450 + logn + minus_one)
    hint = np.stack([top] * (2 * L))
    a, b = extreme_words(rng, 2 * batch, n, qs), extreme_words(rng, 2 * batch, n, qs)
    a[0], b[0] = top, top
    a[1::2], b[1::2] = ones, (ones if minus_one else top)
    s_pre = _minus_one(qs) if minus_one else None
    for d in o.decompose_triv(o.crtinv(o.scale(o.mul(a[1], b[1]), s_pre if s_pre else [1] * L))):
        assert np.array_equal(o.crt(d), top), "a digit's CRT image is not q-1 everywhere"
    gout = g.alloc(2 * batch)
    g.ct_mul_relin(g.hint_load(hint), g.upload(a), g.upload(b), gout, batch, s_pre=s_pre)
    got = gout.download()
    assert_reduced(got, qs)
    for ct in range(batch):
        w0, w1 = o.ct_mul_relin(list(hint), a[2 * ct], a[2 * ct + 1], b[2 * ct], b[2 * ct + 1], s_pre=s_pre)
        assert np.array_equal(got[2 * ct], w0), f"c0 mismatch ct {ct}"
        assert np.array_equal(got[2 * ct + 1], w1), f"c1 mismatch ct {ct}"


# ---- 3. n = 2^11 and 2^15 on the rings around 2^30 and the balanced / unbalanced boundary -------------------------------------------------
def _digit_operands(rng, orc, batch, n, qs):
    """a = (a0, crt(1)), b = (b0, crt(x)): the quadratic coefficient is s x, so the TrivGad digits are the centred lifts of +-x, x per
    coefficient from {0, 1, q-1, (q-1)/2, (q+1)/2, (q-3)/2} (the construction of tests/test_gpu_ks_signed_stage01.py)."""
    one = np.zeros((n, len(qs)), dtype=np.int64)
    one[0, :] = 1
    one_crt = orc.crt(one)
    assert np.all(one_crt == 1)
    a, b = extreme_words(rng, 2 * batch, n, qs), extreme_words(rng, 2 * batch, n, qs)
    x = centred_extreme_words(rng, batch, n, qs)
    for ct in range(batch):
        a[2 * ct + 1] = one_crt
        b[2 * ct + 1] = orc.crt(x[ct])
    return a, b, x


def digits_at_the_ends_case(oracle_lib, n, qs, batch, seed, minus_one):
    """Operands, hint and the oracle's result of case group 3, with the construction confirmed on the oracle: (hint, a, b, s_pre, want)."""
    o = oracle_lib.Ring(n, qs)
    L = len(qs)
    rng = np.random.default_rng(seed)
    hint = extreme_words(rng, 2 * L, n, qs)
    a, b, x = _digit_operands(rng, o, batch, n, qs)
    s_pre = _minus_one(qs) if minus_one else None
    for ct in range(batch):
        c2 = o.crtinv(o.scale(o.mul(a[2 * ct + 1], b[2 * ct + 1]), s_pre if s_pre else [1] * L))
        signed = np.stack([(q - x[ct][:, j]) % q for j, q in enumerate(qs)], axis=1) if minus_one else x[ct]
        assert np.array_equal(c2, signed), f"ct {ct}: the digits are not the centred lifts of +-x"
    # the digits tell BALANCED = true from false exactly where the ring is unbalanced
    assert (lifts_beyond(x, qs) > 0) == (not is_balanced(qs))
    want = [o.ct_mul_relin(list(hint), a[2 * ct], a[2 * ct + 1], b[2 * ct], b[2 * ct + 1], s_pre=s_pre) for ct in range(batch)]
    return hint, a, b, s_pre, want


ENDS_RINGS = ["ABOVE30", "STRADDLE30", "EDGE_BAL31", "EDGE_UNBAL31", "EDGE_BAL30", "EDGE_UNBAL30"]


@pytest.mark.parametrize("minus_one", [False, True], ids=["s_default", "s_minus_one"])
@pytest.mark.parametrize("name", ENDS_RINGS)
@pytest.mark.parametrize("logn,batch", [(11, 2), (11, 9), (15, 2)])
def test_ct_mul_relin_digits_at_the_ends(oracle_lib, logn, batch, name, minus_one):
    """The digits k_ks_accum_half reads are the centred lifts of +-x, at both ends of the centred range of every limb.  On the EDGE
    rings only the digits at +-(qmax - 1) / 2 tell the BALANCED instantiations apart: |z| >= qmin happens nowhere else (the partners
    lie within 2^20 of (qmax - 1) / 2), and products of uniform or extreme operands never land there.  At n = 2^15:
      ABOVE30, STRADDLE30, EDGE_BAL31   k_tensor_intt_split<15, false> into k_ks_accum_half<15, true>
      EDGE_UNBAL31                      k_tensor_intt_split<15, false> into k_ks_accum_half<15, false>
      EDGE_BAL30                        k_tensor_intt_split<15, true> into k_ks_accum_half<15, true, 32, false, true>
      EDGE_UNBAL30                      k_tensor_intt_split<15, true> into k_ks_accum_half<15, false> -- Harvey's tensor kernel in
                                        front of the plain key switch, the pairing OP_KS_ACCUM's `c.q30 && c.balanced` makes
    and with option q30 = 0 the last two run k_tensor_intt_split<15, false>; both settings must give the same words.  At n = 2^11 the
    tensor kernel is k_tensor_intt<11, u32> and the key switch the same instantiations with LOGN = 11; batch 9 there is ragged
    against the group of eight ciphertexts."""
    n, qs = 1 << logn, RINGS[name]
    hint, a, b, s_pre, want = digits_at_the_ends_case(oracle_lib, n, qs, batch, 3500 + 4 * logn + batch + minus_one, minus_one)
    results = []
    for q30 in ((1, 0) if is_q30(qs) else (1,)):
        g, _ = _ring(oracle_lib, n, qs)
        g.set_option("q30", q30)
        gout = g.alloc(2 * batch)
        g.ct_mul_relin(g.hint_load(hint), g.upload(a), g.upload(b), gout, batch, s_pre=s_pre)
        got = gout.download()
        assert_reduced(got, qs)
        for ct in range(batch):
            assert np.array_equal(got[2 * ct], want[ct][0]), f"c0 mismatch ct {ct} q30={q30}"
            assert np.array_equal(got[2 * ct + 1], want[ct][1]), f"c1 mismatch ct {ct} q30={q30}"
        results.append(got)
    if len(results) == 2:
        assert np.array_equal(results[0], results[1]), "option q30 changes the result"


# ---- 4. BaseBGad 2 hints ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("minus_one", [False, True], ids=["s_default", "s_minus_one"])
@pytest.mark.parametrize("name,digits", [("TOP2", (31, 31)), ("TOP_AND_17_BIT", (31, 17)), ("BELOW2", (30, 30))])
@pytest.mark.parametrize("logn", [8, 11])
def test_ct_mul_relin_base2_hint(oracle_lib, logn, name, digits, minus_one):
    """k_crt_base2_digits<u32>: 31 digits on a 31-bit limb, shift counts up to 30.  c2 = +-x with x from {0, 1, q-1, (q-1)/2,
    (q+1)/2, (q-3)/2}: +-(q-1)/2 sets every digit position and the absorbing top digit, with either sign."""
    from alchemy_amd import capi
    from oracle import model
    n, batch, qs = 1 << logn, 2, RINGS[name]
    g, o = _ring(oracle_lib, n, qs)
    D = g.gadget_digits(capi.ALCH_GAD_BASE2)
    assert tuple(model.baseb_digits(q) for q in qs) == digits and D == sum(digits)
    rng = np.random.default_rng(3600 + logn + D + minus_one)
    hint = extreme_words(rng, 2 * D, n, qs)
    a, b, x = _digit_operands(rng, o, batch, n, qs)
    s_pre = _minus_one(qs) if minus_one else None
    gout = g.alloc(2 * batch)
    g.ct_mul_relin(g.hint_load(hint, gadget=capi.ALCH_GAD_BASE2), g.upload(a), g.upload(b), gout, batch, s_pre=s_pre)
    got = gout.download()
    assert_reduced(got, qs)
    for ct in range(batch):
        w0, w1 = oracle_mul_relin_base2(oracle_lib, n, qs, list(hint), a[2 * ct], a[2 * ct + 1], b[2 * ct], b[2 * ct + 1], s_pre=s_pre)
        assert np.array_equal(got[2 * ct], w0), f"c0 mismatch ct {ct}"
        assert np.array_equal(got[2 * ct + 1], w1), f"c1 mismatch ct {ct}"


# ---- 5. PT2CT's whole mul_ ---------------------------------------------------------------------------------------------------------------
# (id, moduli of the hint's ring, L_in, L_out, Pow-basis output)
FULL_CASES = [
    ("4-5-3", TOP5, 4, 3, False),                 # key switch with dup = 1, k_rescale_out_lin<u32, 2, true>
    ("3-4-2", TOP5[:4], 3, 2, False),
    ("2-3-1", TOP5[:3], 2, 1, False),
    ("3-4-3", TOP5[:4], 3, 3, False),             # one limb dropped, balanced: k_rescale_out_lin<u32, 1, true>
    ("4-5-3-pow", TOP5, 4, 3, True),              # Pow-basis output: k_rescale_out<u32>
    ("2-5-2", TOP5, 2, 2, False),                 # dup = 3 and a three-limb drop: k_rescale_out<u32>; n = 2^15: the half-size rescale kernels
    ("below30-4-5-3", BELOW30, 4, 3, False),      # Q30 with an added limb: k_ks_accum_half<LOGN, true, 32, true, true> at n = 2^11 / 2^15
    ("mixed-4-5-3", MIXED_FULL, 4, 3, False),     # drops the 31-bit and the 17-bit limb: an unbalanced two-limb drop, k_rescale_out<u32> / half-size
    ("mixed-4-5-4", MIXED_FULL, 4, 4, False),     # drops the 31-bit limb above a 17-bit one: k_rescale_out_lin<u32, 1, false>
]


def _full_case(oracle_lib, n, qs_h, l_in, l_out, pow_out, batch, seed, minus_one, option_sets=({},)):
    from alchemy_amd import capi
    L = len(qs_h)
    qs_in, qs_out = qs_h[L - l_in:], qs_h[L - l_out:]
    rng = np.random.default_rng(seed)
    hint = extreme_words(rng, 2 * L, n, qs_h)
    a, b = extreme_words(rng, 2 * batch, n, qs_in), extreme_words(rng, 2 * batch, n, qs_in)
    s_pre = _minus_one(qs_in) if minus_one else None
    want = [oracle_full_mul(oracle_lib, n, qs_h, l_in, l_out, list(hint), a[2 * ct], a[2 * ct + 1], b[2 * ct], b[2 * ct + 1],
                            s_pre=s_pre, pow_out=pow_out) for ct in range(batch)]
    for opts in option_sets:
        rin, rh, rout = _rings_full(n, qs_h, l_in, l_out, opts)
        gout = rout.alloc(2 * batch)
        capi.ct_mul_full(rh.hint_load(hint), rin.upload(a), rin.upload(b), gout, batch, s_pre=s_pre, flags=capi.ALCH_POW_OUT if pow_out else 0)
        got = gout.download()
        assert_reduced(got, qs_out)
        for ct in range(batch):
            assert np.array_equal(got[2 * ct], want[ct][0]), f"c0 mismatch ct {ct} {opts}"
            assert np.array_equal(got[2 * ct + 1], want[ct][1]), f"c1 mismatch ct {ct} {opts}"


@pytest.mark.parametrize("minus_one", [False, True], ids=["s_default", "s_minus_one"])
@pytest.mark.parametrize("case", FULL_CASES, ids=[c[0] for c in FULL_CASES])
@pytest.mark.parametrize("logn,batch", [(8, 3), (11, 3), (11, 9), (15, 2)])
def test_ct_mul_full(oracle_lib, logn, batch, case, minus_one):
    """FULL_CASES on extreme words; batch 9 at n = 2^11 is ragged against the key switch's group of eight ciphertexts."""
    _, qs_h, l_in, l_out, pow_out = case
    _full_case(oracle_lib, 1 << logn, qs_h, l_in, l_out, pow_out, batch, 3700 + logn + batch + 2 * len(qs_h) + l_in + minus_one, minus_one)


@pytest.mark.parametrize("minus_one", [False, True], ids=["s_default", "s_minus_one"])
def test_ct_mul_full_n32768_options(oracle_lib, minus_one):
    """4 -> 5 -> 3 at n = 2^15 with rs_half = 1 (k_rescale_drop_half + k_rescale_keep_half where k_rescale_out_lin<15, u32, 2, true>
    would serve) and with rs_lin = 0 (every limb through the Pow basis: k_rescale_out<15, u32>)."""
    _full_case(oracle_lib, 1 << 15, TOP5, 4, 3, False, 2, 3790 + minus_one, minus_one, option_sets=({"rs_half": 1}, {"rs_lin": 0}))


# ---- 6. the rescale at the ends of the centred range -----------------------------------------------------------------------------------------
# (id, moduli of the hint's ring, L_in, L_out)
RESCALE_END_CASES = [
    ("top-4-5-3", TOP5, 4, 3),
    ("edge_bal31-2-3-1", EDGE31_FULL["bal"], 2, 1),       # qmax dropped above the first prime over (qmax - 1) / 2
    ("edge_unbal31-2-3-1", EDGE31_FULL["unbal"], 2, 1),   # ... and above the last one at or under it: DropTab::balanced = 0
    ("edge_bal31-2-3-2", EDGE31_FULL["bal"], 2, 2),       # only the added limb is dropped: k_rescale_out_lin<u32, 1, true> on zeros
    ("edge_unbal31-2-3-2", EDGE31_FULL["unbal"], 2, 2),
    ("edge_bal30-2-3-1", EDGE30_FULL["bal"], 2, 1),       # the same below 2^30: Harvey's key switch in front
    ("edge_unbal30-2-3-1", EDGE30_FULL["unbal"], 2, 1),
    ("edge_bal30-2-3-2", EDGE30_FULL["bal"], 2, 2),
    ("edge_unbal30-2-3-2", EDGE30_FULL["unbal"], 2, 2),
    ("mixed-4-5-3", MIXED_FULL, 4, 3),
]


def rescale_at_the_ends_case(oracle_lib, n, qs_h, l_in, l_out, batch, seed, minus_one):
    """Operands and the oracle's results of case group 6, with the construction confirmed on the oracle: (hint, a, b, s_pre,
    {pow_out: want}).  Zero hint, a = (crt(1), 0) (a1 = crt(1) from the third ciphertext on), b = (crt(q_a x), crt(q_a y)), s_pre =
    +-q_a^-1 for the added modulus q_a: the key switch hands on (0 | +-q_a x) and (0 | +-q_a y), so once the added limb (zeros) is
    dropped the next limb holds +-x, +-y themselves."""
    L = len(qs_h)
    assert L - l_in == 1
    qs_in = qs_h[1:]
    qa = qs_h[0]
    o_in, o_h = oracle_lib.Ring(n, qs_in), oracle_lib.Ring(n, qs_h)
    rng = np.random.default_rng(seed)
    one = np.zeros((n, l_in), dtype=np.int64)
    one[0, :] = 1
    one_crt = o_in.crt(one)
    x = centred_extreme_words(rng, 2 * batch, n, qs_in)
    up = [qa % q for q in qs_in]
    a = np.zeros((2 * batch, n, l_in), dtype=np.int64)
    a[0::2] = one_crt
    a[5::2] = one_crt
    b = np.stack([o_in.crt(o_in.scale(e, up)) for e in x])
    hint = np.zeros((2 * L, n, L), dtype=np.int64)
    s_pre = [pow(qa, -1, q) for q in qs_in]
    if minus_one:
        s_pre = [q - v for v, q in zip(s_pre, qs_in)]
    sign = _minus_one(qs_in) if minus_one else [1] * l_in
    zeros = np.zeros((n, 1), dtype=np.int64)
    for ct in range(batch):
        # the key switch's output in the Pow basis: oracle_full_mul with nothing dropped
        k0, k1 = oracle_full_mul(oracle_lib, n, qs_h, l_in, L, list(hint), a[2 * ct], a[2 * ct + 1], b[2 * ct], b[2 * ct + 1],
                                 s_pre=s_pre, pow_out=True)
        sx = o_in.scale(x[2 * ct], sign)
        sy = o_in.scale(o_in.add(x[2 * ct + 1], x[2 * ct]) if ct >= 2 else x[2 * ct + 1], sign)
        for got, e in ((k0, sx), (k1, sy)):
            assert np.array_equal(got, np.concatenate([zeros, o_in.scale(e, up)], axis=1)), "the key switch does not hand on +-q_a x"
            assert np.array_equal(o_h.rescale_drop0(got), e), "the next limb does not hold +-x"
    # two limbs dropped: the second one's lifts are those of +-x on qs_in[0]; they reach past a kept modulus exactly where that
    # step of the drop is unbalanced -- what tells DropTab::balanced = 1 from 0 on the EDGE rings
    if L - l_out == 2:
        first = x[0::2, :, :1]
        assert (lifts_beyond(np.concatenate([first, np.zeros_like(first)], axis=2), [qs_in[0], min(qs_in[1:])]) > 0) \
            == ((qs_in[0] - 1) // 2 >= min(qs_in[1:]))
    want = {pow_out: [oracle_full_mul(oracle_lib, n, qs_h, l_in, l_out, list(hint), a[2 * ct], a[2 * ct + 1], b[2 * ct], b[2 * ct + 1],
                                      s_pre=s_pre, pow_out=pow_out) for ct in range(batch)] for pow_out in (False, True)}
    return hint, a, b, s_pre, want


@pytest.mark.parametrize("minus_one", [False, True], ids=["plus_x", "minus_x"])
@pytest.mark.parametrize("case", RESCALE_END_CASES, ids=[c[0] for c in RESCALE_END_CASES])
@pytest.mark.parametrize("logn", [8, 15])
def test_ct_mul_full_rescale_at_the_ends(oracle_lib, logn, case, minus_one):
    """The closing modSwitch on centred lifts at both ends of their range (rescale_at_the_ends_case): the added limb holds zeros and
    the next dropped limb holds +-x, +-y with x, y per coefficient from {0, 1, q-1, (q-1)/2, (q+1)/2, (q-3)/2} -- lifts that products
    of random words never reach, and the only ones that tell a balanced drop table from an unbalanced one on the EDGE rings.  The
    expressions (W)(v - r + q), c + (q - reduce_lifted(z)) and red(rr) of kernel_rescale_out.hpp / kernel_rescale_half.hpp are exact
    only while these lifts stay in their range."""
    from alchemy_amd import capi
    _, qs_h, l_in, l_out = case
    n, batch, L = 1 << logn, 2 if logn == 15 else 3, len(qs_h)
    hint, a, b, s_pre, want = rescale_at_the_ends_case(oracle_lib, n, qs_h, l_in, l_out, batch, 3750 + logn + L + l_out + minus_one, minus_one)
    rin, rh, rout = _rings_full(n, qs_h, l_in, l_out)
    gout = rout.alloc(2 * batch)
    for pow_out in (False, True):
        capi.ct_mul_full(rh.hint_load(hint), rin.upload(a), rin.upload(b), gout, batch, s_pre=s_pre, flags=capi.ALCH_POW_OUT if pow_out else 0)
        got = gout.download()
        assert_reduced(got, qs_h[L - l_out:])
        for ct in range(batch):
            assert np.array_equal(got[2 * ct], want[pow_out][ct][0]), f"c0 mismatch ct {ct} pow_out={pow_out}"
            assert np.array_equal(got[2 * ct + 1], want[pow_out][ct][1]), f"c1 mismatch ct {ct} pow_out={pow_out}"


# ---- 7. mul_ one step at a time -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn", [8, 11])
def test_mul_steps_chain(oracle_lib, logn):
    """alch_ct_mul, alch_ct_mod_switch_deg (up, degree 2), alch_ct_key_switch_quad, alch_ct_mod_switch_deg (down): every step against
    the oracle, 4 -> 5 -> 3 limbs on the five largest primes below 2^31, and the chain's result against alch_ct_mul_full."""
    from alchemy_amd import capi, mulsteps as MS
    n, batch, qs_h, l_in, l_out = 1 << logn, 3, TOP5, 4, 3
    L = len(qs_h)
    qs_in, qs_out = qs_h[L - l_in:], qs_h[L - l_out:]
    rin, rh, rout = _rings_full(n, qs_h, l_in, l_out)
    o_in, o_h, o_out = oracle_lib.Ring(n, qs_in), oracle_lib.Ring(n, qs_h), oracle_lib.Ring(n, qs_out)
    rng = np.random.default_rng(3800 + logn)
    hint = extreme_words(rng, 2 * L, n, qs_h)
    a, b = extreme_words(rng, 2 * batch, n, qs_in), extreme_words(rng, 2 * batch, n, qs_in)
    s_pre = _minus_one(qs_in)
    ghint, ga, gb = rh.hint_load(hint), rin.upload(a), rin.upload(b)
    quad = MS.ct_mul(ga, gb, batch, s_pre=s_pre)
    sw = MS.mod_switch(quad, rh, batch, degree=2)
    lin = MS.key_switch_quad(ghint, sw, batch)
    res = MS.mod_switch(lin, rout, batch, degree=1)
    gq, gs, gl, gr = quad.download(0, 3 * batch), sw.download(0, 3 * batch), lin.download(0, 2 * batch), res.download(0, 2 * batch)
    for got, qs in ((gq, qs_in), (gs, qs_h), (gl, qs_h), (gr, qs_out)):
        assert_reduced(got, qs)
    up = [qs_h[0] % q for q in qs_in]
    for ct in range(batch):
        a0, a1, b0, b1 = a[2 * ct], a[2 * ct + 1], b[2 * ct], b[2 * ct + 1]
        c = [o_in.mul(a0, b0), o_in.add(o_in.mul(a0, b1), o_in.mul(a1, b0)), o_in.mul(a1, b1)]
        c = [o_in.scale(x, s_pre) for x in c]
        for k in range(3):
            assert np.array_equal(gq[3 * ct + k], c[k]), ("alch_ct_mul", ct, k)
        c = [np.ascontiguousarray(np.concatenate([np.zeros((n, 1), dtype=np.int64), o_in.scale(x, up)], axis=1)) for x in c]
        for k in range(3):
            assert np.array_equal(gs[3 * ct + k], c[k]), ("alch_ct_mod_switch_deg up", ct, k)
        ks = [c[0], c[1]]
        for i, d in enumerate(o_h.decompose_triv(o_h.crtinv(c[2]))):
            dc = o_h.crt(d)
            ks = [o_h.add(ks[k], o_h.mul(dc, hint[2 * i + k])) for k in range(2)]
        for k in range(2):
            assert np.array_equal(gl[2 * ct + k], ks[k]), ("alch_ct_key_switch_quad", ct, k)
        for k in range(2):
            cur = o_h.crtinv(ks[k])
            for drop in range(L - l_out):
                cur = oracle_lib.Ring(n, qs_h[drop:]).rescale_drop0(cur)
            assert np.array_equal(gr[2 * ct + k], o_out.crt(cur)), ("alch_ct_mod_switch_deg down", ct, k)
    full = rout.alloc(2 * batch)
    capi.ct_mul_full(ghint, ga, gb, full, batch, s_pre=s_pre)
    assert np.array_equal(full.download(), gr)


# ---- 8. element-wise ops, gadget decompositions, rescale ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["TOP3", "MIXED", "EDGE_UNBAL31", "BELOW3"])
def test_elementwise_decompose_and_rescale(oracle_lib, name):
    """k_decompose_triv<u32> balanced and not, k_decompose_base2<u32>, alch_buf_rescale_drop0 (k_rescale_drop0<u32>), scale, add, sub,
    mulPublic, addPublic at n = 64."""
    import alchemy_amd as A
    n, qs = 64, RINGS[name]
    g, o = _ring(oracle_lib, n, qs)
    L = len(qs)
    rng = np.random.default_rng(3900 + L + len(name))
    x = extreme_words(rng, 6, n, qs)
    x[5] = centred_extreme_words(rng, 1, n, qs)[0]               # lifts at +-(q-1)/2 for the digits and the rescale
    gx = g.upload(x)

    def same(buf, want, qq=qs):
        got = buf.download()
        assert_reduced(got, qq)
        assert np.array_equal(got, np.stack(want))

    dst = g.alloc(6)
    dst.add(gx, g.upload(x[::-1]), 6)
    same(dst, [o.add(x[e], x[5 - e]) for e in range(6)])
    dst.sub(gx, g.upload(x[::-1]), 6)
    same(dst, [o.sub(x[e], x[5 - e]) for e in range(6)])
    dst.mul(gx, g.upload(x[::-1]), 6)
    same(dst, [o.mul(x[e], x[5 - e]) for e in range(6)])
    for s in (_minus_one(qs), [(q + 1) // 2 for q in qs], [q - 2 for q in qs]):
        dst.scale(gx, 6, s)
        same(dst, [o.scale(e, s) for e in x])
    dst.mul_public(gx, gx, 5, 6)
    same(dst, [o.mul(e, x[5]) for e in x])
    cts = g.upload(x[:4])
    cts.add_public(gx, 4, 2)
    same(cts, [o.add(x[0], x[4]), x[1], o.add(x[2], x[4]), x[3]])
    # TrivGad digits: host-buffer and device-resident form
    for e in (0, 5):
        want = o.decompose_triv(x[e])
        got = g.decompose_triv(x[e])
        assert len(got) == L
        for i in range(L):
            assert_reduced(got[i], qs)
            assert np.array_equal(got[i], want[i]), ("decompose_triv", e, i)
        dig = g.alloc(L + 1)
        gx.decompose_triv_into(e, dig, 1)
        same(dig.view(1, L), want)
    for e in (0, 5):
        want = o.decompose_base2(x[e])
        got = g.decompose_base2(x[e])
        assert len(got) == len(want) == sum((q - 1).bit_length() for q in qs)
        for i in range(len(want)):
            assert_reduced(got[i], qs)
            assert np.array_equal(got[i], want[i]), ("decompose_base2", e, i)
    # Rescale (a, b) -> b, limb 0 dropped
    gsmall = A.Ring(2 * n, qs[1:])
    assert gsmall.word_bytes == 4
    out = gsmall.alloc(6)
    gx.rescale_drop0_into(out, 6)
    same(out, [o.rescale_drop0(e) for e in x], qs[1:])
