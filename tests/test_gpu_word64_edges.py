"""GPU: the 64-bit word path at both ends of its modulus range.

A ring runs on 8-byte words as soon as one modulus is >= 2^31, and the library accepts every prime below 2^62.  The rest of the suite
runs that word size between 2^58 and 2^60 on uniform words; here it runs
  * on the largest primes below 2^62 (4q within 2^-45 of the word: Harvey's [0,4q) butterflies, the 128-bit Montgomery product and
    the Shoup quotient have no headroom left), on the first primes above 2^31 (the smallest that take the 8-byte kernels),
  * with a 62-bit limb next to a 17-bit and a 32-bit one (the BALANCED = false instantiations at their largest spread), and on the
    two rings either side of the factor-2 boundary (qmax - 1) / 2 < qmin that chooses between the instantiations,
  * on words drawn from {0, 1, q-2, q-1, (q-1)/2, (q+1)/2} (helpers.extreme_words), with s_pre in {None, [q-1 ...]}.
Every case asserts 8-byte words, compares every output word with the C restatement (pinned to the by-definition model at these
moduli by tests/test_oracle_word64.py) and asserts that every stored word is below its modulus.  The host-callable arithmetic of
the same header is checked against unsigned __int128 at every modulus of ALL_MODULI by tests/test_word64_host.py."""
import numpy as np
import pytest

from helpers import (assert_reduced, centred_extreme_words, extreme_words, oracle_full_mul, oracle_full_mul_general,
                     oracle_mul_relin_base2, primes_1_mod, primes_below)

pytestmark = pytest.mark.gpu

M16 = 1 << 16                                                   # moduli = 1 mod 2^16 serve every n <= 2^15
TOP5 = primes_below(M16, 5, 1 << 62)
TOP3 = TOP5[:3]
LOW2 = primes_1_mod(M16, 2, 1 << 31)
MIXED = [TOP3[0], 65537, LOW2[0]]                               # a 62-bit limb next to a 17-bit and a 32-bit one
MIXED_LAST = [65537, LOW2[0], TOP3[0]]                          # the same limbs in another drop order
_HALF = (TOP3[0] - 1) // 2
EDGE_BAL = [TOP3[0], primes_1_mod(M16, 1, _HALF)[0]]            # the first prime above (qmax - 1) / 2: still balanced
EDGE_UNBAL = [TOP3[0], primes_below(M16, 1, _HALF)[0]]          # the last one below it: not any more
EIGHT_TOP = primes_below(1 << 12, 8, 1 << 62)
TUNNEL_TOP2 = primes_below(1 << 13, 2, 1 << 62)
MIXED_FULL = MIXED + TOP3[1:]                                   # MIXED plus two more 62-bit limbs
GEN_M = (33, 1820)                                              # 3 * 11 and 4 * 5 * 7 * 13: every odd prime the general engine serves
GEN_TOP2 = {m: primes_below(m, 2, 1 << 62) for m in GEN_M}
GEN_SMALL = {m: primes_1_mod(m, 1, 0)[0] for m in GEN_M}
STATUS_TOP = primes_below(64, 1, 1 << 62)[0]
STATUS_OVER = primes_1_mod(64, 1, (1 << 62) - 1)[0]            # the smallest prime >= 2^62 that is 1 mod 64

ALL_MODULI = sorted(set(TOP5 + LOW2 + MIXED + EDGE_BAL + EDGE_UNBAL + EIGHT_TOP + TUNNEL_TOP2 + [STATUS_TOP]
                        + [q for m in GEN_M for q in GEN_TOP2[m] + [GEN_SMALL[m]]]))

RINGS = {"TOP3": TOP3, "LOW2": LOW2, "MIXED": MIXED, "MIXED_LAST": MIXED_LAST, "EDGE_BAL": EDGE_BAL, "EDGE_UNBAL": EDGE_UNBAL,
         "TOP1": TOP3[:1], "TOP2": TOP3[:2]}


def test_the_moduli_are_where_the_cases_need_them():
    assert TOP3 == [4611686018427322369, 4611686018425815041, 4611686018423390209] and LOW2 == [2148728833, 2148794369]
    assert all((1 << 61) < q < (1 << 62) for q in TOP5 + EIGHT_TOP + TUNNEL_TOP2 + [STATUS_TOP])
    assert all((1 << 31) < q < (1 << 31) + (1 << 21) for q in LOW2)
    assert STATUS_TOP < (1 << 62) <= STATUS_OVER
    # the boundary r->balanced = (qmax - 1) / 2 < qmin
    assert (max(EDGE_BAL) - 1) // 2 < min(EDGE_BAL)
    assert not (max(EDGE_UNBAL) - 1) // 2 < min(EDGE_UNBAL)
    assert min(EDGE_BAL) - min(EDGE_UNBAL) < 1 << 32              # and both sit next to it
    for qs in (MIXED, MIXED_LAST, MIXED_FULL):
        assert not (max(qs) - 1) // 2 < min(qs)
    for qs in (TOP5, LOW2, EIGHT_TOP, TUNNEL_TOP2):
        assert (max(qs) - 1) // 2 < min(qs)


def _ring(oracle_lib, n, qs):
    import alchemy_amd as A
    g = A.Ring(2 * n, qs)                                        # a refusal (ALCH_E_UNSUPPORTED included) raises: the test fails
    assert g.word_bytes == 8
    return g, oracle_lib.Ring(n, qs)


def _minus_one(qs):
    return [q - 1 for q in qs]


# ---- transforms ----------------------------------------------------------------------------------------------------------------------
CRT_CASES = [(logn, name, half) for logn in (4, 8, 11, 12, 14) for name in ("TOP1", "LOW1", "MIXED")
             for half in ((0, 1) if logn == 14 else (None,)) if name != "MIXED" or logn <= 11] + [(15, "TOP1+LOW1", None)]
CRT_RINGS = {"TOP1": [TOP3[:1]], "LOW1": [LOW2[:1]], "MIXED": [MIXED], "TOP1+LOW1": [TOP3[:1], LOW2[:1]]}


@pytest.mark.parametrize("logn,name,half", CRT_CASES, ids=[f"logn{c[0]}-{c[1]}" + ("" if c[2] is None else f"-half{c[2]}") for c in CRT_CASES])
def test_crt_crtinv_and_products(oracle_lib, logn, name, half):
    """k_crt<LOGN,u64>, k_crt_half<14,u64> (option crt_half), k_crt_split (n = 2^15, both one-limb rings in one case): crt in place,
    crtInv of it, crtInv on CRT-basis input, and the product of two transforms."""
    n = 1 << logn
    for qs in CRT_RINGS[name]:
        g, o = _ring(oracle_lib, n, qs)
        if half is not None:
            g.set_option("crt_half", half)
        rng = np.random.default_rng(6200 + logn)
        x = extreme_words(rng, 2, n, qs)
        want = [o.crt(e) for e in x]
        buf = g.upload(x)
        buf.crt()
        got = buf.download()
        assert_reduced(got, qs)
        for e in range(2):
            assert np.array_equal(got[e], want[e]), f"crt mismatch elem {e}"
        prod = g.alloc(1)
        prod.mul(buf.view(0, 1), buf.view(1, 1), 1)
        got = prod.download()
        assert_reduced(got, qs)
        assert np.array_equal(got[0], o.mul(want[0], want[1])), "product of two transforms"
        buf.crtinv()
        assert np.array_equal(buf.download(), x), "crtInv . crt != id"
        prod.crtinv()
        got = prod.download()
        assert_reduced(got, qs)
        assert np.array_equal(got[0], o.crtinv(o.mul(want[0], want[1])))
        y = extreme_words(rng, 1, n, qs)                             # extreme words AS CRT-basis input
        b2 = g.upload(y)
        b2.crtinv()
        got = b2.download()
        assert_reduced(got, qs)
        assert np.array_equal(got[0], o.crtinv(y[0]))
        del buf, prod, b2, g


# ---- keySwitchQuadCirc hint (a * b) --------------------------------------------------------------------------------------------------
def _relin_case(oracle_lib, n, qs, batch, seed, minus_one, pow_basis=False):
    from alchemy_amd import capi
    g, o = _ring(oracle_lib, n, qs)
    L = len(qs)
    rng = np.random.default_rng(seed)
    hint = extreme_words(rng, 2 * L, n, qs)
    a, b = extreme_words(rng, 2 * batch, n, qs), extreme_words(rng, 2 * batch, n, qs)
    s_pre = _minus_one(qs) if minus_one else None
    gout = g.alloc(2 * batch)
    g.ct_mul_relin(g.hint_load(hint), g.upload(a), g.upload(b), gout, batch, s_pre=s_pre,
                   flags=(capi.ALCH_POW_IN | capi.ALCH_POW_OUT) if pow_basis else 0)
    got = gout.download()
    assert_reduced(got, qs)
    for ct in range(batch):
        w0, w1 = o.ct_mul_relin(list(hint), a[2 * ct], a[2 * ct + 1], b[2 * ct], b[2 * ct + 1], s_pre=s_pre, pow_basis=pow_basis)
        assert np.array_equal(got[2 * ct], w0), f"c0 mismatch ct {ct}"
        assert np.array_equal(got[2 * ct + 1], w1), f"c1 mismatch ct {ct}"


RELIN_RINGS = ["TOP3", "LOW2", "MIXED", "MIXED_LAST", "EDGE_BAL", "EDGE_UNBAL", "TOP1"]


@pytest.mark.parametrize("minus_one", [False, True], ids=["s_default", "s_minus_one"])
@pytest.mark.parametrize("name", RELIN_RINGS)
@pytest.mark.parametrize("logn,batch", [(8, 3), (8, 9), (11, 3), (11, 9)])
def test_ct_mul_relin_crt_basis(oracle_lib, logn, batch, name, minus_one):
    """k_tensor_intt<u64> and k_ks_accum<u64, true / false>; batch 9 is ragged against the group of eight ciphertexts."""
    _relin_case(oracle_lib, 1 << logn, RINGS[name], batch, 6300 + 16 * logn + batch + minus_one, minus_one)


@pytest.mark.parametrize("minus_one", [False, True], ids=["s_default", "s_minus_one"])
def test_ct_mul_relin_eight_62_bit_limbs(oracle_lib, minus_one):
    _relin_case(oracle_lib, 1 << 11, EIGHT_TOP, 2, 6400 + minus_one, minus_one)


@pytest.mark.parametrize("logn", [14, 15])
def test_ct_mul_relin_large(oracle_lib, logn):
    """n = 2^14: the largest LDS-resident 64-bit transform; n = 2^15: split transforms and the unfused key switch."""
    _relin_case(oracle_lib, 1 << logn, TOP3[:2], 2, 6410 + logn, minus_one=True)


@pytest.mark.parametrize("minus_one", [False, True], ids=["s_default", "s_minus_one"])
def test_ct_mul_relin_pow_basis(oracle_lib, minus_one):
    _relin_case(oracle_lib, 1 << 8, TOP3[:2], 3, 6420 + minus_one, minus_one, pow_basis=True)


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


@pytest.mark.parametrize("minus_one", [False, True], ids=["s_default", "s_minus_one"])
@pytest.mark.parametrize("name", ["TOP3", "MIXED", "EDGE_BAL", "EDGE_UNBAL"])
@pytest.mark.parametrize("logn", [8, 11])
def test_ct_mul_relin_digits_at_the_ends(oracle_lib, logn, name, minus_one):
    """The digits k_ks_accum reads are the centred lifts of +-x: both ends of the centred range of a 62-bit limb, into 62-bit limbs
    (v = z + q) and into a 17-bit and a 32-bit one (z + dig_off, then a Montgomery product).  On EDGE_BAL / EDGE_UNBAL the digits
    within 2^32 of +-(qmax - 1) / 2 are the only ones that tell the two instantiations apart (z + q' < 0 for the second ring's q'):
    products of uniform or extreme operands never land there, these digits do."""
    n, qs, batch = 1 << logn, RINGS[name], 2
    g, o = _ring(oracle_lib, n, qs)
    L = len(qs)
    rng = np.random.default_rng(6500 + 4 * logn + minus_one)
    hint = extreme_words(rng, 2 * L, n, qs)
    a, b, x = _digit_operands(rng, o, batch, n, qs)
    s_pre = _minus_one(qs) if minus_one else None
    for ct in range(batch):
        c2 = o.crtinv(o.scale(o.mul(a[2 * ct + 1], b[2 * ct + 1]), s_pre if s_pre else [1] * L))
        want = np.stack([(q - x[ct][:, j]) % q for j, q in enumerate(qs)], axis=1) if minus_one else x[ct]
        assert np.array_equal(c2, want), f"ct {ct}: the digits are not the centred lifts of +-x"
    gout = g.alloc(2 * batch)
    g.ct_mul_relin(g.hint_load(hint), g.upload(a), g.upload(b), gout, batch, s_pre=s_pre)
    got = gout.download()
    assert_reduced(got, qs)
    for ct in range(batch):
        w0, w1 = o.ct_mul_relin(list(hint), a[2 * ct], a[2 * ct + 1], b[2 * ct], b[2 * ct + 1], s_pre=s_pre)
        assert np.array_equal(got[2 * ct], w0), f"c0 mismatch ct {ct}"
        assert np.array_equal(got[2 * ct + 1], w1), f"c1 mismatch ct {ct}"


@pytest.mark.parametrize("minus_one", [False, True], ids=["s_default", "s_minus_one"])
@pytest.mark.parametrize("qs", [TOP3[:2], [TOP3[0], 65537]], ids=["TOP2", "top_and_17_bit"])
def test_ct_mul_relin_base2_hint_62_digits(oracle_lib, qs, minus_one):
    """k_crt_base2_digits<u64>: 62 digits on a 62-bit limb, shift counts up to 61.  c2 = +-x with x from {0, 1, q-1, (q-1)/2,
    (q+1)/2, (q-3)/2}: +-(q-1)/2 sets every digit position and the absorbing top digit, with either sign."""
    from alchemy_amd import capi
    from oracle import model
    n, batch = 1 << 8, 2
    g, o = _ring(oracle_lib, n, qs)
    D = g.gadget_digits(capi.ALCH_GAD_BASE2)
    assert model.baseb_digits(TOP3[0]) == 62 and D == sum(model.baseb_digits(q) for q in qs)
    rng = np.random.default_rng(6600 + len(str(qs[1])) + minus_one)
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


# ---- PT2CT's whole mul_ ----------------------------------------------------------------------------------------------------------------
# (id, moduli of the hint's ring, L_in, L_out, Pow-basis output)
FULL_CASES = [
    ("4-5-3", TOP5, 4, 3, False),                 # k_ks_accum with dup = 1, k_rescale_out_lin<u64, 2, true>
    ("3-4-2", TOP5[:4], 3, 2, False),
    ("2-3-1", TOP5[:3], 2, 1, False),
    ("3-4-3", TOP5[:4], 3, 3, False),             # one limb dropped, balanced: k_rescale_out_lin<u64, 1, true>
    ("4-5-3-pow", TOP5, 4, 3, True),              # Pow-basis output: k_rescale_out<u64>
    ("2-5-2", TOP5, 2, 2, False),                 # dup = 3 and a three-limb drop: k_rescale_out<u64>
    ("mixed-4-5-3", MIXED_FULL, 4, 3, False),     # drops the 62-bit and the 17-bit limb: an unbalanced two-limb drop, k_rescale_out<u64>
    ("mixed-4-5-4", MIXED_FULL, 4, 4, False),     # drops the 62-bit limb above a 17-bit one: k_rescale_out_lin<u64, 1, false>
]


@pytest.mark.parametrize("minus_one", [False, True], ids=["s_default", "s_minus_one"])
@pytest.mark.parametrize("case", FULL_CASES, ids=[c[0] for c in FULL_CASES])
@pytest.mark.parametrize("logn", [8, 11])
def test_ct_mul_full(oracle_lib, logn, case, minus_one):
    import alchemy_amd as A
    from alchemy_amd import capi
    _, qs_h, l_in, l_out, pow_out = case
    n, batch, L = 1 << logn, 3, len(qs_h)
    qs_in, qs_out = qs_h[L - l_in:], qs_h[L - l_out:]
    rin, rh, rout = A.Ring(2 * n, qs_in), A.Ring(2 * n, qs_h), A.Ring(2 * n, qs_out)
    assert rin.word_bytes == rh.word_bytes == rout.word_bytes == 8
    rng = np.random.default_rng(6700 + logn + 2 * L + l_in + minus_one)
    hint = extreme_words(rng, 2 * L, n, qs_h)
    a, b = extreme_words(rng, 2 * batch, n, qs_in), extreme_words(rng, 2 * batch, n, qs_in)
    s_pre = _minus_one(qs_in) if minus_one else None
    gout = rout.alloc(2 * batch)
    capi.ct_mul_full(rh.hint_load(hint), rin.upload(a), rin.upload(b), gout, batch, s_pre=s_pre, flags=capi.ALCH_POW_OUT if pow_out else 0)
    got = gout.download()
    assert_reduced(got, qs_out)
    for ct in range(batch):
        w0, w1 = oracle_full_mul(oracle_lib, n, qs_h, l_in, l_out, list(hint), a[2 * ct], a[2 * ct + 1], b[2 * ct], b[2 * ct + 1],
                                 s_pre=s_pre, pow_out=pow_out)
        assert np.array_equal(got[2 * ct], w0), f"c0 mismatch ct {ct}"
        assert np.array_equal(got[2 * ct + 1], w1), f"c1 mismatch ct {ct}"


# (id, moduli of the hint's ring, L_in, L_out)
RESCALE_END_CASES = [
    ("top-4-5-3", TOP5, 4, 3),
    ("edge_bal-2-3-1", [TOP3[1]] + EDGE_BAL, 2, 1),       # q_u = the largest prime dropped above the first prime over (q_u - 1) / 2
    ("edge_unbal-2-3-1", [TOP3[1]] + EDGE_UNBAL, 2, 1),   # ... and above the last one under it: DropTab::balanced = 0
    ("mixed-4-5-3", MIXED_FULL, 4, 3),
    ("edge_unbal-2-3-2", [TOP3[1]] + EDGE_UNBAL, 2, 2),   # only the added limb is dropped: k_rescale_out_lin<u64, 1, false> on zeros
]


@pytest.mark.parametrize("minus_one", [False, True], ids=["plus_x", "minus_x"])
@pytest.mark.parametrize("case", RESCALE_END_CASES, ids=[c[0] for c in RESCALE_END_CASES])
def test_ct_mul_full_rescale_at_the_ends(oracle_lib, case, minus_one):
    """The closing modSwitch on centred lifts at both ends of their range.  With a zero hint, a0 = a1 = crt(1), b0 = crt(x), b1 = crt(y)
    and s_pre = +-(added modulus)^-1 the key switch hands (+-q_a x, +-q_a y) on to the rescale: the added limb holds zeros, and the
    next dropped limb holds +-x, +-y with x, y per coefficient from {0, 1, q-1, (q-1)/2, (q+1)/2, (q-3)/2} -- lifts that products of
    random words never reach, and the only ones that tell a balanced drop table from an unbalanced one on the EDGE rings."""
    import alchemy_amd as A
    from alchemy_amd import capi
    _, qs_h, l_in, l_out = case
    n, batch, L = 1 << 8, 3, len(qs_h)
    assert L - l_in == 1
    qs_in, qs_out = qs_h[1:], qs_h[L - l_out:]
    rin, rh, rout = A.Ring(2 * n, qs_in), A.Ring(2 * n, qs_h), A.Ring(2 * n, qs_out)
    assert rin.word_bytes == rh.word_bytes == rout.word_bytes == 8
    o_in = oracle_lib.Ring(n, qs_in)
    rng = np.random.default_rng(6750 + L + l_out + minus_one)
    one = np.zeros((n, l_in), dtype=np.int64)
    one[0, :] = 1
    one_crt = o_in.crt(one)
    x = centred_extreme_words(rng, 2 * batch, n, qs_in)
    a = np.stack([one_crt] * (2 * batch))
    b = np.stack([o_in.crt(e) for e in x])
    hint = np.zeros((2 * L, n, L), dtype=np.int64)
    s_pre = [pow(qs_h[0], -1, q) for q in qs_in]
    if minus_one:
        s_pre = [q - v for v, q in zip(s_pre, qs_in)]
    gout = rout.alloc(2 * batch)
    for pow_out in (False, True):
        capi.ct_mul_full(rh.hint_load(hint), rin.upload(a), rin.upload(b), gout, batch, s_pre=s_pre, flags=capi.ALCH_POW_OUT if pow_out else 0)
        got = gout.download()
        assert_reduced(got, qs_out)
        for ct in range(batch):
            w0, w1 = oracle_full_mul(oracle_lib, n, qs_h, l_in, l_out, list(hint), a[2 * ct], a[2 * ct + 1], b[2 * ct], b[2 * ct + 1],
                                     s_pre=s_pre, pow_out=pow_out)
            assert np.array_equal(got[2 * ct], w0), f"c0 mismatch ct {ct}"
            assert np.array_equal(got[2 * ct + 1], w1), f"c1 mismatch ct {ct}"


def test_mul_steps_chain(oracle_lib):
    """alch_ct_mul, alch_ct_mod_switch_deg (up, degree 2), alch_ct_key_switch_quad, alch_ct_mod_switch_deg (down): every step against
    the oracle, 4 -> 5 -> 3 limbs on five 62-bit primes, and the chain's result against alch_ct_mul_full."""
    import alchemy_amd as A
    from alchemy_amd import capi, mulsteps as MS
    n, batch, qs_h, l_in, l_out = 1 << 8, 3, TOP5, 4, 3
    L = len(qs_h)
    qs_in, qs_out = qs_h[L - l_in:], qs_h[L - l_out:]
    rin, rh, rout = A.Ring(2 * n, qs_in), A.Ring(2 * n, qs_h), A.Ring(2 * n, qs_out)
    assert rin.word_bytes == rh.word_bytes == rout.word_bytes == 8
    o_in, o_h, o_out = oracle_lib.Ring(n, qs_in), oracle_lib.Ring(n, qs_h), oracle_lib.Ring(n, qs_out)
    rng = np.random.default_rng(6800)
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


# ---- element-wise ops, gadget decompositions, rescale ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["TOP3", "MIXED", "EDGE_UNBAL"])
def test_elementwise_decompose_and_rescale(oracle_lib, name):
    """k_decompose_triv<u64> balanced and not, BaseBGad 2 digits, alch_buf_rescale_drop0, scale, add, sub, mulPublic, addPublic at
    n = 64."""
    n, qs = 64, RINGS[name]
    g, o = _ring(oracle_lib, n, qs)
    L = len(qs)
    rng = np.random.default_rng(6900 + L + len(name))
    x = extreme_words(rng, 6, n, qs)
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
    for e in range(2):
        want = o.decompose_triv(x[e])
        got = g.decompose_triv(x[e])
        assert len(got) == L
        for i in range(L):
            assert_reduced(got[i], qs)
            assert np.array_equal(got[i], want[i]), ("decompose_triv", e, i)
        dig = g.alloc(L + 1)
        gx.decompose_triv_into(e, dig, 1)
        same(dig.view(1, L), want)
    want = o.decompose_base2(x[0])
    got = g.decompose_base2(x[0])
    assert len(got) == len(want) == sum((q - 1).bit_length() for q in qs)
    for i in range(len(want)):
        assert_reduced(got[i], qs)
        assert np.array_equal(got[i], want[i]), ("decompose_base2", i)
    # Rescale (a, b) -> b, limb 0 dropped
    import alchemy_amd as A
    gsmall = A.Ring(2 * n, qs[1:])
    out = gsmall.alloc(6)
    gx.rescale_drop0_into(out, 6)
    same(out, [o.rescale_drop0(e) for e in x], qs[1:])


# ---- tunnels between two-power rings ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("minus_one", [False, True], ids=["s_default", "s_minus_one"])
@pytest.mark.parametrize("gadget", ["triv", "base2"])
@pytest.mark.parametrize("name", ["TOP2", "MIXED"])
@pytest.mark.parametrize("rp,sp", [(64, 128), (128, 64)])
def test_tunnel_twopower_small(oracle_lib, rp, sp, name, gadget, minus_one):
    """The u64 inner product (plain Montgomery form) of do_tunnel_pow2, every ALCH_POW_IN / ALCH_POW_OUT combination."""
    from alchemy_amd import capi
    from test_gpu_tunnel_twopower import check_parity, need_twopower_tunnels
    need_twopower_tunnels()
    qs = TUNNEL_TOP2 if name == "TOP2" else MIXED
    flag_sets = (0, capi.ALCH_POW_IN, capi.ALCH_POW_OUT, capi.ALCH_POW_IN | capi.ALCH_POW_OUT)
    check_parity(oracle_lib, rp, sp, qs, gadget, 3, False, flag_sets, words=extreme_words, s_pre=_minus_one(qs) if minus_one else None,
                 word_bytes=8)


def test_tunnel_twopower_n2048_to_n4096(oracle_lib):
    from test_gpu_tunnel_twopower import check_parity, need_twopower_tunnels
    need_twopower_tunnels()
    check_parity(oracle_lib, 1 << 12, 1 << 13, TUNNEL_TOP2, "triv", 2, False, (0,), words=extreme_words, s_pre=_minus_one(TUNNEL_TOP2),
                 word_bytes=8)


# ---- general index -----------------------------------------------------------------------------------------------------------------------
def _gen_rings():
    return [(m, qs) for m in GEN_M for qs in (GEN_TOP2[m], [GEN_TOP2[m][0], GEN_SMALL[m]])]


@pytest.mark.parametrize("m,qs", _gen_rings(), ids=[f"m{m}-{'top2' if min(qs) > 1 << 61 else 'mixed'}" for m, qs in _gen_rings()])
def test_general_index_tensor_methods(oracle_lib, m, qs):
    """inst_gen64: the passes for p in {3, 11} (m = 33) and {2, 5, 7, 13} (m = 1820) on extreme words."""
    import alchemy_amd as A
    from alchemy_amd import capi
    g, o = A.Ring(m, qs), oracle_lib.GenRing(m, qs)
    assert g.word_bytes == 8 and g.n == o.n
    rng = np.random.default_rng(7000 + m)
    x = extreme_words(rng, 3, g.n, qs)

    def same(buf, want):
        got = buf.download()
        assert_reduced(got, qs)
        assert np.array_equal(got, np.stack(want))

    for name in ("crt", "crtinv", "l", "linv", "mulg_pow", "mulg_dec", "mulg_crt", "divg_crt"):
        got = getattr(g, name)(x[0])
        assert_reduced(got, qs)
        assert np.array_equal(got, getattr(o, name)(x[0])), name
    for name in ("divg_pow", "divg_dec"):
        want, got = getattr(o, name)(x[0]), getattr(g, name)(x[0])
        assert want is not None and got is not None, name          # g is a unit modulo these primes
        assert_reduced(got, qs)
        assert np.array_equal(got, want), name
    buf = g.upload(x)
    buf.crt()
    crt = [o.crt(e) for e in x]
    same(buf, crt)
    prod = g.alloc(1)
    prod.mul(buf.view(0, 1), buf.view(1, 1), 1)
    same(prod, [o.mul(crt[0], crt[1])])
    buf.mulg(capi.ALCH_BASIS_CRT, 1, 2)
    same(buf, [crt[0], o.mulg_crt(crt[1]), o.mulg_crt(crt[2])])
    assert buf.divg(capi.ALCH_BASIS_CRT, 1, 2)
    same(buf, crt)
    buf.crtinv()
    same(buf, x)
    buf.mulg(capi.ALCH_BASIS_POW, 0, 2)
    same(buf, [o.mulg_pow(x[0]), o.mulg_pow(x[1]), x[2]])
    assert buf.divg(capi.ALCH_BASIS_POW, 0, 2)
    same(buf, x)
    buf.linv(0, 2)
    same(buf, [o.linv(x[0]), o.linv(x[1]), x[2]])
    buf.mulg(capi.ALCH_BASIS_DEC, 0, 1)
    same(buf, [o.mulg_dec(o.linv(x[0])), o.linv(x[1]), x[2]])
    assert buf.divg(capi.ALCH_BASIS_DEC, 0, 1)
    buf.l(0, 2)
    same(buf, x)


@pytest.mark.parametrize("minus_one", [False, True], ids=["s_default", "s_minus_one"])
@pytest.mark.parametrize("m,qs", _gen_rings(), ids=[f"m{m}-{'top2' if min(qs) > 1 << 61 else 'mixed'}" for m, qs in _gen_rings()])
def test_general_index_ct_mul_relin(oracle_lib, m, qs, minus_one):
    """k_gen_tensor_inv and k_gen_ks on 64-bit words."""
    import alchemy_amd as A
    g, o = A.Ring(m, qs), oracle_lib.GenRing(m, qs)
    assert g.word_bytes == 8
    L, batch = len(qs), 3
    rng = np.random.default_rng(7100 + m + minus_one)
    hint, a, b = extreme_words(rng, 2 * L, g.n, qs), extreme_words(rng, 2 * batch, g.n, qs), extreme_words(rng, 2 * batch, g.n, qs)
    s_pre = _minus_one(qs) if minus_one else None
    gout = g.alloc(2 * batch)
    g.ct_mul_relin(g.hint_load(hint), g.upload(a), g.upload(b), gout, batch, s_pre=s_pre)
    got = gout.download()
    assert_reduced(got, qs)
    for ct in range(batch):
        w0, w1 = o.ct_mul_relin(list(hint), a[2 * ct], a[2 * ct + 1], b[2 * ct], b[2 * ct + 1], s_pre)
        assert np.array_equal(got[2 * ct], w0) and np.array_equal(got[2 * ct + 1], w1), ct


# (hint ring as a function of the two 62-bit primes and the small one, L_in, L_out)
GEN_FULL = {"top2": (lambda top, small: [top[1], top[0]], 1, 1),                      # a 62-bit limb dropped above a 62-bit one
            "small_over_big": (lambda top, small: [small, top[0]], 1, 1),             # the small limb dropped above a 62-bit one
            "big_over_small": (lambda top, small: [top[0], small, top[1]], 2, 2)}     # a 62-bit limb's centred lift reduced into the small one


@pytest.mark.parametrize("pow_out", [False, True], ids=["crt_out", "pow_out"])
@pytest.mark.parametrize("m", GEN_M)
@pytest.mark.parametrize("order", list(GEN_FULL))
def test_general_index_ct_mul_full(oracle_lib, m, order, pow_out):
    """k_gen_rescale_* behind the general key switch, one limb added and dropped again; every ring involved has 8-byte words."""
    import alchemy_amd as A
    from alchemy_amd import capi
    make, l_in, l_out = GEN_FULL[order]
    qs_h = make(GEN_TOP2[m], GEN_SMALL[m])
    L = len(qs_h)
    qs_in, qs_out = qs_h[L - l_in:], qs_h[L - l_out:]
    rh, rin, rout = A.Ring(m, qs_h), A.Ring(m, qs_in), A.Ring(m, qs_out)
    assert rh.word_bytes == rin.word_bytes == rout.word_bytes == 8
    batch = 2
    rng = np.random.default_rng(7200 + m + len(order))
    hint = extreme_words(rng, 2 * L, rh.n, qs_h)
    a, b = extreme_words(rng, 2 * batch, rh.n, qs_in), extreme_words(rng, 2 * batch, rh.n, qs_in)
    s_pre = _minus_one(qs_in)
    gout = rout.alloc(2 * batch)
    capi.ct_mul_full(rh.hint_load(hint), rin.upload(a), rin.upload(b), gout, batch, s_pre=s_pre, flags=capi.ALCH_POW_OUT if pow_out else 0)
    got = gout.download()
    assert_reduced(got, qs_out)
    for ct in range(batch):
        w0, w1 = oracle_full_mul_general(oracle_lib, m, qs_h, l_in, l_out, list(hint), a[2 * ct], a[2 * ct + 1], b[2 * ct], b[2 * ct + 1],
                                         s_pre, pow_out)
        assert np.array_equal(got[2 * ct], w0) and np.array_equal(got[2 * ct + 1], w1), ct


# ---- statuses ------------------------------------------------------------------------------------------------------------------------------
def test_the_accepted_range_ends_at_2_62():
    """The largest prime below 2^62 that is 1 mod 64 creates a ring; the smallest one at or above 2^62 answers ALCH_E_UNSUPPORTED on the
    two-power engine (m = 64) and on the general one (m = 16: a two-power index below 32 runs there)."""
    import alchemy_amd as A
    from alchemy_amd import capi
    ring = A.Ring(64, [STATUS_TOP])
    assert ring.word_bytes == 8 and ring.n == 32
    buf = ring.alloc(1)
    buf.fill_uniform(1)
    before = buf.download()
    assert_reduced(before, [STATUS_TOP])
    buf.crt()
    buf.crtinv()
    assert np.array_equal(buf.download(), before)
    for m in (64, 16):
        code = None
        try:
            A.Ring(m, [STATUS_OVER])
        except A.AlchemyError as e:
            code = e.code
        assert code == capi.ALCH_E_UNSUPPORTED, (m, code)
        code = None
        try:
            A.Ring(m, [STATUS_TOP, STATUS_OVER])
        except A.AlchemyError as e:
            code = e.code
        assert code == capi.ALCH_E_UNSUPPORTED, (m, code)
