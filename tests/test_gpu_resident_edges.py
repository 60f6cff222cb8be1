"""GPU: the resident-batch entry points and the Tensor methods between two indices at the edges of both word sizes.

tests/test_gpu_word64_edges.py and tests/test_gpu_word32_edges.py pin the transforms, the key switch and the closing modSwitch at
the extremes of their modulus ranges; the entry points that arrived later ran on primes next to 2^29 or 2^60 and mostly on uniform
words.  Here they run
  * on the two largest primes below 2^31 (TOP31: a + b < 2q has 2^17 to spare in a 4-byte word) and below 2^62 (TOP62), on the first
    two primes above 2^31 (LOW64: the smallest ring on 8-byte words, 32 digits per limb),
  * with the largest 31-bit prime next to a 17-bit and a 21-bit one (MIX31), the largest 62-bit prime next to a 17-bit and a 32-bit
    one (MIX64), and on either side of (qmax - 1) / 2 < qmin for either top prime (EDGE_*; helpers.resident_edge_rings),
  * on words from {0, 1, q-2, q-1, (q-1)/2, (q+1)/2} (helpers.extreme_words) and on the element that is q-1 everywhere.
Indices: m' = 45 (n = 24: g table, 16-byte packs on both word sizes), 27 (n = 18: one 4-byte word per lane), 64 (two-power, no g),
one n = 1024 row for alch_ct_add; batches 1 and 3.

  1. test_between_index_methods        k_ext_gather_rows<W>, k_ext_twace_crt<W> (alch_buf_embed / _twace / _coeffs), <u64> included
  2. test_ct_add                       k_ct_add<W, VW, DA, DB> (alch_ct_add), every degree pair and g-power pair, out aliasing an operand
  3. test_ct_encrypt, test_ks_hint*    k_ct_encrypt<W, VW>, k_ct_ks_hint<W, VW> (alch_ct_encrypt, alch_ct_ks_hint, alch_ct_ks_hint_part)
  4. test_gauss_dec                    k_gauss_sample<W, true> / k_gauss_round<W>: both branches of gauss::reduce in one launch

References: Python integers and the by-definition model (oracle/model_gen.py), the C restatement for the encrypt product and
tests/gauss_model.py for the sampler; tests/test_oracle_resident_edges.py pins them at these moduli without a GPU.  Every comparison
is exact, every case asserts the word size of every ring it creates and that every stored word is below its modulus."""
import functools

import numpy as np
import pytest

from helpers import RESIDENT_WORD_BYTES, assert_reduced, check_resident_edge_rings, extreme_words, resident_edge_rings
from oracle import model_gen as G

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
ALL_RINGS = list(RESIDENT_WORD_BYTES)
CORE_RINGS = ["TOP31", "MIX31", "LOW64", "TOP62", "MIX64"]
EXT_PAIRS = [(9, 45), (8, 40), (4, 8), (32, 96), (1, 7)]                    # (m, m'): moduli = 1 mod m' on both rings
ADD_CASES = ([(mp, name) for mp in (45, 27, 64) for name in ALL_RINGS if mp == 45 or not name.startswith("EDGE")]
             + [(2048, "TOP31"), (2048, "TOP62")])                           # n = 1024: a row spans several workgroups
RLWE_M = (45, 64)
BASE2_DIGITS = {"TOP31": 62, "MIX31": 31 + 17 + 21, "LOW64": 64, "TOP62": 124, "MIX64": 62 + 17 + 32}
GAUSS_RINGS = {"MIX31": lambda r: r["MIX31"], "MIX64": lambda r: r["MIX64"], "TOP31_1": lambda r: r["TOP31"][:1]}
GAUSS_COSETS = [None, 7, (1 << 31) - 1]
GAUSS_SIGMA = float(1 << 21)                                                # |z| passes a 17-bit limb, 9 sigma stays far below 2^30
INDICES = sorted({45, 27, 64, 2048} | {mb for _, mb in EXT_PAIRS})

rings = functools.lru_cache(maxsize=None)(resident_edge_rings)


def ints(a):
    return np.asarray(a).astype(object)


def minus_one_element(n, qs):
    return np.ascontiguousarray(np.broadcast_to(np.array([q - 1 for q in qs], dtype=np.int64), (n, len(qs))))


def make_ring(m, name, qs=None):
    import alchemy_amd as A
    qs = rings(m)[name] if qs is None else qs
    ring = A.Ring(m, qs)                                                     # a refusal raises: the test fails
    assert ring.word_bytes == RESIDENT_WORD_BYTES[name], (m, name)
    return ring


def check_the_moduli():
    """The part of the moduli test that needs no ring (run on the CPU by tests/test_oracle_resident_edges.py)."""
    from test_tensor_ext import PAIRS
    assert set(EXT_PAIRS) <= set(PAIRS)
    for m in INDICES:
        r = rings(m)
        check_resident_edge_rings(r)
        assert all(q % m == 1 for qs in r.values() for q in qs), m
    assert rings(45) == {"TOP31": [2147482801, 2147482621], "MIX31": [2147482801, 65701, 1048681],
                         "EDGE_BAL31": [2147482801, 1073741671], "EDGE_UNBAL31": [2147482801, 1073741311],
                         "LOW64": [2147484061, 2147484331], "TOP62": [4611686018427387631, 4611686018427387271],
                         "MIX64": [4611686018427387631, 65701, 2147484061],
                         "EDGE_BAL62": [4611686018427387631, 2305843009213693951],
                         "EDGE_UNBAL62": [4611686018427387631, 2305843009213692601]}
    assert rings(64)["TOP31"] == [2147483137, 2147482817] and rings(64)["MIX64"] == [4611686018427387329, 65537, 2147483713]
    for name, digits in BASE2_DIGITS.items():
        for m in RLWE_M:
            assert sum((q - 1).bit_length() for q in rings(m)[name]) == digits, (m, name)


def test_the_moduli_are_where_the_cases_need_them():
    check_the_moduli()
    for m in (45, 64):                                                       # the word size each ring gets
        for name in ALL_RINGS:
            make_ring(m, name)


# ---- 1. the Tensor methods between two indices --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CORE_RINGS)
@pytest.mark.parametrize("m,mb", EXT_PAIRS, ids=[f"{m}-{mb}" for m, mb in EXT_PAIRS])
def test_between_index_methods(m, mb, name):
    """alch_buf_embed (Pow, Dec, CRT), alch_buf_twace (Pow, Dec, CRT) and alch_buf_coeffs with count 3: two extreme elements and the
    element q-1 everywhere, which in the CRT basis puts every term of twaceCRT's fibre sum and the sum after every conditional
    subtraction at its largest.  Against the model limb by limb; then crt . embedPow = embedCRT . crt and crt . twacePowDec =
    twaceCRT . crt on the extreme elements, both sides also against crt by definition."""
    from alchemy_amd import capi
    qs = rings(mb)[name]
    s, b = G.Index(m), G.Index(mb)
    rs, rb = make_ring(m, name, qs), make_ring(mb, name, qs)
    assert (rs.n, rb.n) == (s.n, b.n)
    B = 3
    rng = np.random.default_rng(9100 + 100 * m + mb)
    xs = np.concatenate([extreme_words(rng, 2, s.n, qs), minus_one_element(s.n, qs)[None]])
    ys = np.concatenate([extreme_words(rng, 2, b.n, qs), minus_one_element(b.n, qs)[None]])

    def same(buf, want_limb, src):
        """want_limb(limb values as Python integers, q) -> the limb's values of the result."""
        got = buf.download()
        assert_reduced(got, qs)
        for e in range(B):
            for j, q in enumerate(qs):
                assert got[e][:, j].tolist() == want_limb(src[e][:, j].tolist(), q), (e, j)

    bx, by = rs.upload(xs), rb.upload(ys)
    big, small = rb.alloc(B), rs.alloc(B)
    big.embed_from(bx, B, capi.ALCH_BASIS_POW)
    same(big, lambda v, q: G.embed_pow(v, s, b), xs)
    big.embed_from(bx, B, capi.ALCH_BASIS_DEC)
    same(big, lambda v, q: G.embed_dec_def(v, s, b, q), xs)
    big.embed_from(bx, B, capi.ALCH_BASIS_CRT)
    same(big, lambda v, q: G.embed_crt_def(v, s, b), xs)
    for basis in (capi.ALCH_BASIS_POW, capi.ALCH_BASIS_DEC):
        small.twace_from(by, B, basis)
        same(small, lambda v, q: G.twace_pow_dec(v, s, b), ys)
    small.twace_from(by, B, capi.ALCH_BASIS_CRT)
    same(small, lambda v, q: G.twace_crt_def(v, s, b, q), ys)
    rows = G.coeffs_indices(s, b)
    cbuf = rs.alloc(B * len(rows))
    cbuf.coeffs_from(by, B)
    got = cbuf.download()
    assert_reduced(got, qs)
    got = got.reshape(B, len(rows), s.n, len(qs))
    for e in range(B):
        for j in range(len(qs)):
            assert [c[:, j].tolist() for c in got[e]] == G.coeffs(ys[e][:, j].tolist(), s, b), (e, j)
    assert np.array_equal(bx.download(), xs) and np.array_equal(by.download(), ys)          # sources untouched
    # the identities that make the instance sound
    bx.crt()
    big.embed_from(bx, B, capi.ALCH_BASIS_CRT)                                # embedCRT . crt
    lhs = rb.alloc(B)
    lhs.embed_from(rs.upload(xs), B, capi.ALCH_BASIS_POW)
    lhs.crt()                                                                # crt . embedPow
    assert np.array_equal(lhs.download()[:2], big.download()[:2])
    same(big, lambda v, q: G.crt_def(G.embed_pow(v, s, b), b, q), xs)
    by.crt()
    small.twace_from(by, B, capi.ALCH_BASIS_CRT)                              # twaceCRT . crt
    lhs = rs.alloc(B)
    lhs.twace_from(rb.upload(ys), B, capi.ALCH_BASIS_POW)
    lhs.crt()                                                                # crt . twacePowDec
    assert np.array_equal(lhs.download()[:2], small.download()[:2])
    same(small, lambda v, q: G.crt_def(G.twace_pow_dec(v, s, b), s, q), ys)


# ---- 2. alch_ct_add -----------------------------------------------------------------------------------------------------------------
SCALARS = (lambda q: q - 1, lambda q: 1, lambda q: (q + 1) // 2)


@pytest.mark.parametrize("mp,name", ADD_CASES, ids=[f"m{mp}-{name}" for mp, name in ADD_CASES])
def test_ct_add(mp, name):
    """out = s_a G^g_a a + s_b G^g_b b slot by slot in Python integers, G = the model's CRT image of g: the four degree pairs, the four
    g-power pairs, extreme operands, scalars from {q-1, 1, (q+1)/2} or NULL on one side, out aliasing a and aliasing b where the
    degrees allow; a c2 that only one operand has is scaled, never summed.  Once per ring the unary form with g^3 and no scalar."""
    from alchemy_amd.ctadd import ct_add_raw
    from test_gpu_ct_add import DEG_PAIRS, G_PAIRS
    ring = make_ring(mp, name)
    qs, n, L = rings(mp)[name], ring.n, ring.L
    q = np.array(qs, dtype=object)
    gimg = [G.g_crt(G.Index(mp), qj) for qj in qs]                           # [limb][slot]
    gpow = {g: np.array([[pow(gimg[j][i], g, qs[j]) for j in range(L)] for i in range(n)], dtype=object)
            for g in {g for pair in G_PAIRS for g in pair}}
    rng = np.random.default_rng(9200 + mp)
    combo = 0
    for batch in (1, 3):
        host = {(side, d): extreme_words(rng, (d + 1) * batch, n, qs) for side in "ab" for d in (1, 2)}
        dev = {k: ring.upload(v) for k, v in host.items()}
        terms = {}

        def term(side, d, g, s):
            if (side, d, g) not in terms:
                terms[side, d, g] = ints(host[side, d]).reshape(batch, d + 1, n, L) * gpow[g] % q
            return terms[side, d, g] if s is None else terms[side, d, g] * np.array(s, dtype=object) % q

        for da, db in DEG_PAIRS:
            do, lo = max(da, db), min(da, db)
            for g_a, g_b in G_PAIRS:
                combo += 1
                s_a, s_b = [SCALARS[combo % 3](qj) for qj in qs], [SCALARS[combo // 3 % 3](qj) for qj in qs]
                if combo % 4 == 1:
                    s_a = None
                elif combo % 4 == 3:
                    s_b = None
                ta, tb = term("a", da, g_a, s_a), term("b", db, g_b, s_b)
                want = np.concatenate([(ta[:, :lo + 1] + tb[:, :lo + 1]) % q, (ta if da > db else tb)[:, lo + 1:]], axis=1)
                out = ring.alloc((do + 1) * batch)
                out.fill_uniform(7)
                ct_add_raw(out, batch, dev["a", da], da, s_a, g_a, dev["b", db], db, s_b, g_b)
                got = out.download().reshape(batch, do + 1, n, L)
                assert_reduced(got, qs)
                assert np.array_equal(ints(got), want), (batch, da, db, g_a, g_b)
                for side, d in (("a", da), ("b", db)):
                    if d != do:
                        continue
                    alias = ring.upload(host[side, d])
                    if side == "a":
                        ct_add_raw(alias, batch, alias, da, s_a, g_a, dev["b", db], db, s_b, g_b)
                    else:
                        ct_add_raw(alias, batch, dev["a", da], da, s_a, g_a, alias, db, s_b, g_b)
                    assert np.array_equal(alias.download().reshape(got.shape), got), ("out = " + side, batch, da, db, g_a, g_b)
        for k, v in host.items():
            assert np.array_equal(dev[k].download(), v), k                   # operands untouched
    out = ring.alloc(3 * batch)
    ct_add_raw(out, batch, dev["a", 2], 2, None, 3, None, 0, None, 0)
    got = out.download().reshape(batch, 3, n, L)
    assert_reduced(got, qs)
    assert np.array_equal(ints(got), term("a", 2, 3, None)), "unary form"


# ---- 3. encrypt and hints -----------------------------------------------------------------------------------------------------------
def uniform_word(seed, elem, j, k, n, qs):
    """Word (elem, limb j, slot k) of alch_buf_fill_uniform(seed) in Python integers."""
    from alchemy_amd.encrypt import splitmix64
    return splitmix64((seed + (elem * len(qs) + j) * n + k) & M64) % qs[j]


@pytest.mark.parametrize("name", CORE_RINGS)
@pytest.mark.parametrize("m", RLWE_M)
def test_ct_encrypt(m, name):
    """alch_ct_encrypt with error terms and key from extreme_words, batches 1 and 3: c1 is what the counter rule gives (one element
    also against splitmix64(...) % q in Python integers: the remainder is a software one), c0 = err - c1 s in Python integers."""
    from test_gpu_encrypt import check_ct_encrypt
    qs = rings(m)[name]
    q = np.array(qs, dtype=object)
    for B in (1, 3):
        seed, got, u, e, s = check_ct_encrypt(m, qs, B, words=extreme_words, word_bytes=RESIDENT_WORD_BYTES[name])
        n = got.shape[1]
        assert_reduced(got, qs)
        for b in range(B):
            assert np.array_equal(ints(got[2 * b]), (ints(e[1 + b]) - ints(got[2 * b + 1]) * ints(s)) % q), (B, b)
        elem = 2 * (B - 1) + 1
        assert got[elem].tolist() == [[uniform_word(seed, elem, j, k, n, qs) for j in range(len(qs))] for k in range(n)]
        assert u[elem].tolist() == got[elem].tolist()


@pytest.mark.parametrize("gadget", ["triv", "base2"])
@pytest.mark.parametrize("name", CORE_RINGS)
@pytest.mark.parametrize("m", RLWE_M)
def test_ks_hint(m, name, gadget):
    """alch_ct_ks_hint, both gadgets, n_v = 2, a nonzero offset on every buffer, values / error terms / key from extreme_words, against
    expected_pairs.  The digit counts (62 on TOP31, 64 on LOW64, 124 on TOP62, 62 + 17 + 32 on MIX64) mean the top exponent of every
    limb is reached: (W)1 << 30 on a 4-byte word, 1 << 61 on an 8-byte one."""
    from test_gpu_hints import BASE2, TRIV, check_ks_hint
    qs = rings(m)[name]
    D = check_ks_hint(m, qs, BASE2 if gadget == "base2" else TRIV, words=extreme_words, word_bytes=RESIDENT_WORD_BYTES[name])
    assert D == (BASE2_DIGITS[name] if gadget == "base2" else len(qs))


def test_ks_hint_part_cut_inside_the_17_bit_limb():
    """alch_ct_ks_hint_part on MIX64: one call against two parts cut at entry 62 + 8, inside the 17-bit limb's digits of value 0."""
    from test_gpu_hints import BASE2, check_cut, expected_pairs, same
    m, qs = 45, rings(45)["MIX64"]
    assert (qs[0] - 1).bit_length() == 62 and (qs[1] - 1).bit_length() == 17
    ring, one, v, err, sk, seed, ct0 = check_cut(m, qs, BASE2, 2, 62 + 8, words=extreme_words)
    assert ring.word_bytes == 8
    assert_reduced(one, qs)
    n, L = ring.n, ring.L
    uni = lambda e: np.array([[uniform_word(seed, 2 * ((ct0 + e) & M64) + 1, j, k, n, qs) for j in range(L)] for k in range(n)], dtype=object)
    want = expected_pairs(qs, BASE2, v.download(), err.download(), sk.download()[0], uni)
    assert len(want) == 2 * BASE2_DIGITS["MIX64"]
    for e, (b, a) in enumerate(want):
        assert same(one[2 * e + 1], a) and same(one[2 * e], b), e


# ---- 4. alch_buf_gauss_dec ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(GAUSS_RINGS))
@pytest.mark.parametrize("m", [64, 45])
def test_gauss_dec(m, kind):
    """Three elements at first = 1 of a five-element buffer against tests/gauss_model.py bit for bit, cosets none, 7 and 2^31 - 1.  The
    variance puts sigma at 2^21 on every coordinate: the model's |z| passes the 17-bit limb and stays below the largest one (asserted
    before the device runs), so gauss::reduce takes its remainder branch and its |z| < q branch in one launch."""
    import math
    import gauss_model as GM
    from alchemy_amd import encrypt as E
    from test_gpu_gauss import coset_buffer
    qs = GAUSS_RINGS[kind](rings(m))
    ring = make_ring(m, "MIX64" if kind == "MIX64" else "MIX31", qs)
    rad = math.prod(p for p, _ in GM.factor(m))
    svar = 2.0 * math.pi * GAUSS_SIGMA * GAUSS_SIGMA / float(m // rad)
    for i, p in enumerate(GAUSS_COSETS):
        seed, elem0 = 0xED6E0000 + 977 * m + i, ((1 << 64) - 2 if p == 7 else 5 * i)
        dst = ring.alloc(5)
        dst.fill_uniform(5)
        before = dst.download()
        cb = cw = None
        if p:
            zp, cb, cw = coset_buffer(m, p, 5, 60 + i)
        z = GM.gauss_dec(m, svar, seed, elem0, 3, p, cw[1:4] if p else None)
        zmax = int(np.abs(z).max())
        assert zmax < max(qs), (kind, p)
        if len(qs) > 1:
            assert zmax >= min(qs), (kind, p)                                # the small limb takes the remainder, the large one does not
        if p:
            assert np.array_equal(np.mod(z, p), cw[1:4])
        E.gauss_dec(dst, svar, seed, 1, 3, cb, 1, elem0)
        got = dst.download()
        assert_reduced(got, qs)
        assert np.array_equal(got[1:4], GM.words(z, qs)), (m, kind, p)
        assert np.array_equal(got[0], before[0]) and np.array_equal(got[4], before[4])
        del dst, cb
