"""CPU: the C restatement (oracle/cref.py) against the by-definition model (oracle/model.py, oracle/model_gen.py) at the moduli of
tests/test_gpu_word64_edges.py -- just below 2^62, just above 2^31, a 62-bit limb next to a 17-bit one, either side of the
balanced / unbalanced boundary -- on words from helpers.extreme_words.  This is what makes the restatement a valid judge of the
device kernels at 62 bits: its own products are 128-bit, and nothing else in the suite runs it above 2^60."""
import numpy as np
import pytest

import test_gpu_word64_edges as W
from helpers import decompose_base2, extreme_words, from_aos, to_aos
from oracle import model as M
from oracle import model_gen as G

RINGS = {"TOP3": W.TOP3, "LOW2": W.LOW2, "MIXED": W.MIXED, "MIXED_LAST": W.MIXED_LAST, "EDGE_BAL": W.EDGE_BAL, "EDGE_UNBAL": W.EDGE_UNBAL,
         "EIGHT_TOP": W.EIGHT_TOP, "TOP5": W.TOP5, "MIXED_FULL": W.MIXED_FULL, "TUNNEL_TOP2": W.TUNNEL_TOP2}


def test_digit_counts():
    for q in W.TOP5 + W.EIGHT_TOP + W.TUNNEL_TOP2:
        assert M.baseb_digits(q) == 62 == (q - 1).bit_length()
    for q in W.LOW2:
        assert M.baseb_digits(q) == 32
    assert M.baseb_digits(65537) == 17


@pytest.mark.parametrize("n", [16, 64])
@pytest.mark.parametrize("name", list(RINGS))
def test_c_restatement_matches_the_model(oracle_lib, name, n):
    qs = RINGS[name]
    L = len(qs)
    o = oracle_lib.Ring(n, qs)
    rng = np.random.default_rng(6100 + n + L)
    x = extreme_words(rng, 4, n, qs)
    a, b = from_aos(x[0]), from_aos(x[1])
    # crt by direct evaluation, its inverse, pointwise products, the ring product
    ca, cb = o.crt(x[0]), o.crt(x[1])
    assert from_aos(ca) == [M.crt_def(al, q) for al, q in zip(a, qs)]
    assert np.array_equal(o.crtinv(ca), x[0])
    assert from_aos(o.mul(x[0], x[1])) == [[u * v % q for u, v in zip(al, bl)] for al, bl, q in zip(a, b, qs)]
    assert from_aos(o.crtinv(o.mul(ca, cb))) == M.rns_mul(a, b, qs)
    assert from_aos(o.add(x[0], x[1])) == M.rns_add(a, b, qs)
    assert from_aos(o.sub(x[0], x[1])) == M.rns_add(a, M.rns_neg(b, qs), qs)
    s = [q - 1 for q in qs]
    assert from_aos(o.scale(x[0], s)) == M.rns_scale(a, s, qs)
    # gadget decompositions, reduced into every limb
    for e in range(2):
        c = from_aos(x[e])
        for digs, want in ((o.decompose_triv(x[e]), M.decompose_triv(c, qs)), (o.decompose_base2(x[e]), M.decompose_baseb(c, qs, 2))):
            assert len(digs) == len(want)
            for d, w in zip(digs, want):
                assert from_aos(d) == M.rns_reduce(w, qs)
        for d, w in zip(decompose_base2(x[e], qs), o.decompose_base2(x[e])):           # the numpy form the tunnel oracle composes
            assert np.array_equal(d, w)
    # Rescale (a, b) -> b
    if L > 1:
        assert from_aos(o.rescale_drop0(x[0])) == M.rescale_down(a, qs, 1)
        cur = x[1]
        for drop in range(L - 1):
            cur = oracle_lib.Ring(n, qs[drop:]).rescale_drop0(cur)
        assert from_aos(cur) == M.rescale_down(b, qs, L - 1)
    # keySwitchQuadCirc hint (a * b): the fused entry against its composition from the primitives checked above
    hint = extreme_words(rng, 2 * L, n, qs)
    for s_pre in (None, s):
        for pow_basis in (False, True):
            w0, w1 = o.ct_mul_relin(list(hint), x[0], x[1], x[2], x[3], s_pre=s_pre, pow_basis=pow_basis)
            a0, a1, b0, b1 = [o.crt(e) for e in x] if pow_basis else list(x)
            sc = s_pre if s_pre is not None else [1] * L
            c0 = o.scale(o.mul(a0, b0), sc)
            c1 = o.scale(o.add(o.mul(a0, b1), o.mul(a1, b0)), sc)
            c2 = o.scale(o.mul(a1, b1), sc)
            for i, d in enumerate(o.decompose_triv(o.crtinv(c2))):
                dc = o.crt(d)
                c0 = o.add(c0, o.mul(dc, hint[2 * i]))
                c1 = o.add(c1, o.mul(dc, hint[2 * i + 1]))
            if pow_basis:
                c0, c1 = o.crtinv(c0), o.crtinv(c1)
            assert np.array_equal(w0, c0) and np.array_equal(w1, c1), (s_pre is None, pow_basis)


@pytest.mark.parametrize("mixed", [False, True], ids=["top2", "mixed"])
@pytest.mark.parametrize("m", W.GEN_M)
def test_general_c_restatement_matches_the_model(oracle_lib, m, mixed):
    """The general-index restatement at 62 bits: m = 33 against every definition, m = 1820 (n = 576) on crt as the Kronecker product
    of the per-axis definitions and the homomorphism / inverse properties."""
    qs = [W.GEN_TOP2[m][0], W.GEN_SMALL[m]] if mixed else W.GEN_TOP2[m]
    idx = G.Index(m)
    R = oracle_lib.GenRing(m, qs)
    assert R.n == idx.n and R.has_crt
    x = extreme_words(np.random.default_rng(6150 + m), 2, idx.n, qs)
    a = from_aos(x[0])
    ca, cb = R.crt(x[0]), R.crt(x[1])
    assert from_aos(ca) == [G.crt_kron(al, idx, q) for al, q in zip(a, qs)]      # Python integers (crt_def multiplies in uint64: q < 2^32)
    assert np.array_equal(R.crtinv(ca), x[0])
    assert np.array_equal(R.crt(R.mulg_pow(x[0])), R.mulg_crt(ca))
    assert np.array_equal(R.divg_pow(R.mulg_pow(x[0])), x[0]) and np.array_equal(R.divg_dec(R.mulg_dec(x[0])), x[0])
    assert np.array_equal(R.divg_crt(R.mulg_crt(ca)), ca)
    assert np.array_equal(R.l(R.linv(x[0])), x[0])
    if m < 100:
        b = from_aos(x[1])
        assert from_aos(R.crtinv(R.mul(ca, cb))) == [G.ring_mul_def(al, bl, idx, q) for al, bl, q in zip(a, b, qs)]
        for cname, fn in (("l", G.l_def), ("linv", G.linv_def), ("mulg_pow", G.mulg_pow_def), ("mulg_dec", G.mulg_dec_def),
                          ("divg_pow", G.divg_pow_def), ("divg_dec", G.divg_dec_def)):
            assert from_aos(getattr(R, cname)(x[0])) == [fn(al, idx, q) for al, q in zip(a, qs)], cname
        assert from_aos(R.mulg_crt(x[0])) == [[u * v % q for u, v in zip(G.g_crt(idx, q), al)] for al, q in zip(a, qs)]
        assert from_aos(R.rescale_drop0(x[0])) == M.rescale_down(a, qs, 1)
