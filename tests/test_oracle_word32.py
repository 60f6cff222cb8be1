"""CPU: the C restatement (oracle/cref.py) against the by-definition model (oracle/model.py) at the moduli of
tests/test_gpu_word32_edges.py -- just below 2^31, on either side of 2^30, a 31-bit limb next to a 17-bit one, either side of the
balanced / unbalanced boundary for a 31-bit and a 30-bit qmax -- on words from helpers.extreme_words and on the two constant
elements.  The restatement's own 32-bit products are plain `%` on 64-bit values ((q-1)^2 < 2^62); this file is what entitles it to
judge the device kernels at these moduli.  It also checks, without a GPU, that every modulus of the GPU file lies in the class its
cases need."""
import numpy as np
import pytest

import test_gpu_word32_edges as W
from helpers import centred_extreme_words, decompose_base2, extreme_words, from_aos, oracle_full_mul, word32_edge_rings
from oracle import model as M

RINGS = {name: W.RINGS[name] for name in ("TOP5", "ABOVE30", "BELOW30", "STRADDLE30", "EDGE_BAL31", "EDGE_UNBAL31", "EDGE_BAL30",
                                          "EDGE_UNBAL30", "MIXED", "MIXED_LAST", "MIXED_FULL", "EIGHT_TOP", "TOP17", "BELOW30_17",
                                          "TOP_AND_17_BIT")}
RINGS["TOP6"] = W.TOP6
EDGE_FULL = {"edge31-bal": W.EDGE31_FULL["bal"], "edge31-unbal": W.EDGE31_FULL["unbal"],
             "edge30-bal": W.EDGE30_FULL["bal"], "edge30-unbal": W.EDGE30_FULL["unbal"]}


def test_the_moduli_lie_in_their_classes():
    W.test_the_moduli_are_where_the_cases_need_them()
    for q in W.ALL_MODULI:
        assert M.is_prime(q) and q < (1 << 31)                    # 4-byte words on every ring of the GPU file
    for name in ("TOP5", "EIGHT_TOP", "TOP17", "ABOVE30", "STRADDLE30", "EDGE_BAL31", "EDGE_UNBAL31", "MIXED", "MIXED_LAST", "MIXED_FULL"):
        assert max(W.RINGS[name]) > (1 << 30), name               # not q30: the non-Harvey kernels
    for q in W.TOP6 + W.ABOVE30:
        assert q > (1 << 30)
    for name in ("BELOW30", "EDGE_BAL30", "EDGE_UNBAL30", "BELOW30_17", "EDGE30_FULL_BAL", "EDGE30_FULL_UNBAL"):
        assert max(W.RINGS[name]) < (1 << 30), name               # q30
    for bal, unbal in ((W.EDGE_BAL31, W.EDGE_UNBAL31), (W.EDGE_BAL30, W.EDGE_UNBAL30)):
        assert bal[0] == unbal[0] == max(bal) == max(unbal)
        assert (bal[0] - 1) // 2 < bal[1] and (unbal[0] - 1) // 2 >= unbal[1]
        assert bal[1] - unbal[1] < 1 << 20
    # the class the sweeps draw from is built by the same rule
    assert word32_edge_rings(W.M16) == {"above30": W.ABOVE30, "straddle30": W.STRADDLE30, "edge_bal31": W.EDGE_BAL31,
                                        "edge_unbal31": W.EDGE_UNBAL31, "edge_bal30": W.EDGE_BAL30, "edge_unbal30": W.EDGE_UNBAL30}
    # sizes the GPU file runs them at
    for q in W.TOP6 + W.ABOVE30 + W.BELOW30 + W.MIXED + W.EDGE_BAL30 + W.EDGE_UNBAL30:
        assert q % (1 << 16) == 1
    for q in W.TOP17 + [W.BELOW30_17]:
        assert q % (1 << 17) == 1
    for q in W.EIGHT_TOP:
        assert q % (1 << 12) == 1


def test_digit_counts():
    for q in W.TOP6 + W.EIGHT_TOP + W.TOP17 + W.ABOVE30:
        assert M.baseb_digits(q) == 31 == (q - 1).bit_length()
    for q in W.BELOW30:
        assert M.baseb_digits(q) == 30
    assert M.baseb_digits(65537) == 17 and M.baseb_digits(786433) == 20


@pytest.mark.parametrize("n", [16, 64])
@pytest.mark.parametrize("name", list(RINGS))
def test_c_restatement_matches_the_model(oracle_lib, name, n):
    qs = RINGS[name]
    L = len(qs)
    o = oracle_lib.Ring(n, qs)
    rng = np.random.default_rng(3100 + n + L)
    x = np.concatenate([extreme_words(rng, 4, n, qs), W.constant_elements(n, qs)])
    # crt by direct evaluation, its inverse, pointwise products, the ring product -- extreme * extreme, extreme * constant, constant * constant
    crt = [o.crt(e) for e in x]
    for e in range(6):
        assert from_aos(crt[e]) == [M.crt_def(al, q) for al, q in zip(from_aos(x[e]), qs)], e
        assert np.array_equal(o.crtinv(crt[e]), x[e]), e
        assert from_aos(o.crtinv(x[e])) == [M.crtinv_def(al, q) for al, q in zip(from_aos(x[e]), qs)], e
    for i, j in ((0, 1), (0, 4), (1, 5), (4, 5), (4, 4)):
        a, b = from_aos(x[i]), from_aos(x[j])
        assert from_aos(o.mul(x[i], x[j])) == [[u * v % q for u, v in zip(al, bl)] for al, bl, q in zip(a, b, qs)]
        assert from_aos(o.crtinv(o.mul(crt[i], crt[j]))) == M.rns_mul(a, b, qs)
        assert from_aos(o.add(x[i], x[j])) == M.rns_add(a, b, qs)
        assert from_aos(o.sub(x[i], x[j])) == M.rns_add(a, M.rns_neg(b, qs), qs)
    for s in ([q - 1 for q in qs], [(q + 1) // 2 for q in qs], [q - 2 for q in qs]):
        for e in (0, 4, 5):
            assert from_aos(o.scale(x[e], s)) == M.rns_scale(from_aos(x[e]), s, qs)
    # gadget decompositions, reduced into every limb; the centred extremes put lifts at +-(q-1)/2
    y = centred_extreme_words(rng, 1, n, qs)[0]
    for e in (x[0], x[4], x[5], y):
        c = from_aos(e)
        for digs, want in ((o.decompose_triv(e), M.decompose_triv(c, qs)), (o.decompose_base2(e), M.decompose_baseb(c, qs, 2))):
            assert len(digs) == len(want)
            for d, w in zip(digs, want):
                assert from_aos(d) == M.rns_reduce(w, qs)
        for d, w in zip(decompose_base2(e, qs), o.decompose_base2(e)):           # the numpy form the tunnel oracle composes
            assert np.array_equal(d, w)
    # Rescale (a, b) -> b, one limb and down to one limb
    if L > 1:
        for e in (x[0], x[4], y):
            assert from_aos(o.rescale_drop0(e)) == M.rescale_down(from_aos(e), qs, 1)
            cur = e
            for drop in range(L - 1):
                cur = oracle_lib.Ring(n, qs[drop:]).rescale_drop0(cur)
            assert from_aos(cur) == M.rescale_down(from_aos(e), qs, L - 1)
    # keySwitchQuadCirc hint (a * b): the fused entry against its composition from the primitives checked above
    hint = extreme_words(rng, 2 * L, n, qs)
    s = [q - 1 for q in qs]
    for ops in ((x[0], x[1], x[2], x[3]), (x[0], x[4], x[5], x[4]), (x[2], crt[0] * 0 + 1, x[3], o.crt(y))):
        for s_pre in (None, s):
            for pow_basis in (False, True):
                w0, w1 = o.ct_mul_relin(list(hint), *ops, s_pre=s_pre, pow_basis=pow_basis)
                a0, a1, b0, b1 = [o.crt(e) for e in ops] if pow_basis else list(ops)
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


def _model_full_mul(qs_h, l_in, l_out, hint_pow, a0, a1, b0, b1, s):
    """PT2CT's mul_ on Pow-basis, limb-major operands from the model's definitions alone: (*) and the scalar, Rescale up, TrivGad key
    switch, Rescale down."""
    L = len(qs_h)
    qs_in = qs_h[L - l_in:]
    c = [M.rns_mul(a0, b0, qs_in), M.rns_add(M.rns_mul(a0, b1, qs_in), M.rns_mul(a1, b0, qs_in), qs_in), M.rns_mul(a1, b1, qs_in)]
    c = [M.rescale_up(M.rns_scale(e, s, qs_in), qs_in, qs_h[:L - l_in]) for e in c]
    digs = M.decompose_triv(c[2], qs_h)
    assert len(digs) == L
    out = []
    for k in range(2):
        acc = c[k]
        for i, d in enumerate(digs):
            acc = M.rns_add(acc, M.rns_mul(M.rns_reduce(d, qs_h), hint_pow[2 * i + k], qs_h), qs_h)
        out.append(M.rescale_down(acc, qs_h, L - l_out))
    return out


@pytest.mark.parametrize("minus_one", [False, True], ids=["plus_x", "minus_x"])
@pytest.mark.parametrize("n", [16, 64])
@pytest.mark.parametrize("name", list(EDGE_FULL))
def test_oracle_full_mul_matches_the_model_on_the_edge_rings(oracle_lib, name, n, minus_one):
    """helpers.oracle_full_mul, 2 -> 3 -> 1 limbs on each EDGE pair behind one added limb, against the model: on extreme operands and
    an extreme hint, and on the operands of the GPU file's rescale-at-the-ends cases (whose construction checks run here as well)."""
    qs_h, l_in, l_out = EDGE_FULL[name], 2, 1
    qs_in = qs_h[1:]
    o_in, o_h = oracle_lib.Ring(n, qs_in), oracle_lib.Ring(n, qs_h)
    rng = np.random.default_rng(3150 + n + minus_one)
    hint = extreme_words(rng, 2 * len(qs_h), n, qs_h)
    ops = extreme_words(rng, 4, n, qs_in)
    s_pre = [q - 1 for q in qs_in] if minus_one else [1] * l_in
    w = oracle_full_mul(oracle_lib, n, qs_h, l_in, l_out, [o_h.crt(h) for h in hint], *[o_in.crt(e) for e in ops], s_pre=s_pre, pow_out=True)
    want = _model_full_mul(qs_h, l_in, l_out, [from_aos(h) for h in hint], *[from_aos(e) for e in ops], s_pre)
    assert [from_aos(w[0]), from_aos(w[1])] == want
    hint0, a, b, s_end, res = W.rescale_at_the_ends_case(oracle_lib, n, qs_h, l_in, l_out, 3, 3160 + n, minus_one)
    for ct in range(3):
        ops = [from_aos(o_in.crtinv(e)) for e in (a[2 * ct], a[2 * ct + 1], b[2 * ct], b[2 * ct + 1])]
        want = _model_full_mul(qs_h, l_in, l_out, [from_aos(h) for h in hint0], *ops, s_end)
        assert [from_aos(res[True][ct][0]), from_aos(res[True][ct][1])] == want, ct
        o_out = oracle_lib.Ring(n, qs_h[2:])
        assert [from_aos(o_out.crtinv(res[False][ct][k])) for k in range(2)] == want, ct


@pytest.mark.parametrize("minus_one", [False, True], ids=["s_default", "s_minus_one"])
@pytest.mark.parametrize("name", W.ENDS_RINGS)
def test_the_digits_at_the_ends_construction(oracle_lib, name, minus_one):
    """The construction checks of the GPU file's digits-at-the-ends cases, at n = 64: c2 = +-x, and the digits reach past another
    limb's modulus exactly on the unbalanced rings.  The oracle's result is compared with the model's key switch."""
    n, qs = 64, W.RINGS[name]
    o = oracle_lib.Ring(n, qs)
    hint, a, b, s_pre, want = W.digits_at_the_ends_case(oracle_lib, n, qs, 2, 3170 + minus_one, minus_one)
    s = s_pre if s_pre is not None else [1] * len(qs)
    hint_pow = [from_aos(o.crtinv(h)) for h in hint]
    for ct in range(2):
        a0, a1, b0, b1 = [from_aos(o.crtinv(e)) for e in (a[2 * ct], a[2 * ct + 1], b[2 * ct], b[2 * ct + 1])]
        c = [M.rns_mul(a0, b0, qs), M.rns_add(M.rns_mul(a0, b1, qs), M.rns_mul(a1, b0, qs), qs), M.rns_mul(a1, b1, qs)]
        c = [M.rns_scale(e, s, qs) for e in c]
        for k in range(2):
            acc = c[k]
            for i, d in enumerate(M.decompose_triv(c[2], qs)):
                acc = M.rns_add(acc, M.rns_mul(M.rns_reduce(d, qs), hint_pow[2 * i + k], qs), qs)
            assert from_aos(o.crtinv(want[ct][k])) == acc, (ct, k)
