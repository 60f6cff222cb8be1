"""CPU: the C restatement (oracle/cref.py) against the by-definition model (oracle/model.py) on exactly the rings and shapes of
tests/test_gpu_item_walks.py -- one to eight limbs on the largest primes below 2^31 and below 2^30, a 31-bit / 30-bit limb next to a
17-bit and a 20-bit one, eight-limb hints, and mul_ at 4 -> 5 -> 3, 7 -> 8 -> 5, 3 -> 4 -> 1 and 4 -> 5 -> 4 limbs -- at n = 2^4 .. 2^6, on
the GPU file's own operand draw (ciphertexts and hint elements alternating between uniform and extreme words).  The restatement had
never run on TOP8[4:], B30_8[5:], an eight-limb hint or a three-limb drop; this file is what entitles it to judge the device kernels
there.  It also checks, without a GPU, that every ring of the GPU file lies in the class its cases claim."""
import numpy as np
import pytest

import test_gpu_item_walks as IW
from helpers import from_aos, oracle_full_mul
from oracle import model as M
from test_oracle_word32 import _model_full_mul

SIZES = [16, 32, 64]


def test_the_rings_lie_in_their_classes():
    IW.test_the_moduli_are_where_the_cases_need_them()
    for q in IW.TOP8 + IW.B30_8 + IW.SMALL + IW.TOP17_8:
        assert M.is_prime(q) and q < (1 << 31)                    # 4-byte words on every ring of the GPU file
    for q in IW.TOP8 + IW.TOP17_8:
        assert q > (1 << 30)
    for name, (qs, bal, q30) in IW.RELIN_RINGS.items():
        assert ((max(qs) - 1) // 2 < min(qs)) == bal and all(q < (1 << 30) for q in qs) == q30, name
        assert all(q % (1 << 16) == 1 for q in qs), name
    for name, (qs_h, l_in, l_out, _, bal, q30, sizes) in IW.FULL_ROWS.items():
        assert ((max(qs_h) - 1) // 2 < min(qs_h)) == bal and all(q < (1 << 30) for q in qs_h) == q30, name
        assert all(q % (1 << 16) == 1 for q in qs_h) and set(sizes) <= {11, 15}, name
    # the closing modSwitch every row claims, by the dispatch's rule restated in the GPU file (the source text it pins is read there)
    for name, (k11, k15, ddn, lo) in IW.FULL_REACHES.items():
        qs_h, _, l_out, opts, _, _, sizes = IW.FULL_ROWS[name]
        assert (len(qs_h) - l_out, l_out) == (ddn, lo), name
        for logn in sizes:
            assert IW.rescale_kernel(logn, qs_h, l_out, opts) == (k15 if logn == 15 else k11), (name, logn)
    # every limb count of 1, 2, 3, 5, 8 and both Harvey rings; ks_map = 1 is served at L | 8 and must be ignored at 3 and 5
    assert {len(v[0]) for v in IW.RELIN_RINGS.values()} == {1, 2, 3, 5, 8}
    # every walk the GPU file asks for is at least three items long, ti_split = 7 at L = 1 and 2 excepted (its stand-in follows it)
    for logn in (11, 15):
        for name, (qs, _, _) in IW.RELIN_RINGS.items():
            sets = IW.relin_option_sets(logn, len(qs), IW.BATCH)
            assert sets[0] == ({}, False) and sum(both for _, both in sets) == 1
            for opts, _ in sets:
                IW.assert_walks(opts, IW.BATCH, len(qs), logn)
            if logn == 15:
                walks = [o["ti_split"] for o, _ in sets if "ti_split" in o and o.get("walk", True)]
                assert len(walks) == 1 and 3 * walks[0] <= 9 * len(qs) and (walks[0] == 7 or len(qs) <= 2)
                assert any(o.get("ti_split") == 7 for o, _ in sets)


def _model_relin(qs, hint_pow, a0, a1, b0, b1, s):
    """keySwitchQuadCirc hint (a * b) on Pow-basis, limb-major operands from the model's definitions alone."""
    c = [M.rns_mul(a0, b0, qs), M.rns_add(M.rns_mul(a0, b1, qs), M.rns_mul(a1, b0, qs), qs), M.rns_mul(a1, b1, qs)]
    c = [M.rns_scale(e, s, qs) for e in c]
    digs = M.decompose_triv(c[2], qs)
    assert len(digs) == len(qs)
    out = []
    for k in range(2):
        acc = c[k]
        for i, d in enumerate(digs):
            acc = M.rns_add(acc, M.rns_mul(M.rns_reduce(d, qs), hint_pow[2 * i + k], qs), qs)
        out.append(acc)
    return out


RELIN_CASES = [(name, qs) for name, (qs, _, _) in IW.RELIN_RINGS.items()] + list(IW.SPLIT_RINGS.items())


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name,qs", RELIN_CASES, ids=[c[0] for c in RELIN_CASES])
def test_ct_mul_relin_matches_the_model(oracle_lib, name, qs, n):
    """The transforms by direct evaluation and the fused key switch against the model's, on the operand draw of the GPU file: an
    even (uniform) and an odd (extreme) ciphertext, with s_pre = 1 and -1."""
    L = len(qs)
    o = oracle_lib.Ring(n, qs)
    rng = np.random.default_rng(6000 + n + L)
    hint = IW.alternating_words(rng, 2 * L, 1, n, qs)
    a, b = IW.alternating_words(rng, 2, 2, n, qs), IW.alternating_words(rng, 2, 2, n, qs)
    IW.assert_distinct(a, b, 2)
    for e in (a[0], a[3], hint[1]):
        assert from_aos(o.crt(e)) == [M.crt_def(al, q) for al, q in zip(from_aos(e), qs)]
        assert from_aos(o.crtinv(e)) == [M.crtinv_def(al, q) for al, q in zip(from_aos(e), qs)]
    hint_pow = [from_aos(o.crtinv(h)) for h in hint]
    for ct in range(2):
        ops = (a[2 * ct], a[2 * ct + 1], b[2 * ct], b[2 * ct + 1])
        pow_ops = [from_aos(o.crtinv(e)) for e in ops]
        for s in ([1] * L, [q - 1 for q in qs]):
            w = o.ct_mul_relin(list(hint), *ops, s_pre=s)
            assert [from_aos(o.crtinv(w[0])), from_aos(o.crtinv(w[1]))] == _model_relin(qs, hint_pow, *pow_ops, s), (ct, s[0])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("row", list(IW.FULL_ROWS))
def test_oracle_full_mul_matches_the_model(oracle_lib, row, n):
    """helpers.oracle_full_mul at the shapes of the GPU file's full-multiply rows (eight-limb hint, three-limb drops, a drop down to
    one limb) against the model: modSwitch up, TrivGad key switch, modSwitch down."""
    qs_h, l_in, l_out = IW.FULL_ROWS[row][:3]
    L = len(qs_h)
    qs_in, qs_out = qs_h[L - l_in:], qs_h[L - l_out:]
    o_in, o_h, o_out = oracle_lib.Ring(n, qs_in), oracle_lib.Ring(n, qs_h), oracle_lib.Ring(n, qs_out)
    rng = np.random.default_rng(6050 + n + 4 * L + l_out)
    hint = IW.alternating_words(rng, 2 * L, 1, n, qs_h)
    a, b = IW.alternating_words(rng, 2, 2, n, qs_in), IW.alternating_words(rng, 2, 2, n, qs_in)
    hint_pow = [from_aos(o_h.crtinv(h)) for h in hint]
    for ct in range(2):
        ops = (a[2 * ct], a[2 * ct + 1], b[2 * ct], b[2 * ct + 1])
        pow_ops = [from_aos(o_in.crtinv(e)) for e in ops]
        for s in ([1] * l_in, [q - 1 for q in qs_in]):
            want = _model_full_mul(qs_h, l_in, l_out, hint_pow, *pow_ops, s)
            w = oracle_full_mul(oracle_lib, n, qs_h, l_in, l_out, list(hint), *ops, s_pre=s)
            assert [from_aos(o_out.crtinv(w[0])), from_aos(o_out.crtinv(w[1]))] == want, (ct, s[0])
            wp = oracle_full_mul(oracle_lib, n, qs_h, l_in, l_out, list(hint), *ops, s_pre=s, pow_out=True)
            assert [from_aos(wp[0]), from_aos(wp[1])] == want, (ct, s[0])
