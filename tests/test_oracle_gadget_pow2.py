"""CPU: the test-side reference of the BaseBGad 2^w gadget (tests/gadget_pow2_ref.py) against the exact model
(oracle.model.decompose_baseb / gadget_baseb, stated for any base) and against helpers.decompose_base2 at w = 1; and the model's own
check that a hint built from gadget_baseb(qs, 2^w) key-switches x * y to a ciphertext that decrypts to the negacyclic product."""
import random

import numpy as np
import pytest

from gadget_pow2_ref import decompose_pow2, digit_counts, gadget_pow2, model_hint_pow2, model_key_switch_pow2
from helpers import decompose_base2, extreme_words, primes_1_mod, primes_below, to_aos

WIDTHS = list(range(1, 17))


def _rings():
    q31 = primes_below(32, 1, 1 << 31)[0]
    q62 = primes_below(32, 1, 1 << 62)[0]
    return [(16, [12289, 65537, q31]), (16, [65537, q62]), (6, primes_1_mod(9, 2, lo=1 << 20) + primes_below(9, 1, 1 << 31))]


@pytest.mark.parametrize("w", WIDTHS)
def test_decompose_pow2_equals_the_model(w):
    from oracle import model as M
    rng = np.random.default_rng(600 + w)
    for n, qs in _rings():
        for elem in extreme_words(rng, 2, n, qs):
            got = decompose_pow2(elem, qs, w)
            want = M.decompose_baseb([[int(x) for x in elem[:, i]] for i in range(len(qs))], qs, 1 << w)
            assert len(got) == len(want) == sum(digit_counts(qs, w)) == sum(M.baseb_digits(q, 1 << w) for q in qs)
            for g, d in zip(got, want):
                assert np.array_equal(g, np.stack([[x % q for x in d] for q in qs], axis=1))
        # the gadget: entry t of limb i is 2^(w t) on limb i
        assert [[pow(2, w * t, q) if j == i else 0 for j, q in enumerate(qs)] for i, t in gadget_pow2(qs, w)] == M.gadget_baseb(qs, 1 << w)
        assert all(1 << (w * (k - 1)) < q <= 1 << (w * k) for q, k in zip(qs, digit_counts(qs, w)))


def test_decompose_pow2_at_width_1_is_decompose_base2():
    rng = np.random.default_rng(77)
    for n, qs in _rings():
        for elem in extreme_words(rng, 3, n, qs):
            got, want = decompose_pow2(elem, qs, 1), decompose_base2(elem, qs)
            assert len(got) == len(want) and all(np.array_equal(g, d) for g, d in zip(got, want))


@pytest.mark.parametrize("w", [1, 3, 4, 8, 16])
def test_a_base_pow2_hint_key_switches_to_the_product_on_the_exact_model(w):
    from oracle import model as M
    rng = random.Random(5200 + w)
    n, npt, p = 64, 8, 7
    qs = primes_1_mod(2 * n, 2, lo=1 << 29)
    sk = M.gen_sk(n, 3.0, rng)
    pt1, pt2 = [rng.randrange(p) for _ in range(npt)], [rng.randrange(p) for _ in range(npt)]
    x, y = M.encrypt(sk, pt1, p, qs, 3.0, rng), M.encrypt(sk, pt2, p, qs, 3.0, rng)
    hint = model_hint_pow2(sk, qs, 3.0, rng, w)
    assert len(hint.h) == sum(digit_counts(qs, w))
    got = model_key_switch_pow2(hint, M.ct_mul(x, y), w)
    assert len(got.c) == 2 and M.decrypt(sk, got, npt) == M.negacyclic_mul(pt1, pt2, p)
    if w == 1:                                            # the model's own BaseBGad 2 path gives the same ciphertext
        hint.gadget = "base2"
        assert M.key_switch_quad_circ(hint, M.ct_mul(x, y)).c == got.c
