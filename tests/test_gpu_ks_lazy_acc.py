"""GPU: the lazy accumulators of the two-workgroup key-switch kernel (kernel_ks_half.hpp) on worst-case words.

The kernel keeps its accumulators in [0, 2q) for a whole work item (unreduced tensor values, one borrow-corrected subtraction per
hint product of the negated digit) and brings them to [0, q) only where it stores them.  Every case goes through the C ABI, is compared
bit for bit with the oracle and asserts that every output word is below its modulus.  Operands and hint rows are drawn from
{0, 1, q-2, q-1, (q-1)/2, (q+1)/2} mixed per word with uniform filler: the values at which a missing or doubled correction shows."""
import numpy as np
import pytest

from conftest import CFG3_QS
from helpers import assert_reduced as _assert_reduced, extreme_words as _worst, oracle_full_mul
from test_gpu_full_mul import SIX_QS
from test_gpu_parity import EIGHT_QS, UNBAL_QS

pytestmark = pytest.mark.gpu


def _relin_case(oracle_lib, n, qs, batch, seed, s_pre=None, diagonal_hint=False):
    import alchemy_amd as A
    g, o = A.Ring(2 * n, qs), oracle_lib.Ring(n, qs)
    L = len(qs)
    rng = np.random.default_rng(seed)
    hint = _worst(rng, 2 * L, n, qs)
    if diagonal_hint:                       # row (digit i, limb j) is zero unless i == j: no product ever touches the lazy tensor values
        for i in range(L):
            for j in range(L):
                if i != j:
                    hint[2 * i:2 * i + 2, :, j] = 0
    a, b = _worst(rng, 2 * batch, n, qs), _worst(rng, 2 * batch, n, qs)
    gout = g.alloc(2 * batch)
    g.ct_mul_relin(g.hint_load(hint), g.upload(a), g.upload(b), gout, batch, s_pre=s_pre)
    got = gout.download()
    _assert_reduced(got, qs)
    for ct in range(batch):
        w0, w1 = o.ct_mul_relin(list(hint), a[2 * ct], a[2 * ct + 1], b[2 * ct], b[2 * ct + 1], s_pre=s_pre)
        assert np.array_equal(got[2 * ct], w0), f"c0 mismatch ct {ct}"
        assert np.array_equal(got[2 * ct + 1], w1), f"c1 mismatch ct {ct}"


@pytest.mark.parametrize("minus_one", [False, True], ids=["s_default", "s_minus_one"])
@pytest.mark.parametrize("diagonal_hint", [False, True], ids=["full_hint", "diagonal_hint"])
def test_worst_case_words_n2048(oracle_lib, diagonal_hint, minus_one):
    """n = 2^11, four 31-bit limbs, batch 3 -- with every off-diagonal hint row zero the unreduced tensor values reach the store
    untouched, so the conditional subtraction there is all that stands between [0, 2q) and the caller."""
    s = [q - 1 for q in CFG3_QS] if minus_one else None
    _relin_case(oracle_lib, 1 << 11, CFG3_QS, 3, seed=9100 + 2 * diagonal_hint + minus_one, s_pre=s, diagonal_hint=diagonal_hint)


def test_worst_case_words_eight_limbs(oracle_lib):
    """Seven borrow-corrected subtractions per accumulator."""
    _relin_case(oracle_lib, 1 << 11, EIGHT_QS, 2, seed=9110)


def test_worst_case_words_unbalanced(oracle_lib):
    """The general digit reduce, by the negated Montgomery one."""
    _relin_case(oracle_lib, 1 << 11, UNBAL_QS, 2, seed=9120)


def test_worst_case_words_headline_instantiation(oracle_lib):
    """n = 2^15, the benchmark's ring."""
    _relin_case(oracle_lib, 1 << 15, CFG3_QS, 2, seed=9130)


def test_worst_case_words_full_mul_added_limb(oracle_lib):
    """alch_ct_mul_full, 4 -> 5 -> 3 limbs at n = 2^11 (built as tests/test_gpu_full_mul.py builds its cases): the added limb's
    accumulators start from zero, and the rescale that follows reads the key switch's stored words."""
    import alchemy_amd as A
    n, qs_h, l_in, l_out, batch = 1 << 11, SIX_QS[:5], 4, 3, 3
    L = len(qs_h)
    rng = np.random.default_rng(9140)
    rin, rh, rout = A.Ring(2 * n, qs_h[L - l_in:]), A.Ring(2 * n, qs_h), A.Ring(2 * n, qs_h[L - l_out:])
    hint = _worst(rng, 2 * L, n, qs_h)
    a, b = _worst(rng, 2 * batch, n, qs_h[L - l_in:]), _worst(rng, 2 * batch, n, qs_h[L - l_in:])
    gout = rout.alloc(2 * batch)
    A.capi.ct_mul_full(rh.hint_load(hint), rin.upload(a), rin.upload(b), gout, batch)
    got = gout.download()
    _assert_reduced(got, qs_h[L - l_out:])
    for ct in range(batch):
        w0, w1 = oracle_full_mul(oracle_lib, n, qs_h, l_in, l_out, list(hint), a[2 * ct], a[2 * ct + 1], b[2 * ct], b[2 * ct + 1])
        assert np.array_equal(got[2 * ct], w0), f"c0 mismatch ct {ct}"
        assert np.array_equal(got[2 * ct + 1], w1), f"c1 mismatch ct {ct}"
