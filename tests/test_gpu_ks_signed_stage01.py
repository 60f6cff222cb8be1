"""GPU: stages 0-1 of the two-workgroup key-switch kernel's pass G as one signed sum over the centred digits
(kernel_ks_half.hpp, stage01_signed in modarith.hpp), with digits that sit on the extremes of the centred range.

The kernel multiplies the TrivGad digits -- centred lifts, |z| <= (q_i - 1)/2 -- by centred constants and reduces four products at
once; the headroom argument is tight exactly where |z| is largest.  The digits are driven through the public entry points: with
a1 = crt(1) and b1 = crt(x) the quadratic coefficient is c2 = s x, so for s = 1 and s = -1 its Pow-basis coefficients are x and -x
and the digits are their centred lifts.  x is drawn per coefficient from {0, 1, q-1, (q-1)/2, (q+1)/2, (q-3)/2} (centred: 0, 1, -1,
the largest positive digit, the most negative one, the second largest) with uniform filler; the other operands and the hint rows
come from the same sets.  Every case is compared bit for bit with the oracle and every stored word must be below its modulus."""
import numpy as np
import pytest

from conftest import CFG3_QS, Q30_QS
from helpers import assert_reduced as _assert_reduced, centred_extreme_words as _extreme, oracle_full_mul
from test_gpu_full_mul import SIX_QS
from test_gpu_parity import EIGHT_QS, UNBAL_QS

pytestmark = pytest.mark.gpu


def _operands(rng, orc, batch, n, qs):
    """a = (a0, crt(1)), b = (b0, crt(x)) per ciphertext pair; returns a, b as (2 batch, n, L) and the Pow-basis x."""
    one = np.zeros((n, len(qs)), dtype=np.int64)
    one[0, :] = 1
    one_crt = orc.crt(one)
    assert np.all(one_crt == 1)
    a, b = _extreme(rng, 2 * batch, n, qs), _extreme(rng, 2 * batch, n, qs)
    x = _extreme(rng, batch, n, qs)
    for ct in range(batch):
        a[2 * ct + 1] = one_crt
        b[2 * ct + 1] = orc.crt(x[ct])
    return a, b, x


def _relin_case(oracle_lib, n, qs, batch, seed, minus_one=False, q30=None):
    import alchemy_amd as A
    g, o = A.Ring(2 * n, qs), oracle_lib.Ring(n, qs)
    if q30 is not None:
        g.set_option("q30", q30)
    L = len(qs)
    rng = np.random.default_rng(seed)
    hint = _extreme(rng, 2 * L, n, qs)
    a, b, x = _operands(rng, o, batch, n, qs)
    s_pre = [q - 1 for q in qs] if minus_one else None
    # the digits the kernel will read: crtInv(a1 b1 s) = +-x, so their centred lifts reach both ends of the range
    for ct in range(batch):
        c2 = o.crtinv(o.scale(o.mul(a[2 * ct + 1], b[2 * ct + 1]), s_pre if s_pre else [1] * L))
        want = np.mod(-x[ct], np.array(qs, dtype=np.int64)) if minus_one else x[ct]
        assert np.array_equal(c2, want), f"ct {ct}: the digits are not the centred lifts of +-x"
    gout = g.alloc(2 * batch)
    g.ct_mul_relin(g.hint_load(hint), g.upload(a), g.upload(b), gout, batch, s_pre=s_pre)
    got = gout.download()
    _assert_reduced(got, qs)
    for ct in range(batch):
        w0, w1 = o.ct_mul_relin(list(hint), a[2 * ct], a[2 * ct + 1], b[2 * ct], b[2 * ct + 1], s_pre=s_pre)
        assert np.array_equal(got[2 * ct], w0), f"c0 mismatch ct {ct}"
        assert np.array_equal(got[2 * ct + 1], w1), f"c1 mismatch ct {ct}"


@pytest.mark.parametrize("minus_one", [False, True], ids=["s_default", "s_minus_one"])
def test_extreme_digits_headline_moduli_n2048(oracle_lib, minus_one):
    """n = 2^11, batch 3: the smallest size the kernel is instantiated at, the headline's four 31-bit moduli."""
    _relin_case(oracle_lib, 1 << 11, CFG3_QS, 3, seed=9200 + minus_one, minus_one=minus_one)


@pytest.mark.parametrize("minus_one", [False, True], ids=["s_default", "s_minus_one"])
def test_extreme_digits_eight_limbs(oracle_lib, minus_one):
    """Seven digit transforms per limb, each from another modulus' centred range."""
    _relin_case(oracle_lib, 1 << 11, EIGHT_QS, 2, seed=9210 + minus_one, minus_one=minus_one)


@pytest.mark.parametrize("minus_one", [False, True], ids=["s_default", "s_minus_one"])
def test_extreme_digits_unbalanced(oracle_lib, minus_one):
    """A digit of the 31-bit limb is far larger than the small limbs' moduli: the signed products take it unreduced."""
    _relin_case(oracle_lib, 1 << 11, UNBAL_QS, 2, seed=9220 + minus_one, minus_one=minus_one)


@pytest.mark.parametrize("q30", [1, 0], ids=["q30_on", "q30_off"])
@pytest.mark.parametrize("minus_one", [False, True], ids=["s_default", "s_minus_one"])
def test_extreme_digits_moduli_below_2_30(oracle_lib, minus_one, q30):
    """Four moduli below 2^30 through the Harvey-butterfly instantiation (positive digit, outputs taken as [0,4q) values) and,
    with option q30 = 0, through the general one."""
    _relin_case(oracle_lib, 1 << 11, Q30_QS[:4], 2, seed=9230 + minus_one, minus_one=minus_one, q30=q30)


def test_extreme_digits_headline_instantiation(oracle_lib):
    """n = 2^15, batch 2: the benchmark's instantiation."""
    _relin_case(oracle_lib, 1 << 15, CFG3_QS, 2, seed=9240, minus_one=True)


@pytest.mark.parametrize("minus_one", [False, True], ids=["s_default", "s_minus_one"])
def test_extreme_digits_full_mul_added_limb(oracle_lib, minus_one):
    """alch_ct_mul_full, 4 -> 5 -> 3 limbs at n = 2^11: the <UP> instantiation, whose added limb has a zero diagonal digit and
    transforms all four digits.  modSwitch up multiplies c2 by the added modulus; s_pre = +-(that modulus)^-1 takes it out again,
    so the digits are the centred lifts of +-x here too."""
    import alchemy_amd as A
    n, qs_h, l_in, l_out, batch = 1 << 11, SIX_QS[:5], 4, 3, 3
    L = len(qs_h)
    qs_in = qs_h[L - l_in:]
    rng = np.random.default_rng(9250 + minus_one)
    rin, rh, rout = A.Ring(2 * n, qs_in), A.Ring(2 * n, qs_h), A.Ring(2 * n, qs_h[L - l_out:])
    hint = _extreme(rng, 2 * L, n, qs_h)
    a, b, _ = _operands(rng, oracle_lib.Ring(n, qs_in), batch, n, qs_in)
    s_pre = [pow(qs_h[0], -1, q) for q in qs_in]
    if minus_one:
        s_pre = [q - s for s, q in zip(s_pre, qs_in)]
    gout = rout.alloc(2 * batch)
    A.capi.ct_mul_full(rh.hint_load(hint), rin.upload(a), rin.upload(b), gout, batch, s_pre=s_pre)
    got = gout.download()
    _assert_reduced(got, qs_h[L - l_out:])
    for ct in range(batch):
        w0, w1 = oracle_full_mul(oracle_lib, n, qs_h, l_in, l_out, list(hint), a[2 * ct], a[2 * ct + 1], b[2 * ct], b[2 * ct + 1],
                                 s_pre=s_pre)
        assert np.array_equal(got[2 * ct], w0), f"c0 mismatch ct {ct}"
        assert np.array_equal(got[2 * ct + 1], w1), f"c1 mismatch ct {ct}"
