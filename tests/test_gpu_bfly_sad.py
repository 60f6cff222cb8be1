"""GPU: the forward butterflies of 32-bit rings with the difference leg as one v_sad_u32 (modarith.hpp: bfly_fwd(u32...), bfly_fwd4),
on the smallest shapes that reach every kernel family that runs them, bit for bit against the oracle:

  * ct_mul_relin at n = 2^11, L = 4, 9 ciphertexts (k_ks_accum_half<11>: one full group of eight and a ragged one),
  * ct_mul_relin at n = 2^15, L = 4, 2 ciphertexts on the headline's moduli (k_ks_accum_half<15>, the benchmark's instantiation),
  * the same on the benchmark's four moduli below 2^30 (the Q30 instantiation: bfly_fwd4),
  * crt then crtInv of 4 polynomials at n = 2^15 (k_crt_half, and k_crt with option crt_half = 0) and at n = 2^10 (k_crt<10>),

each on uniform words, on all-zero words (every butterfly sees y = 0, so t = 0 and the leg returns xx + q) and on all-(q - 1) words.
The formulas themselves are compared word for word on the host by tests/test_bfly_sad.py."""
import numpy as np
import pytest

from conftest import CFG3_QS, Q30_QS
from helpers import assert_reduced

pytestmark = pytest.mark.gpu

FILLS = ["uniform", "zero", "q_minus_1"]


def _words(rng, fill, count, n, qs):
    if fill == "uniform":
        return np.ascontiguousarray(np.stack([rng.integers(0, q, size=(count, n), dtype=np.int64) for q in qs], axis=2))
    out = np.zeros((count, n, len(qs)), dtype=np.int64)
    if fill == "q_minus_1":
        out[:] = np.array(qs, dtype=np.int64) - 1
    return out


def _relin_case(oracle_lib, n, qs, batch, fill, seed):
    import alchemy_amd as A
    g, o = A.Ring(2 * n, qs), oracle_lib.Ring(n, qs)
    rng = np.random.default_rng(seed)
    hint, a, b = _words(rng, fill, 2 * len(qs), n, qs), _words(rng, fill, 2 * batch, n, qs), _words(rng, fill, 2 * batch, n, qs)
    gout = g.alloc(2 * batch)
    g.ct_mul_relin(g.hint_load(hint), g.upload(a), g.upload(b), gout, batch)
    got = gout.download()
    assert_reduced(got, qs)
    # all ciphertexts of a constant fill are equal: one oracle call serves them all
    want = {}
    for ct in range(batch):
        key = ct if fill == "uniform" else 0
        if key not in want:
            want[key] = o.ct_mul_relin(list(hint), a[2 * ct], a[2 * ct + 1], b[2 * ct], b[2 * ct + 1])
        w0, w1 = want[key]
        assert np.array_equal(got[2 * ct], w0), f"c0 mismatch ct {ct}"
        assert np.array_equal(got[2 * ct + 1], w1), f"c1 mismatch ct {ct}"


@pytest.mark.parametrize("fill", FILLS)
def test_mul_relin_n2048_nine_ciphertexts(oracle_lib, fill):
    _relin_case(oracle_lib, 1 << 11, CFG3_QS, 9, fill, seed=9400)


@pytest.mark.parametrize("fill", FILLS)
def test_mul_relin_headline_instantiation(oracle_lib, fill):
    _relin_case(oracle_lib, 1 << 15, CFG3_QS, 2, fill, seed=9410)


@pytest.mark.parametrize("fill", FILLS)
def test_mul_relin_moduli_below_2_30(oracle_lib, fill):
    _relin_case(oracle_lib, 1 << 15, Q30_QS[:4], 2, fill, seed=9420)


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("logn,half", [(15, 1), (15, 0), (10, None)], ids=["n32768_half", "n32768_whole", "n1024"])
def test_crt_then_crtinv(oracle_lib, logn, half, fill):
    import alchemy_amd as A
    n, qs = 1 << logn, CFG3_QS
    g, o = A.Ring(2 * n, qs), oracle_lib.Ring(n, qs)
    if half is not None:
        g.set_option("crt_half", half)
    x = _words(np.random.default_rng(9430 + logn), fill, 4, n, qs)
    buf = g.upload(x)
    buf.crt()
    got = buf.download()
    assert_reduced(got, qs)
    for e in range(4 if fill == "uniform" else 1):
        assert np.array_equal(got[e], o.crt(x[e])), f"crt mismatch elem {e}"
    if fill != "uniform":
        assert all(np.array_equal(got[e], got[0]) for e in range(1, 4))
    buf.crtinv()
    assert np.array_equal(buf.download(), x), "crtInv . crt != id"
