"""GPU: the butterflies with Plantard twiddles (modarith.hpp: plant_mul3, the 7-instruction forward butterfly of the passes whose
twiddles a wave shares, the 8- / 12-instruction inverse butterflies of k_tensor_intt_split on values kept in [0, q]) on the smallest
shapes that reach every kernel family that reads a Plantard table or must NOT read one, bit for bit against the oracle:

  * ct_mul_relin at n = 2^11, L = 4, 9 ciphertexts (k_ks_accum_half<11>: stage 2 of pass G; one full group of eight and a ragged one),
  * ct_mul_relin at n = 2^15, L = 4, 2 ciphertexts on the headline's moduli (k_tensor_intt_split and k_ks_accum_half<15>, the
    benchmark's instantiations: inverse passes on [0, q], forward stage 2 and the wave-uniform LDS pass),
  * the same on the benchmark's four moduli below 2^30 (the Q30 instantiations, which keep the Montgomery table in every pass: a build
    that handed them two-word constants computed wrong results here),
  * ct_mul_full with a 5-limb hint at n = 2^11, 3 ciphertexts (k_ks_accum_half<UP>: the tables of a suffix ring),
  * crt then crtInv of 4 polynomials at n = 2^15 (k_crt_half, and k_crt with option crt_half = 0) and at n = 2^10 (k_crt<10>),
  * one ciphertext of ct_mul_relin at n = 2^16 on the benchmark's six moduli (the split kernels: half-size transforms with a prefix),

each on uniform words, on all-zero words (every twiddle product is 0, the one value a Plantard product may return as q) and on
all-(q - 1) words.  The formulas themselves are checked on the host by tests/test_plant3.py."""
import numpy as np
import pytest

from conftest import CFG3_QS, Q30_QS
from helpers import assert_reduced, oracle_full_mul

pytestmark = pytest.mark.gpu

FILLS = ["uniform", "zero", "q_minus_1"]
N16_QS = [2147352577, 2146959361, 2146041857, 2144468993, 2142502913, 2135818241]      # all = 1 mod 2^17
FULL_QS = [2144468993, 2147352577, 2146959361, 2146041857, 2145976321]                 # hint ring; operands on the last four


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
    _relin_case(oracle_lib, 1 << 11, CFG3_QS, 9, fill, seed=9500)


@pytest.mark.parametrize("fill", FILLS)
def test_mul_relin_headline_instantiation(oracle_lib, fill):
    _relin_case(oracle_lib, 1 << 15, CFG3_QS, 2, fill, seed=9510)


@pytest.mark.parametrize("fill", FILLS)
def test_mul_relin_moduli_below_2_30(oracle_lib, fill):
    _relin_case(oracle_lib, 1 << 15, Q30_QS[:4], 2, fill, seed=9520)


@pytest.mark.parametrize("fill", FILLS)
def test_mul_relin_n65536_six_moduli_one_ciphertext(oracle_lib, fill):
    _relin_case(oracle_lib, 1 << 16, N16_QS, 1, fill, seed=9530)


@pytest.mark.parametrize("fill", FILLS)
def test_mul_full_five_limb_hint_n2048(oracle_lib, fill):
    import alchemy_amd as A
    n, batch, qs_h = 1 << 11, 3, FULL_QS
    rin, rh, rout = A.Ring(2 * n, qs_h[1:]), A.Ring(2 * n, qs_h), A.Ring(2 * n, qs_h[2:])
    rng = np.random.default_rng(9540)
    hint, a, b = _words(rng, fill, 2 * len(qs_h), n, qs_h), _words(rng, fill, 2 * batch, n, qs_h[1:]), _words(rng, fill, 2 * batch, n, qs_h[1:])
    gout = rout.alloc(2 * batch)
    A.capi.ct_mul_full(rh.hint_load(hint), rin.upload(a), rin.upload(b), gout, batch)
    got = gout.download()
    assert_reduced(got, qs_h[2:])
    for ct in range(batch if fill == "uniform" else 1):
        w0, w1 = oracle_full_mul(oracle_lib, n, qs_h, 4, 3, list(hint), a[2 * ct], a[2 * ct + 1], b[2 * ct], b[2 * ct + 1])
        assert np.array_equal(got[2 * ct], w0), f"c0 mismatch ct {ct}"
        assert np.array_equal(got[2 * ct + 1], w1), f"c1 mismatch ct {ct}"
    if fill != "uniform":
        assert all(np.array_equal(got[2 * ct + c], got[c]) for ct in range(1, batch) for c in range(2))


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("logn,half", [(15, 1), (15, 0), (10, None)], ids=["n32768_half", "n32768_whole", "n1024"])
def test_crt_then_crtinv(oracle_lib, logn, half, fill):
    import alchemy_amd as A
    n, qs = 1 << logn, CFG3_QS
    g, o = A.Ring(2 * n, qs), oracle_lib.Ring(n, qs)
    if half is not None:
        g.set_option("crt_half", half)
    x = _words(np.random.default_rng(9550 + logn), fill, 4, n, qs)
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
