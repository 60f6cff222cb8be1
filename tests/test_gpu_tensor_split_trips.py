"""GPU: the tensor kernel of the n = 2^15 headline (k_tensor_intt_split, kernel_tensor_split.hpp) with its 14 half-size stages run as
two stages in registers on load plus three LDS passes, and stage 0, the scaling, the centred lift and the digit stores straight out
of the last pass.

The kernel exists only at n = 2^15, so the small shapes are small batches: 1, 3 and 9 ciphertext pairs (nine gives more than one
item per limb residue and rotates the slice order through several values).  The operands pin the new code: a1 b1 = 0 in every slot
(neither operand zero), a1 b1 = q - 1 in every slot (every lazy value at the edge of its range through the on-load stages), and
uniform words.  One set of nine pairs and its oracle results are computed once per ring; the batches are its prefixes (a
ciphertext's result does not depend on the batch it runs in).  Every stored word is compared with the C restatement."""
import numpy as np
import pytest

from conftest import CFG3_QS, Q30_QS
from helpers import assert_reduced as _assert_reduced, oracle_full_mul
from test_gpu_full_mul import SIX_QS

pytestmark = pytest.mark.gpu

N = 1 << 15
KINDS = ["uniform", "zero", "edge"]          # ciphertext ct of a set has kind KINDS[ct % 3]: every prefix starts with a uniform pair


def _rand(rng, count, n, qs):
    return np.stack([np.stack([rng.integers(0, q, size=n, dtype=np.int64) for q in qs], axis=1) for _ in range(count)])


def _operands(rng, batch, n, qs):
    """a, b as (2 batch, n, L): a0, b0 uniform; a1, b1 by the ciphertext's kind."""
    a, b = _rand(rng, 2 * batch, n, qs), _rand(rng, 2 * batch, n, qs)
    qv = np.array(qs, dtype=np.int64)
    for ct in range(batch):
        kind = KINDS[ct % 3]
        if kind == "zero":                   # a1 vanishes on a random set of slots, b1 on the others
            mask = rng.integers(0, 2, size=(n, len(qs))).astype(bool)
            a[2 * ct + 1][mask] = 0
            b[2 * ct + 1][~mask] = 0
            assert not np.any((a[2 * ct + 1] != 0) & (b[2 * ct + 1] != 0))
        elif kind == "edge":                 # (q - 1) * 1 and 1 * (q - 1) in turn
            minus, one = np.broadcast_to(qv - 1, (n, len(qs))), np.ones((n, len(qs)), dtype=np.int64)
            a[2 * ct + 1], b[2 * ct + 1] = (minus, one) if (ct // 3) % 2 == 0 else (one, minus)
    return a, b


def _relin_set(oracle_lib, qs, seed):
    rng = np.random.default_rng(seed)
    hint = _rand(rng, 2 * len(qs), N, qs)
    a, b = _operands(rng, 9, N, qs)
    o = oracle_lib.Ring(N, qs)
    want = [o.ct_mul_relin(list(hint), a[2 * ct], a[2 * ct + 1], b[2 * ct], b[2 * ct + 1]) for ct in range(9)]
    for arr in (hint, a, b):
        arr.setflags(write=False)
    return hint, a, b, want


@pytest.fixture(scope="module")
def headline_set(oracle_lib):
    return _relin_set(oracle_lib, CFG3_QS, 9300)


@pytest.fixture(scope="module")
def q30_set(oracle_lib):
    return _relin_set(oracle_lib, Q30_QS[:4], 9301)


def _relin_prefix(qs, data, batch, q30=None):
    import alchemy_amd as A
    hint, a, b, want = data
    g = A.Ring(2 * N, qs)
    if q30 is not None:
        g.set_option("q30", q30)
    gout = g.alloc(2 * batch)
    g.ct_mul_relin(g.hint_load(hint), g.upload(a[:2 * batch]), g.upload(b[:2 * batch]), gout, batch)
    got = gout.download()
    _assert_reduced(got, qs)
    for ct in range(batch):
        assert np.array_equal(got[2 * ct], want[ct][0]), f"c0 mismatch ct {ct} ({KINDS[ct % 3]})"
        assert np.array_equal(got[2 * ct + 1], want[ct][1]), f"c1 mismatch ct {ct} ({KINDS[ct % 3]})"


@pytest.mark.parametrize("batch", [1, 3, 9])
def test_relin_headline_moduli(headline_set, batch):
    """The benchmark's four 31-bit moduli: the general instantiation."""
    _relin_prefix(CFG3_QS, headline_set, batch)


@pytest.mark.parametrize("batch", [1, 3, 9])
def test_relin_moduli_below_2_30(q30_set, batch):
    """The four moduli of the benchmark's line below 2^30: the Harvey-butterfly instantiation."""
    _relin_prefix(Q30_QS[:4], q30_set, batch, q30=1)


def test_full_mul_added_limb(oracle_lib):
    """alch_ct_mul_full, 4 -> 5 -> 3 limbs, batch 3 (uniform, zero, edge): the kernel also feeds the <UP> key switch, where digit i
    belongs to limb i + 1 of the hint's ring."""
    import alchemy_amd as A
    qs_h, l_in, l_out, batch = SIX_QS[:5], 4, 3, 3
    L = len(qs_h)
    qs_in = qs_h[L - l_in:]
    rng = np.random.default_rng(9302)
    rin, rh, rout = A.Ring(2 * N, qs_in), A.Ring(2 * N, qs_h), A.Ring(2 * N, qs_h[L - l_out:])
    hint = _rand(rng, 2 * L, N, qs_h)
    a, b = _operands(rng, batch, N, qs_in)
    gout = rout.alloc(2 * batch)
    A.capi.ct_mul_full(rh.hint_load(hint), rin.upload(a), rin.upload(b), gout, batch)
    got = gout.download()
    _assert_reduced(got, qs_h[L - l_out:])
    for ct in range(batch):
        w0, w1 = oracle_full_mul(oracle_lib, N, qs_h, l_in, l_out, list(hint), a[2 * ct], a[2 * ct + 1], b[2 * ct], b[2 * ct + 1])
        assert np.array_equal(got[2 * ct], w0), f"c0 mismatch ct {ct} ({KINDS[ct % 3]})"
        assert np.array_equal(got[2 * ct + 1], w1), f"c1 mismatch ct {ct} ({KINDS[ct % 3]})"
