"""CPU: the references of tests/test_gpu_resident_edges.py at the moduli of that file, so that a mismatch on the device points at the
kernel.  The C restatement's mul, sub, add, scale, crt and crtInv (oracle/cref.py: what check_ct_encrypt and the decrypt rows compare
with) on helpers.extreme_words against Python integers and the by-definition transform of oracle/model_gen.py, on every ring of the
GPU file at m' = 45 and 64; the model's twaceCRT / embedCRT against crt of twacePowDec / embedPow at the top of both word sizes (above
2^32 crt_def leaves numpy for Python integers: a product of two residues no longer fits 64 bits); the reduction of
tests/gauss_model.py at 62-bit moduli; and the assertions on the moduli themselves, which need no ring.  Class 2 of
tests/test_gpu_word32_thresholds.py is checked against its thresholds here as tests/test_lazy_sums_host.py checks classes 3 .. 11."""
import numpy as np
import pytest

import test_gpu_resident_edges as R
from helpers import (check_resident_edge_rings, extreme_words, from_aos, group_class_primes, lazy_group, resident_edge_rings, to_aos,
                     word32_edge_rings)
from oracle import model_gen as G
from oracle.model import is_prime


def test_the_moduli_lie_in_their_classes():
    R.check_the_moduli()
    for m in R.INDICES:
        r = resident_edge_rings(m)
        check_resident_edge_rings(r)
        assert all(is_prime(q) and q % m == 1 for qs in r.values() for q in qs), m
        assert r["EDGE_BAL31"] == word32_edge_rings(m)["edge_bal31"] and r["EDGE_UNBAL31"] == word32_edge_rings(m)["edge_unbal31"]
    r = resident_edge_rings(1 << 16)                               # the 62-bit EDGE pair follows the rule of tests/test_gpu_word64_edges.py
    import test_gpu_word64_edges as W
    assert (r["EDGE_BAL62"], r["EDGE_UNBAL62"], r["TOP62"]) == (W.EDGE_BAL, W.EDGE_UNBAL, W.TOP3[:2])
    for name, digits in R.BASE2_DIGITS.items():
        for m in R.RLWE_M:
            assert sum((q - 1).bit_length() for q in resident_edge_rings(m)[name]) == digits
    assert {name for _, name in R.ADD_CASES} == set(R.ALL_RINGS)


def test_class_2_of_the_threshold_file_sits_next_to_its_thresholds():
    import test_gpu_word32_thresholds as TW
    near, u32 = 1 << 18, (1 << 32) - 1
    assert TW.TUNNEL_CLASSES == [2] + TW.CLASSES and TW.CLASS_K[2] == 0
    for m in TW.TP_MODULI + TW.GEN_MODULI + TW.PT_MODULI:
        top, bottom = group_class_primes(m, 2)
        assert top % m == 1 and bottom % m == 1 and top < (1 << 31)
        assert 0 <= u32 // 2 - top < near and 0 < bottom - u32 // 3 < near, m
        assert u32 // top == 2 == u32 // bottom and lazy_group(top) == lazy_group(bottom) == 0
        assert 2 * top < (1 << 32) <= 3 * bottom
    assert u32 // 1543651201 == 2                                  # the reference's own moduli are of this class
    import math
    cases = [(max(TW.TP_PAIRS[d]), L) for kmax, d, L in TW.TP_CASES if kmax == 2]
    cases += [(math.lcm(*TW.GEN_PAIRS[d]), L) for kmax, d, L in TW.GEN_CASES if kmax == 2]
    assert len(cases) == 4
    for m, L in cases:
        for end in ("top", "bottom"):
            assert len(set(TW.class_ring(m, 2, L, end))) == L          # class_ring asserts the class of every limb


def ints(a):
    return np.asarray(a).astype(object)


@pytest.mark.parametrize("name", R.ALL_RINGS)
@pytest.mark.parametrize("m", [45, 64])
def test_c_restatement_matches_python_integers(oracle_lib, m, name):
    qs = resident_edge_rings(m)[name]
    q = np.array(qs, dtype=object)
    idx = G.Index(m)
    gen = oracle_lib.GenRing(m, qs)
    rings = [gen] + ([oracle_lib.Ring(m // 2, qs)] if m == 64 else [])     # the restatement check_ct_encrypt picks on a two-power index
    rng = np.random.default_rng(9000 + m)
    x = extreme_words(rng, 4, idx.n, qs)
    x[3] = q.astype(np.int64) - 1                                         # q-1 everywhere
    for o in rings:
        for i, j in ((0, 1), (2, 3), (3, 3), (0, 3)):
            a, b = ints(x[i]), ints(x[j])
            assert np.array_equal(ints(o.mul(x[i], x[j])), a * b % q)
            assert np.array_equal(ints(o.add(x[i], x[j])), (a + b) % q)
            assert np.array_equal(ints(o.sub(x[i], x[j])), (a - b) % q)
            assert np.array_equal(ints(o.sub(x[i], o.mul(x[j], x[i]))), (a - b * a) % q)         # c0 = err - c1 s
        for s in ([v - 1 for v in qs], [1] * len(qs), [(v + 1) // 2 for v in qs]):
            for e in (0, 3):
                assert np.array_equal(ints(o.scale(x[e], s)), ints(x[e]) * np.array(s, dtype=object) % q)
    for e in range(4):
        want = [G.crt_def(al, idx, qj) for al, qj in zip(from_aos(x[e]), qs)]
        c = gen.crt(x[e])
        assert from_aos(c) == want, e
        assert np.array_equal(gen.crtinv(c), x[e]), e
        assert [G.crt_def(al, idx, qj) for al, qj in zip(from_aos(gen.crtinv(x[e])), qs)] == from_aos(x[e]), e


def test_crt_def_is_exact_above_2_32():
    """crt_def against the Kronecker product of the per-axis definitions (Python integers throughout) on a 62-bit and a 32-bit prime."""
    for m in (45, 8, 96):
        idx = G.Index(m)
        r = resident_edge_rings(m)
        for q in (r["TOP62"][0], r["LOW64"][0], r["TOP31"][0]):
            a = extreme_words(np.random.default_rng(m), 1, idx.n, [q])[0][:, 0].tolist()
            assert G.crt_def(a, idx, q) == G.crt_kron(a, idx, q), (m, q)


@pytest.mark.parametrize("name", ["TOP62", "TOP31"])
@pytest.mark.parametrize("m,mb", [(9, 45), (4, 8)])
def test_the_crt_ext_funcs_at_the_top_of_both_word_sizes(m, mb, name):
    s, b = G.Index(m), G.Index(mb)
    qs = resident_edge_rings(mb)[name]
    rng = np.random.default_rng(9050 + mb)
    xs = np.concatenate([extreme_words(rng, 2, s.n, qs), to_aos([[q - 1] * s.n for q in qs])[None]])
    ys = np.concatenate([extreme_words(rng, 2, b.n, qs), to_aos([[q - 1] * b.n for q in qs])[None]])
    for e in range(3):
        for j, q in enumerate(qs):
            x, y = xs[e][:, j].tolist(), ys[e][:, j].tolist()
            assert G.twace_crt_def(G.crt_def(y, b, q), s, b, q) == G.crt_def(G.twace_pow_dec(y, s, b), s, q), (e, j)
            assert G.embed_crt_def(G.crt_def(x, s, q), s, b) == G.crt_def(G.embed_pow(x, s, b), b, q), (e, j)
            assert G.twace_pow_dec(G.embed_pow(x, s, b), s, b) == x
            assert all(0 <= v < q for v in G.twace_crt_def(y, s, b, q) + G.embed_dec_def(x, s, b, q))


def test_gauss_model_words_at_62_bit_moduli():
    import gauss_model as GM
    qs = resident_edge_rings(45)["MIX64"]
    z = np.array([[0, 1, -1, 65536, -65537, (1 << 30) + 12345, -(1 << 30) - 12345, (1 << 31), -(1 << 31) - 1]], dtype=np.int64)
    got = GM.words(z, qs)
    assert got.tolist() == [[[int(v) % q for q in qs] for v in z[0]]]
