"""CPU: alch_automorph_table (host-only; alchemy_amd/csrc/automorph_host.hpp) against the permutation restated from the header's slot
rule in Python integers (tests/automorph_model.py), and against sigma_j evaluated straight from its definition with the oracle's
by-definition pieces.  Indices: 16 (a two-power index below 32: general engine), 32 and 64 (radix-16 engine), 11 (one prime, the
largest the pass engine has beside 13), 9 and 121 (prime powers), 15, 21, 45, 63 (mixed)."""
import ctypes as C
import math
import random

import numpy as np
import pytest

import automorph_model as M
from alchemy_amd import capi
from alchemy_amd.automorph import automorph_table
from helpers import primes_1_mod
from oracle import model_gen as G

INDICES = [16, 32, 64, 9, 11, 15, 21, 45, 63, 121]


@pytest.mark.parametrize("m", INDICES)
def test_table_equals_the_model_for_every_unit(m):
    n = M.phi(m)
    for j in M.units(m):
        got = automorph_table(m, j)
        assert got.dtype == np.uint32 and got.shape == (n,)
        assert got.tolist() == M.table(m, j), (m, j)


@pytest.mark.parametrize("m", INDICES)
def test_identity_composition_and_reduction_mod_m(m):
    n = M.phi(m)
    assert automorph_table(m, 1).tolist() == list(range(n))
    us = M.units(m)
    rnd = random.Random(m)
    pairs = [(a, b) for a in us for b in us] if len(us) <= 12 else [(rnd.choice(us), rnd.choice(us)) for _ in range(60)]
    for j1, j2 in pairs:
        # crt(sigma_j1 sigma_j2 a)[k] = crt(sigma_j2 a)[t1[k]] = crt(a)[t2[t1[k]]]: the outer map's table is applied first
        t1, t2 = automorph_table(m, j1), automorph_table(m, j2)
        assert np.array_equal(automorph_table(m, j1 * j2 % m), t2[t1]), (m, j1, j2)
    for j in us[:6]:
        assert np.array_equal(automorph_table(m, j), automorph_table(m, j + m))
        assert np.array_equal(automorph_table(m, j), automorph_table(m, j + 5 * m))


def test_refusals():
    lib = capi.load_library()
    fn = lib.alch_automorph_table
    n = C.c_size_t(0)
    assert fn(45, 7, None, None) == capi.ALCH_E_INVALID                                  # null len
    for m, j in ((45, 3), (45, 0), (64, 2), (121, 11), (9, 12)):                         # non-units, before and after reduction
        assert fn(m, j, None, C.byref(n)) == capi.ALCH_E_INVALID, (m, j)
        assert b"unit" in lib.alch_last_error()
    for m in (17, 34, 51 * 4, 1 << 18, 3 ** 11):                                         # the prime 17; past either engine's size
        assert fn(m, 1, None, C.byref(n)) == capi.ALCH_E_UNSUPPORTED, m
    assert fn(0, 1, None, C.byref(n)) == capi.ALCH_E_INVALID
    assert fn(45, 7, None, C.byref(n)) == capi.ALCH_OK and n.value == 24
    out = (C.c_uint32 * 24)(*([0xFFFFFFFF] * 24))
    short = C.c_size_t(23)
    assert fn(45, 7, out, C.byref(short)) == capi.ALCH_E_INVALID                         # a short capacity: nothing written
    assert list(out) == [0xFFFFFFFF] * 24
    roomy = C.c_size_t(24)
    assert fn(45, 7, out, C.byref(roomy)) == capi.ALCH_OK and roomy.value == 24 and list(out) == M.table(45, 7)
    # the sizes the engines do serve, without the word-size test of alch_ring_create: 2^17 and the largest general dimension asked for
    assert fn(1 << 17, 5, None, C.byref(n)) == capi.ALCH_OK and n.value == 1 << 16
    assert fn(11648, 5, None, C.byref(n)) == capi.ALCH_OK and n.value == M.phi(11648)


@pytest.mark.parametrize("m", INDICES)
def test_table_equals_sigma_evaluated_from_its_definition(m):
    """Independent of the slot rule's inverse: sigma_j(a) = sum_i a_i zeta^(e(i) j) evaluated at omega^u from the exponents alone
    equals crt(a), by definition, read through the table at the slot that holds omega^u."""
    idx = G.Index(m)
    q = primes_1_mod(m, 1, 1 << 20)[0]
    rnd = random.Random(1000 + m)
    a = [rnd.randrange(q) for _ in range(idx.n)]
    w = G.omega_m(q, m)
    crt_a = G.crt_def(a, idx, q)
    ex = [idx.pow_exponent(i) for i in range(idx.n)]
    us = M.units(m)
    for j in (us if len(us) <= 12 else rnd.sample(us, 12)):
        tab = automorph_table(m, j)
        for k in range(idx.n):
            u = idx.slot_unit(k)
            direct = sum(x * pow(w, e * j * u % m, q) for x, e in zip(a, ex)) % q
            assert direct == crt_a[int(tab[k])], (m, j, k)
        # and through the powerful basis: crt of the substituted element is the permuted crt
        assert G.crt_def(M.sigma_pow(a, idx, j, q), idx, q) == [crt_a[int(t)] for t in tab], (m, j)


def test_two_power_substitution_agrees_with_the_general_reduction():
    idx = G.Index(32)
    rnd = random.Random(3)
    a = [rnd.randrange(-50, 50) for _ in range(16)]
    for j in M.units(32):
        assert M.sigma_pow_twopower(a, j) == M.sigma_pow(a, idx, j)
    assert math.gcd(5, 32) == 1
