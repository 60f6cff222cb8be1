"""GPU: alch_buf_gauss_dec (kernels k_gauss_sample, k_gauss_axis, k_gauss_round of alchemy_amd/csrc/kernel_rlwe.hpp) against the Python
model written from the definition (tests/gauss_model.py): every stored word equal, bit for bit, and below its modulus.

Indices: 16 (general engine, n = 8), 64 (fused two-power), 21 (n = 12, not a multiple of the vector width), 45 (prime power,
m_p' = 3), 60 (2^2 and two odd axes), 91 (h = 12), 1365 (axes of 3, 5, 7 and 13 at once).  Rings: one and three 31-bit limbs (32-bit
words), three limbs just below 2^62 (64-bit words).  Cosets: none, p in {2, 32, 7, 2^31 - 1}.

On the parent commit the library has no such symbol and the package no `encrypt` module: this module does not import there."""
import ctypes as C
import math

import numpy as np
import pytest

import alchemy_amd as A
import gauss_model as GM
from alchemy_amd import capi
from alchemy_amd import encrypt as E
from helpers import assert_reduced, primes_1_mod, primes_below

pytestmark = pytest.mark.gpu

INDICES = [16, 64, 21, 45, 60, 91, 1365]
P_SET = [None, 2, 32, 7, (1 << 31) - 1]
RINGS = ["w32x1", "w32x3", "w64x3"]


def ring_moduli(m, kind):
    if kind == "w32x1":
        return primes_1_mod(m, 1, 1 << 29)
    if kind == "w32x3":
        return primes_1_mod(m, 3, 1 << 20)                 # far below the largest |z| of the big cosets: the remainder path runs
    return primes_below(m, 3, 1 << 62)


def svar_for(m, p):
    return 3.0 / math.sqrt(GM.totient(m)) * (float(p) * float(p) if p else 1.0)


def coset_buffer(m, p, count, seed):
    zp = A.Ring(m, [p], nocrt=True)
    buf = zp.alloc(count)
    buf.fill_uniform(seed)
    return zp, buf, buf.download()[:, :, 0]


@pytest.mark.parametrize("kind", RINGS)
@pytest.mark.parametrize("m", INDICES)
def test_words_equal_the_model(m, kind):
    """count = 5 at first = 1 of a seven-element buffer (coset_first = 1 likewise): the five elements equal the model's, the other
    two keep what fill_uniform wrote; one of the runs has its counters wrap mod 2^64."""
    qs = ring_moduli(m, kind)
    ring = A.Ring(m, qs)
    assert ring.word_bytes == (8 if kind == "w64x3" else 4)
    for i, p in enumerate(P_SET):
        seed, elem0 = 0xA1C0000 + 977 * m + i, ((1 << 64) - 3 if p == 7 else 11 * i)
        dst = ring.alloc(7)
        dst.fill_uniform(5)
        before = dst.download()
        zp = cb = cw = None
        if p:
            zp, cb, cw = coset_buffer(m, p, 7, 40 + i)
        E.gauss_dec(dst, svar_for(m, p), seed, 1, 5, cb, 1, elem0)
        got = dst.download()
        z = GM.gauss_dec(m, svar_for(m, p), seed, elem0, 5, p, cw[1:6] if p else None)
        assert np.array_equal(got[1:6], GM.words(z, qs)), (m, kind, p)
        assert np.array_equal(got[0], before[0]) and np.array_equal(got[6], before[6])
        assert_reduced(got, qs)
        assert int(np.abs(z).max()) > (p or 1) // 2                       # not all zero: the sampler did something
        if p:
            assert np.array_equal(np.mod(z, p), cw[1:6])
        del dst, cb, zp


def test_destinations_without_crt_basis():
    """A Z_p ring as destination, with its own elements as the coset (in place), and the integers (modulus 0: z itself)."""
    m, p = 21, 32
    zp, buf, cw = coset_buffer(m, p, 3, 9)
    E.gauss_dec(buf, svar_for(m, p), 77, 0, 3, buf, 0, 0)
    z = GM.gauss_dec(m, svar_for(m, p), 77, 0, 3, p, cw)
    assert np.array_equal(buf.download()[:, :, 0], np.mod(z, p)) and np.array_equal(np.mod(z, p), cw)
    zint = A.Ring(m, [0], nocrt=True)
    out = zint.alloc(3)
    E.gauss_dec(out, svar_for(m, p), 77, 0, 3, buf, 0, 0)
    assert np.array_equal(out.download()[:, :, 0], z)


def test_chunks_give_the_words_of_one_call():
    m, p = 45, 7
    qs = primes_1_mod(m, 2, 1 << 29)
    ring = A.Ring(m, qs)
    zp, cb, cw = coset_buffer(m, p, 5, 3)
    whole, parts = ring.alloc(5), ring.alloc(5)
    E.gauss_dec(whole, svar_for(m, p), 123, 0, 5, cb, 0, 1000)
    E.gauss_dec(parts, svar_for(m, p), 123, 0, 2, cb, 0, 1000)
    E.gauss_dec(parts, svar_for(m, p), 123, 2, 3, cb, 2, 1002)
    assert np.array_equal(whole.download(), parts.download())
    assert np.array_equal(whole.download(), GM.words(GM.gauss_dec(m, svar_for(m, p), 123, 1000, 5, p, cw), qs))


def test_past_the_grid():
    """m = 4096, 300 elements: 614 400 deviates against 2048 workgroups of 256 lanes, so the grid-stride loop wraps."""
    m, count = 4096, 300
    qs = primes_1_mod(m, 1, 1 << 29)
    ring = A.Ring(m, qs)
    dst = ring.alloc(count)
    E.gauss_dec(dst, svar_for(m, None), 2026, 0, count, None, 0, 0)
    got = dst.download()
    assert np.array_equal(got, GM.words(GM.gauss_dec(m, svar_for(m, None), 2026, 0, count), qs))
    assert_reduced(got, qs)


def test_statuses():
    lib = capi.load_library()
    fn = lib.alch_buf_gauss_dec
    qs = primes_1_mod(21, 2, 1 << 29)
    ring = A.Ring(21, qs)
    dst = ring.alloc(4)
    dst.fill_uniform(1)
    before = dst.download()
    zp, zp64, zp2 = A.Ring(21, [32], nocrt=True), A.Ring(64, [32], nocrt=True), A.Ring(21, [32, 7], nocrt=True)
    cs, cs64, cs2, csq = zp.alloc(4), zp64.alloc(4), zp2.alloc(4), ring.alloc(4)
    ok = E.double_bits(1.0)
    # count 0: success, nothing queued -- with and without a coset
    assert fn(dst._h, 0, 0, ok, None, 0, 1, 0) == 0 and fn(dst._h, 4, 0, ok, cs._h, 4, 1, 0) == 0
    assert np.array_equal(dst.download(), before)
    bad = [
        (dst._h, 0, 4, E.double_bits(0.0), None, 0, 1, 0),
        (dst._h, 0, 4, E.double_bits(-1.0), None, 0, 1, 0),
        (dst._h, 0, 4, E.double_bits(float("nan")), None, 0, 1, 0),
        (dst._h, 0, 4, E.double_bits(float("inf")), None, 0, 1, 0),
        (dst._h, 0, 4, E.double_bits(1e36), None, 0, 1, 0),              # sigma ~ 4e17: 9 sigma times the axis norms passes 2^62
        (dst._h, 0, 4, E.double_bits(1e300), None, 0, 1, 0),
        (dst._h, 1, 4, ok, None, 0, 1, 0),                               # destination range
        (dst._h, 5, 0, ok, None, 0, 1, 0),
        (dst._h, 0, 4, ok, cs._h, 1, 1, 0),                              # coset range
        (dst._h, 0, 4, ok, cs64._h, 0, 1, 0),                            # coset of another index
        (dst._h, 0, 4, ok, cs2._h, 0, 1, 0),                             # two coset moduli
        (dst._h, 0, 4, ok, csq._h, 0, 1, 0),                             # two coset moduli (a CRT ring)
        (None, 0, 4, ok, None, 0, 1, 0),
    ]
    for args in bad:
        assert fn(*args) == capi.ALCH_E_INVALID, args
        assert lib.alch_last_error().decode().startswith("alch_buf_gauss_dec")
    assert np.array_equal(dst.download(), before)
    # the largest svar the bound admits still runs and still matches
    E.gauss_dec(dst, 1e30, 5, 0, 4)
    assert np.array_equal(dst.download(), GM.words(GM.gauss_dec(21, 1e30, 5, 0, 4), qs))
