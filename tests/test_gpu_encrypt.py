"""GPU: SymmSHE encrypt on resident batches -- alch_ct_encrypt (k_ct_encrypt, alchemy_amd/csrc/kernel_rlwe.hpp) against the C
restatement word for word, and gen_sk + encrypt_batch (alchemy_amd/encrypt.py) closed by decrypt_batch: the plaintexts come back, and
the error rates of the fresh batch are max |z| / Q of the model's error terms exactly (c(s) of a fresh ciphertext is the error itself).

On the parent commit the package has no `encrypt` module: this module does not import there."""
from fractions import Fraction

import numpy as np
import pytest

import alchemy_amd as A
import gauss_model as GM
from alchemy_amd import capi
from alchemy_amd import encrypt as E
from helpers import assert_reduced, primes_1_mod, primes_below
from oracle import cref
from oracle import model_gen as G

pytestmark = pytest.mark.gpu


def oracle_ring(m, qs):
    return cref.Ring(m // 2, qs) if m & (m - 1) == 0 else cref.GenRing(m, qs)


def check_ct_encrypt(m, qs, B, words=None, word_bytes=None):
    """B ciphertexts from error terms at err_first = 1 and the key element 1; then the last B - B // 2 of them once more through a view
    of another buffer with ct0 advanced.  words(rng, count, n, qs): the error terms and the key (default: alch_buf_fill_uniform)."""
    ring, orc = A.Ring(m, qs), oracle_ring(m, qs)
    assert word_bytes is None or ring.word_bytes == word_bytes
    err, sk, out, uni = ring.alloc(B + 1), ring.alloc(2), ring.alloc(2 * B), ring.alloc(2 * B)
    err.fill_uniform(11)
    sk.fill_uniform(12)
    if words is not None:
        rng = np.random.default_rng(m + B)
        err.upload(words(rng, B + 1, ring.n, qs))
        sk.upload(words(rng, 2, ring.n, qs))
    seed = 0xC1C1 + m
    uni.fill_uniform(seed)
    E.ct_encrypt(out, B, err, sk, seed, err_first=1, sk_index=1)
    got, u, e, s = out.download(), uni.download(), err.download(), sk.download()[1]
    assert_reduced(got, qs)
    for b in range(B):
        assert np.array_equal(got[2 * b + 1], u[2 * b + 1]), (m, b)
        assert np.array_equal(got[2 * b], orc.sub(e[1 + b], orc.mul(u[2 * b + 1], s))), (m, b)
    skip = B // 2
    other = ring.alloc(2 * B)
    other.fill_uniform(1)
    keep = other.download()
    E.ct_encrypt(other.view(2 * skip, 2 * (B - skip)), B - skip, err, sk, seed, err_first=1 + skip, sk_index=1, ct0=skip)
    again = other.download()
    assert np.array_equal(again[2 * skip:], got[2 * skip:]) and np.array_equal(again[:2 * skip], keep[:2 * skip])
    return seed, got, u, e, s


@pytest.mark.parametrize("word", [32, 64])
@pytest.mark.parametrize("m", [16, 64, 21, 45])
def test_ct_encrypt_equals_the_restatement(m, word):
    qs = primes_1_mod(m, 2, 1 << 29) if word == 32 else primes_below(m, 2, 1 << 62)
    check_ct_encrypt(m, qs, 4)


def test_ct_encrypt_at_a_split_size():
    m = 1 << 17                                             # n = 2^16: the largest 32-bit ring, run as two halves by the transforms
    check_ct_encrypt(m, primes_1_mod(m, 1, 1 << 29), 2)


def test_ct_encrypt_statuses():
    lib = capi.load_library()
    fn = lib.alch_ct_encrypt
    qs = primes_1_mod(64, 2, 1 << 29)
    ring, other, zp = A.Ring(64, qs), A.Ring(64, qs[:1]), A.Ring(64, [8], nocrt=True)
    out, err, sk = ring.alloc(4), ring.alloc(2), ring.alloc(1)
    for b in (out, err, sk):
        b.fill_uniform(3)
    err_other, sk_other = other.alloc(2), other.alloc(1)
    before = out.download()
    assert fn(out._h, 0, err._h, 0, sk._h, 0, 1, 0) == 0 and fn(out._h, 0, err._h, 2, sk._h, 0, 1, 0) == 0
    assert np.array_equal(out.download(), before)
    bad = [
        (out._h, 3, err._h, 0, sk._h, 0, 1, 0),                          # six elements wanted of four
        (out._h, 2, err._h, 1, sk._h, 0, 1, 0),                          # error-term range
        (out._h, 2, err._h, 0, sk._h, 1, 1, 0),                          # key index
        (out._h, 2, err_other._h, 0, sk._h, 0, 1, 0),                    # error terms of another ring
        (out._h, 2, err._h, 0, sk_other._h, 0, 1, 0),                   # key of another ring
        (out._h, 2, out._h, 0, sk._h, 0, 1, 0),                          # the error terms alias the output
        (out._h, 1, err._h, 0, out._h, 1, 1, 0),                         # the key lies in the output
        (None, 2, err._h, 0, sk._h, 0, 1, 0),
        (out._h, 2, None, 0, sk._h, 0, 1, 0),
    ]
    for args in bad:
        assert fn(*args) == capi.ALCH_E_INVALID, args
        assert lib.alch_last_error().decode().startswith("alch_ct_encrypt")
    zo, ze, zs = zp.alloc(2), zp.alloc(1), zp.alloc(1)
    assert fn(zo._h, 1, ze._h, 0, zs._h, 0, 1, 0) == capi.ALCH_E_NO_CRT
    assert np.array_equal(out.download(), before)


@pytest.mark.parametrize("m,mp,p", [(3, 21, 4), (8, 32, 32), (5, 45, 8), (4, 60, 2)])
def test_encrypt_then_decrypt_returns_the_plaintext(m, mp, p):
    batch, seed = 5, 4242 + mp
    qs = primes_1_mod(mp, 1, 1 << 20) + primes_1_mod(mp, 1, 1 << 29)
    Q = qs[0] * qs[1]
    small, big = G.Index(m), G.Index(mp)
    ring, zp_small, zp_big = A.Ring(mp, qs), A.Ring(m, [p], nocrt=True), A.Ring(mp, [p], nocrt=True)
    svar = 3.0 / np.sqrt(float(big.n))
    sk = E.gen_sk(ring, svar, seed + 1)
    rng = np.random.default_rng(seed)
    pts = rng.integers(0, p, size=(batch, small.n, 1), dtype=np.int64)
    cts = E.encrypt_batch(ring, sk, zp_small.upload(pts), zp_small, zp_big, svar, seed)
    assert cts.n_elems == 2 * batch
    assert_reduced(cts.download(), qs)
    back = A.decrypt_batch(cts, batch, sk, zp_big, zp_small, 0, 1)
    assert np.array_equal(back.download(0, batch), pts)
    # the model's error terms: the coset is lInv(embed(pt)) on the Z_p ring, the stream splitmix64(seed), svar * p^2
    coset = np.array([G.linv_def(G.embed_pow([int(v) for v in pts[b, :, 0]], small, big), big, p) for b in range(batch)], dtype=np.int64)
    z = GM.gauss_dec(mp, float(svar) * p * p, E.splitmix64(seed), 0, batch, p, np.mod(coset, p))
    assert int(np.abs(z).max()) * 2 < Q
    rates = A.error_rates(cts, batch, sk)
    assert rates == [float(Fraction(int(np.abs(z[b]).max()), Q)) for b in range(batch)]
    # and the secret key is the model's rounded sample, taken to the powerful and the CRT basis
    zs = GM.gauss_dec(mp, float(svar), E.splitmix64(seed + 1), 0, 1)[0]
    want_sk = np.stack([np.array(G.l_def([int(v) for v in zs], big, q), dtype=np.int64) % q for q in qs], axis=1)
    got_sk = ring.alloc(1)
    got_sk.copy_from(sk, 1)
    got_sk.crtinv()
    assert np.array_equal(got_sk.download()[0], want_sk)
