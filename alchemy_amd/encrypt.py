"""SymmSHE encrypt on device-resident batches (include/alchemy_hip.h, "encrypt on resident batches": alch_buf_gauss_dec,
alch_ct_encrypt; host-only alch_gauss_table, alch_gauss_plan) -- the mirror image of decrypt.py.

The error sampler is counter-based: every stored word is an integer-exact function of (seed, position), so a batch cut into chunks
gives the words of one call.  splitmix64 is a statistical generator, not a cryptographic one: for real secrets set a key on the ring that
is written (Ring.set_rng_key) -- the same calls then draw from ChaCha20 keystreams addressed by (key, seed, domain, position), and a
(key, seed) pair serves one batch per entry point."""
from __future__ import annotations

import ctypes as C
import struct

from .capi import ALCH_BASIS_POW, Buf, Ring, _check, load_library

_M64 = (1 << 64) - 1


def splitmix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def double_bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def bits_double(b: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", int(b)))[0]


def gauss_table() -> list:
    """The cumulative table T[t] = floor(2^63 P(|K| <= t)), K ~ D_{Z,64} (host only)."""
    lib, n = load_library(), C.c_size_t(0)
    _check(lib.alch_gauss_table(None, C.byref(n)))
    arr = (C.c_uint64 * n.value)()
    _check(lib.alch_gauss_table(arr, C.byref(n)))
    return [int(v) for v in arr]


def gauss_plan(m: int, svar: float):
    """(scale, [Cholesky factor of p I - J as a flat row-major list, for every odd prime p of m ascending]) (host only)."""
    lib, scale, n = load_library(), C.c_uint64(), C.c_size_t(0)
    _check(lib.alch_gauss_plan(m, double_bits(svar), C.byref(scale), None, C.byref(n)))
    arr = (C.c_uint64 * max(1, n.value))()
    _check(lib.alch_gauss_plan(m, double_bits(svar), C.byref(scale), arr, C.byref(n)))
    flat, out, at, t, p = [bits_double(arr[i]) for i in range(n.value)], [], 0, m, 3
    while t % 2 == 0:
        t //= 2
    while t > 1:
        if t % p == 0:
            out.append(flat[at:at + (p - 1) ** 2])
            at += (p - 1) ** 2
            while t % p == 0:
                t //= p
        p += 2
    return bits_double(scale.value), out


def gauss_dec(dst: Buf, svar: float, seed: int, first: int = 0, count: int | None = None, coset: Buf | None = None,
              coset_first: int = 0, elem0: int = 0):
    """Elements [first, first + count) of `dst` become errorRounded (coset None) or errorCoset samples of scaled variance `svar` on the
    decoding basis, reduced into dst's moduli.  coset: a buffer of a one-modulus ring of the same index.  elem0 shifts the counters."""
    count = dst.n_elems - first if count is None else count
    _check(load_library().alch_buf_gauss_dec(dst._h, first, count, double_bits(svar), coset._h if coset is not None else None,
                                             coset_first, C.c_uint64(seed & _M64), C.c_uint64(elem0 & _M64)))


def ct_encrypt(out: Buf, batch: int, err_crt: Buf, sk_crt: Buf, seed: int, err_first: int = 0, sk_index: int = 0, ct0: int = 0):
    """out[2b] = err[err_first + b] - c1 * sk, out[2b + 1] = c1 (uniform from `seed`), everything on the CRT basis."""
    _check(load_library().alch_ct_encrypt(out._h, batch, err_crt._h, err_first, sk_crt._h, sk_index, C.c_uint64(seed & _M64),
                                          C.c_uint64(ct0 & _M64)))


def gen_sk(ring: Ring, svar: float, seed: int) -> Buf:
    """SymmSHE genSK: one rounded sample (stream splitmix64(seed)), taken to the powerful and then the CRT basis."""
    sk = ring.alloc(1)
    gauss_dec(sk, svar, splitmix64(seed))
    sk.l()
    sk.crt()
    return sk


def encrypt_batch(ring: Ring, sk_crt: Buf, pt: Buf, zp_small_ring: Ring, zp_big_ring: Ring, svar: float, seed: int,
                  sk_index: int = 0) -> Buf:
    """SymmSHE encrypt of a resident plaintext batch: `pt` holds Pow-basis elements of `zp_small_ring` (the plaintext index, one
    modulus p); zp_big_ring is the same modulus over the ciphertext index.  Returns 2 * batch elements of `ring`, CRT basis:
    `CT LSD 0 1 [c0, c1]` per plaintext.  The Gaussian uses the stream splitmix64(seed), the uniform c1 splitmix64(seed + 1)."""
    assert pt.ring is zp_small_ring
    batch, p = pt.n_elems, zp_big_ring.qs[0]
    big = zp_big_ring.alloc(max(1, batch))
    if zp_small_ring is zp_big_ring:
        big.copy_from(pt, batch)
    else:
        big.embed_from(pt, batch, ALCH_BASIS_POW)
    big.linv(0, batch)
    err = ring.alloc(max(1, batch))
    gauss_dec(err, svar * p * p, splitmix64(seed), 0, batch, big)
    err.l(0, batch)                        # an integer matrix: it commutes with the reduction mod q_j
    err.crt(0, batch)
    out = ring.alloc(max(1, 2 * batch))
    ct_encrypt(out, batch, err, sk_crt, splitmix64(seed + 1), 0, sk_index)
    return out
