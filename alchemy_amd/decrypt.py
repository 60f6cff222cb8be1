"""SymmSHE decrypt and the ErrorRateWriter's errorRate_ on device-resident ciphertext batches (include/alchemy_hip.h, "since 1.8":
alch_ct_error_term, alch_buf_lift, alch_ct_decrypt_lift).

Both start from c(s) -- the ciphertext polynomial evaluated at the secret key -- on the decoding basis and lift it, centred, from
Z_q to the integers (Crypto/Alchemy/Interpreter/PT2CT.hs:91-99, Eval.hs:150-160).  The device returns error magnitudes as exact
mixed-radix digit vectors; this module turns them into Python integers and rounds once, at the end."""
from __future__ import annotations

import ctypes as C
from fractions import Fraction

from .capi import (ALCH_BASIS_DEC, ALCH_NOT_DIVISIBLE, AlchemyError, Buf, Ring, _check, _pu64, load_library)


def _prod(qs) -> int:
    out = 1
    for q in qs:
        out *= int(q)
    return out


def digits_to_int(digits, qs) -> int:
    """The integer d_0 + q_0 (d_1 + q_1 (d_2 + ...)) of one mixed-radix digit vector (limb 0 least significant)."""
    x = 0
    for d, q in zip(reversed(list(digits)), reversed(list(qs))):
        x = x * int(q) + int(d)
    return x


def _digit_rows(arr, count: int, L: int):
    return [[int(arr[i * L + j]) for j in range(L)] for i in range(count)]


def error_term(cts: Buf, batch: int, sk: Buf, degree: int = 1, s_pre=None, flags: int = 0, out: Buf | None = None,
               out_first: int = 0, sk_index: int = 0) -> Buf:
    """c_b(s) for the `batch` ciphertexts of `cts` (elements (degree + 1) b ..; CRT basis, or Pow with ALCH_POW_IN) and the key
    element `sk_index` of `sk` (CRT basis), times toLSD's per-limb scalar `s_pre`; the result (a new buffer unless `out` is given)
    is on the decoding basis -- the object errorTermUnrestricted lifts.  The input is left untouched."""
    if out is None:
        out, out_first = cts.ring.alloc(max(1, batch)), 0
    sp = _pu64(s_pre) if s_pre is not None else None
    _check(load_library().alch_ct_error_term(cts._h, batch, degree, sk._h, sk_index, sp, out._h, out_first, flags))
    return out


def lift(buf: Buf, dst: Buf | None = None, l: int = 1, want_max: bool = False, first: int = 0, count: int | None = None,
         dst_first: int = 0):
    """Centred lift mod Q = prod q_j of every coefficient of elements [first, first + count) of `buf` (Pow or Dec basis).
    dst: a buffer of a one-modulus ring of the same index; element dst_first + i becomes l * (lift mod p) mod p.
    want_max: returns, per element, the digit vector (limb 0 least significant) of the largest |lift|; digits_to_int turns one into
    an integer.  Returns None otherwise."""
    count = buf.n_elems - first if count is None else count
    L = buf.ring.L
    arr = (C.c_uint64 * max(1, count * L))() if want_max else None
    _check(load_library().alch_buf_lift(buf._h, first, count, dst._h if dst is not None else None, dst_first, C.c_uint64(int(l)), arr))
    return _digit_rows(arr, count, L) if want_max else None


def decrypt_lift(cts: Buf, batch: int, sk: Buf, degree: int = 1, s_pre=None, dst: Buf | None = None, l: int = 1,
                 want_max: bool = False, flags: int = 0, dst_first: int = 0, sk_index: int = 0):
    """error_term followed by lift in one call, the intermediate in the ring's own scratch: what decrypt and errorRate_ need."""
    L = cts.ring.L
    arr = (C.c_uint64 * max(1, batch * L))() if want_max else None
    sp = _pu64(s_pre) if s_pre is not None else None
    _check(load_library().alch_ct_decrypt_lift(cts._h, batch, degree, sk._h, sk_index, sp, dst._h if dst is not None else None,
                                               dst_first, C.c_uint64(int(l)), arr, flags))
    return _digit_rows(arr, batch, L) if want_max else None


def error_rates(cts: Buf, batch: int, sk: Buf, degree: int = 1, s_pre=None, flags: int = 0, sk_index: int = 0) -> list:
    """errorRate_ of every ciphertext of the batch: max_k |liftDec(c(s))_k| / Q, computed exactly (Python integers, Fraction) from
    the device's digit vectors and rounded to a float once."""
    qs = cts.ring.qs
    Q = _prod(qs)
    rows = decrypt_lift(cts, batch, sk, degree, s_pre, None, 1, True, flags, 0, sk_index)
    return [float(Fraction(digits_to_int(d, qs), Q)) for d in rows]


def decrypt_batch(cts: Buf, batch: int, sk: Buf, zp_big_ring: Ring, zp_small_ring: Ring, k: int, l: int, degree: int = 1,
                  s_pre=None, flags: int = 0, sk_index: int = 0) -> Buf:
    """SymmSHE decrypt of a resident batch: l * twace(g^-k (liftDec(c(s)) mod p)) as a buffer of `zp_small_ring` (the plaintext
    index, one modulus p) on the Pow basis.  zp_big_ring: the same modulus over the ciphertext index.  k, l: the g-power and Z_p
    scalar of the LSD form, s_pre its per-limb scalar (None when the ciphertexts are LSD already).  Raises AlchemyError with the
    library's ALCH_NOT_DIVISIBLE status when a divG fails."""
    big = zp_big_ring.alloc(max(1, batch))
    decrypt_lift(cts, batch, sk, degree, s_pre, big, l, False, flags, 0, sk_index)
    for _ in range(k):
        if not big.divg(ALCH_BASIS_DEC, 0, batch):
            raise AlchemyError(ALCH_NOT_DIVISIBLE, "decrypt: divG failed on the plaintext ring (Lol's Nothing)")
    if zp_small_ring is zp_big_ring:
        out = big
    else:
        out = zp_small_ring.alloc(max(1, batch))
        out.twace_from(big, batch, ALCH_BASIS_DEC)
    out.l(0, batch)
    return out
