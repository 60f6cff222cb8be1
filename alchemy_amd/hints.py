"""Key-switch and tunnel hints generated on device-resident buffers (include/alchemy_hip.h, "key-switch and tunnel hints":
alch_ct_ks_hint, alch_ct_ks_hint_part) -- ksHint, ksQuadCircHint and tunnelHint of KeysHints.hs:101-129.

Seeds follow encrypt_batch: the Gaussian stream is splitmix64(seed), the uniform stream splitmix64(seed + 1).  Every stored word is an
integer-exact function of (seed, position), so a hint made in chunks has the words of one call.  splitmix64 is a statistical
generator, not a cryptographic one; with a key on the ring (Ring.set_rng_key) both streams are ChaCha20 keystreams and the seeds are nonces."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .capi import ALCH_EXT_COEFFS, ALCH_GAD_TRIV, Buf, Hint, Ring, Tunnel, _check, ext_table, load_library
from .encrypt import _M64, gauss_dec, splitmix64

# error terms held at once by ks_hint (bytes); a longer hint is made in parts
CHUNK_BYTES = 256 << 20


def ct_ks_hint(out: Buf, gadget: int, n_v: int, v_crt: Buf, err_crt: Buf, sk_crt: Buf, seed: int, out_first: int = 0, v_first: int = 0,
               err_first: int = 0, sk_index: int = 0, ct0: int = 0):
    """For i < n_v, t < D, e = i D + t: out[out_first + 2e + 1] = a (uniform from `seed`, counter ct0 + e),
    out[out_first + 2e] = g_t v[v_first + i] + err[err_first + e] - a * sk, everything on the CRT basis."""
    _check(load_library().alch_ct_ks_hint(out._h, out_first, gadget, n_v, v_crt._h, v_first, err_crt._h, err_first, sk_crt._h, sk_index,
                                          C.c_uint64(seed & _M64), C.c_uint64(ct0 & _M64)))


def ct_ks_hint_part(out: Buf, gadget: int, e_first: int, e_count: int, v_crt: Buf, err_crt: Buf, sk_crt: Buf, seed: int,
                    out_first: int = 0, v_first: int = 0, err_first: int = 0, sk_index: int = 0, ct0: int = 0):
    """Entries [e_first, e_first + e_count) of the same hint; out_first, err_first and ct0 are those of entry e_first."""
    _check(load_library().alch_ct_ks_hint_part(out._h, out_first, gadget, e_first, e_count, v_crt._h, v_first, err_crt._h, err_first,
                                               sk_crt._h, sk_index, C.c_uint64(seed & _M64), C.c_uint64(ct0 & _M64)))


def ks_hint(ring: Ring, gadget: int, sk_crt: Buf, v_crt: Buf, n_v: int, svar: float, seed: int, sk_index: int = 0,
            chunk_bytes: int | None = None) -> Buf:
    """ksHint for the values v_crt[0 .. n_v) under the key: 2 * n_v * D elements of `ring` on the CRT basis, order value, gadget entry,
    (b, a) with b + a s = g_t v + e.  e: rounded samples of scaled variance `svar` (errorRounded), taken to the powerful and the CRT
    basis.  The layout is alch_hint_from_buf's for n_v = 1 and the ks_crt of alch_tunnel_create for n_v = d_rel."""
    D = ring.gadget_digits(gadget)
    total = n_v * D
    out = ring.alloc(max(1, 2 * total))
    elem_bytes = ring.n * ring.L * ring.word_bytes
    chunk = max(1, (CHUNK_BYTES if chunk_bytes is None else chunk_bytes) // elem_bytes)
    err = ring.alloc(max(1, min(chunk, total)))
    g_seed, u_seed = splitmix64(seed), splitmix64(seed + 1)
    for done in range(0, total, chunk):
        now = min(chunk, total - done)
        gauss_dec(err, svar, g_seed, 0, now, elem0=done)
        err.l(0, now)                       # an integer matrix: it commutes with the reduction mod q_j
        err.crt(0, now)
        if now == total:
            ct_ks_hint(out, gadget, n_v, v_crt, err, sk_crt, u_seed, sk_index=sk_index)
        else:
            ct_ks_hint_part(out, gadget, done, now, v_crt, err, sk_crt, u_seed, out_first=2 * done, sk_index=sk_index, ct0=done)
    return out


def ks_quad_circ_hint(ring: Ring, gadget: int, sk_crt: Buf, svar: float, seed: int) -> Hint:
    """ksQuadCircHint: the hint that takes the s^2 component of a quadratic ciphertext back under s."""
    s2 = ring.alloc(1)
    s2.mul(sk_crt, sk_crt, 1)
    return ring.hint_from_buf(ks_hint(ring, gadget, sk_crt, s2, 1, svar, seed), gadget)


def _zero(buf: Buf):
    buf.scale(buf, buf.n_elems, [0] * buf.ring.L)


def tunnel_values(ring_r: Ring, ring_s: Ring, lin_crt: Buf, sk_in_crt: Buf) -> Buf:
    """v_i = f'(s_in p_i), i < d_rel, on the CRT basis of ring_s: p_i the relative powerful basis of R'/E', f' the E'-linear function
    whose values on the relative decoding basis are lin_crt.  Computed by the tunnel entry point itself: a tunnel with an all-zero hint
    sends the ciphertext (x, 0) to (f'(x), 0)."""
    ep, d_rel = Tunnel.info(ring_r, ring_s)
    D = ring_s.L                                                        # TrivGad: the smallest zero hint
    zero = ring_s.alloc(2 * d_rel * D)
    _zero(zero)
    tun = Tunnel(ring_r, ring_s, lin_crt, zero, gadget=ALCH_GAD_TRIV)
    pos = ext_table(ep, ring_r.m, ALCH_EXT_COEFFS).reshape(d_rel, -1)[:, 0]
    units = np.zeros((2 * d_rel, ring_r.n, ring_r.L), dtype=np.int64)
    for i in range(d_rel):
        units[2 * i, int(pos[i]), :] = 1
    cin = ring_r.upload(units)
    cin.crt()
    prod = ring_r.alloc(2 * d_rel)
    prod.mul_public(cin, sk_in_crt, 0, 2 * d_rel)                       # (s_in p_i, 0)
    cout = ring_s.alloc(2 * d_rel)
    tun.apply(prod, cout, d_rel)
    v = ring_s.alloc(d_rel)
    for i in range(d_rel):
        v.copy_from(cout, 1, i, 2 * i)
    ring_s.sync()
    tun.free()
    return v


def tunnel_hint(ring_r: Ring, ring_s: Ring, gadget: int, lin_crt: Buf, sk_out_crt: Buf, sk_in_crt: Buf, svar: float, seed: int) -> Tunnel:
    """tunnelHint f sk_out sk_in: the device-resident tunnel from ring_r = R'_q to ring_s = S'_q whose hints encrypt f'(s_in p_i) under
    s_out.  lin_crt: the d_rel values of f' on the relative decoding basis, CRT basis of ring_s (alch_tunnel_create)."""
    _, d_rel = Tunnel.info(ring_r, ring_s)
    v = tunnel_values(ring_r, ring_s, lin_crt, sk_in_crt)
    ks = ks_hint(ring_s, gadget, sk_out_crt, v, d_rel, svar, seed)
    return Tunnel(ring_r, ring_s, lin_crt, ks, gadget=gadget)
