"""Galois automorphisms sigma_j : zeta_m -> zeta_m^j on device-resident batches (include/alchemy_hip.h, "Galois automorphisms":
alch_automorph_table, alch_buf_automorph, alch_automorph_create / _free, alch_ct_automorph).

On the CRT basis sigma_j is a permutation of slots, crt(sigma_j a)[slot(u)] = crt(a)[slot(u j mod m)]; on a ciphertext it is that
permutation of (c0, c1) followed by ONE linear key switch from sigma_j(s) back to s.  The hint of that key switch is an ordinary
ksHint for the value sigma_j(s): `automorph_hint` composes it as `ks_hint` composes every other hint, so seeds, chunking and keyed
streams (Ring.set_rng_key) apply unchanged."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .capi import ALCH_AUTO_SUM, ALCH_GAD_TRIV, Buf, Ring, _check, _pu64, load_library
from .hints import ks_hint


def automorph_table(m: int, j: int) -> np.ndarray:
    """Host only (no GPU needed): entry k is the SOURCE slot of destination slot k under sigma_j on the CRT basis of index m."""
    lib, n = load_library(), C.c_size_t(0)
    _check(lib.alch_automorph_table(m, j % (1 << 32), None, C.byref(n)))
    out = np.zeros(n.value, dtype=np.uint32)
    _check(lib.alch_automorph_table(m, j % (1 << 32), out.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(n)))
    return out


def buf_automorph(dst: Buf, src: Buf, j: int, count: int | None = None, dst_first: int = 0, src_first: int = 0):
    """dst[dst_first + e] = sigma_j(src[src_first + e]), e < count, CRT-basis elements of one ring; the ranges share no byte."""
    count = src.n_elems - src_first if count is None else count
    _check(load_library().alch_buf_automorph(dst._h, dst_first, src._h, src_first, count, j % src.ring.m))


def automorph_hint(ring: Ring, sk_crt: Buf, j: int, gadget: int = ALCH_GAD_TRIV, svar: float = 1.0, seed: int = 0) -> Buf:
    """The 2 * D elements (b_t, a_t) with b_t + a_t s = g_t sigma_j(s) + e_t: ks_hint for the one value sigma_j(s)."""
    v = ring.alloc(1)
    buf_automorph(v, sk_crt, j, 1)
    return ks_hint(ring, gadget, sk_crt, v, 1, svar, seed)


class Automorph:
    """alch_automorph: sigma_j on linear ciphertexts of `ring` at one key switch (the hint is copied: `ks_crt` may be reused)."""

    def __init__(self, ring: Ring, j: int, ks_crt: Buf, gadget: int = ALCH_GAD_TRIV):
        self.ring, self.j, self.gadget = ring, j % ring.m, gadget
        h = C.c_void_p()
        _check(ring._l.alch_automorph_create(ring._h, self.j, gadget, ks_crt._h, C.byref(h)))
        self._h = h

    def free(self):
        if getattr(self, "_h", None):
            if getattr(self.ring, "_h", None):                  # see Buf.free
                self.ring._l.alch_automorph_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def ct_automorph(auto: Automorph, ct: Buf, batch: int, s_pre=None, out: Buf | None = None, flags: int = 0, meta=None):
    """out[b] = keySwitch(sigma_j(ct[b])) for the `batch` linear ciphertexts (k = 0) of `ct`, CRT basis in and out; s_pre: toMSD's
    per-limb scalar.  Returns the result buffer (a new one unless `out` is given), or (buffer, meta) when a CtMeta is passed: sigma_j
    fixes Z_p and the call serves k = 0, so the record passes through unchanged (an encoding change made through s_pre is the
    caller's to record, as for a tunnel)."""
    if out is None:
        out = auto.ring.alloc(max(1, 2 * batch))
    sp = _pu64(s_pre) if s_pre is not None else None
    _check(auto.ring._l.alch_ct_automorph(auto._h, ct._h, out._h, batch, sp, flags))
    return out if meta is None else (out, meta)


# ---- hoisted automorphisms: several sigma_j of one batch at one gadget decomposition (include/alchemy_hip.h, "Hoisted automorphisms")
def automorph_set_hints(ring: Ring, sk_crt: Buf, js, gadget: int = ALCH_GAD_TRIV, svar: float = 1.0, seed: int = 0) -> Buf:
    """One buffer holding the len(js) hints one after the other, 2 * D elements each: hint r is automorph_hint(.., js[r], ..) on seed
    `seed + 2 r` (a hint draws from its seed and the next one)."""
    D = ring.gadget_digits(gadget)
    out = ring.alloc(max(1, 2 * D * len(js)))
    for r, j in enumerate(js):
        h = automorph_hint(ring, sk_crt, j % ring.m, gadget, svar, seed + 2 * r)
        out.copy_from(h, 2 * D, 2 * D * r, 0)
    return out


class AutomorphSet:
    """alch_automorph_set: up to 32 units with their hints (copied: `ks_crt` may be reused), for ct_automorph_hoisted."""

    def __init__(self, ring: Ring, js, ks_crt: Buf, gadget: int = ALCH_GAD_TRIV):
        self.ring, self.js, self.gadget = ring, [j % ring.m for j in js], gadget
        arr = (C.c_uint32 * max(1, len(js)))(*[j % (1 << 32) for j in js])
        h = C.c_void_p()
        _check(ring._l.alch_automorph_set_create(ring._h, len(js), arr, gadget, ks_crt._h, C.byref(h)))
        self._h = h

    def free(self):
        if getattr(self, "_h", None):
            if getattr(self.ring, "_h", None):                  # see Buf.free
                self.ring._l.alch_automorph_set_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def ct_automorph_hoisted(aset: AutomorphSet, ct: Buf, batch: int, s_pre=None, out: Buf | None = None, sum: bool = False, meta=None):
    """out[r * batch + b] = keySwitch(sigma_(j_r)(ct[b])) for every unit of the set at ONE decomposition of the batch; sum=True:
    out[b] = sum_r of those (ALCH_AUTO_SUM).  Linear ciphertexts (k = 0), CRT basis in and out; s_pre as in ct_automorph.  Returns the
    result buffer (a new one unless `out` is given), or (buffer, meta) when a CtMeta is passed (unchanged, as in ct_automorph)."""
    if out is None:
        out = aset.ring.alloc(max(1, 2 * batch * (1 if sum else len(aset.js))))
    sp = _pu64(s_pre) if s_pre is not None else None
    _check(aset.ring._l.alch_ct_automorph_hoisted(aset._h, ct._h, out._h, batch, sp, ALCH_AUTO_SUM if sum else 0))
    return out if meta is None else (out, meta)


# ---- weighted sums of hoisted rotations: the diagonals of a slot-wise linear map (include/alchemy_hip.h, "Weighted sums of hoisted rotations")
def ct_automorph_lincomb(aset: AutomorphSet, weights: Buf, ct: Buf, batch: int, n_out: int = 1, w_first: int = 0, s_pre=None,
                         out: Buf | None = None, meta=None):
    """out[g * batch + b] = sum_r weights[w_first + g R + r] (.) keySwitch(sigma_(j_r)(ct[b])), g < n_out, over the R units of the set
    at ONE decomposition of the batch: `weights` holds n_out * R public CRT-basis elements (canonical residues), read at call time.
    Linear ciphertexts (k = 0), CRT basis in and out; s_pre as in ct_automorph.  Returns the result buffer (a new one unless `out` is
    given), or (buffer, meta) when a CtMeta is passed (unchanged, as in ct_automorph_hoisted: a public product keeps k, l and p)."""
    if out is None:
        out = aset.ring.alloc(max(1, 2 * batch * n_out))
    sp = _pu64(s_pre) if s_pre is not None else None
    _check(aset.ring._l.alch_ct_automorph_lincomb(aset._h, weights._h, w_first, n_out, ct._h, out._h, batch, sp, 0))
    return out if meta is None else (out, meta)
