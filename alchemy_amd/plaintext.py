"""The plaintext half of the reference's acceptance check on device-resident batches (include/alchemy_hip.h, "plaintext ring
elements on resident batches": alch_pt_mul, alch_pt_linear_create, alch_pt_eval_lin, alch_pt_rescale, alch_buf_add_bcast).

The reference evaluates every example twice -- `eval` on plaintexts, `eval . pt2ct` on ciphertexts -- and compares
(examples/HomomRLWR.hs:64-75).  E's mul_, div2_ and linearCyc_ on `Cyc t m zp` (Eval.hs:65-67, 72-88, 136-148) run here on batches
of rings without a CRT basis (Ring(m, [p], nocrt=True)); products go through a lifting ring, any CRT ring of the same index, and
are exact as long as Q/2 exceeds coeff_bound (the library refuses the call otherwise)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .capi import ALCH_NOT_DIVISIBLE, Buf, Ring, _check, load_library


def coeff_bound(m: int, p: int, terms: int = 1) -> int:
    """alch_pt_bound: terms * phi(m) * 2^(odd primes of m) * (p // 2)^2, a bound on every integer coefficient of a `terms`-term sum of
    products of centred mod-p elements on the powerful basis of index m.  Host-only."""
    lo, hi = C.c_uint64(), C.c_uint64()
    _check(load_library().alch_pt_bound(m, C.c_uint64(p), terms, C.byref(lo), C.byref(hi)))
    return (int(hi.value) << 64) | int(lo.value)


def pt_mul(lift: Ring, dst: Buf, a: Buf, b: Buf, count: int):
    """dst[e] = a[e] * b[e] in Z_p[zeta_m] (Pow basis); dst may be a or b."""
    _check(load_library().alch_pt_mul(lift._h, dst._h, a._h, b._h, count, 0))


class PtLinear:
    """alch_ptlin: an E-linear function R_p -> S_p (`linearDec ys`), resident in the CRT basis of the lifting ring of index s."""

    def __init__(self, lift_s: Ring, ys: Buf, m_r: int):
        self.lift, self.m_r = lift_s, int(m_r)
        h = C.c_void_p()
        _check(load_library().alch_pt_linear_create(lift_s._h, ys._h, self.m_r, C.byref(h)))
        self._h = h

    def apply(self, src: Buf, dst: Buf, count: int):
        _check(load_library().alch_pt_eval_lin(self._h, src._h, dst._h, count, 0))

    def free(self):
        if getattr(self, "_h", None):
            load_library().alch_pt_linear_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def pt_linear(lift_s: Ring, ys: Buf, m_r: int) -> PtLinear:
    return PtLinear(lift_s, ys, m_r)


def pt_eval_lin(f: PtLinear, src: Buf, dst: Buf, count: int):
    """dst[b] = sum_i y_i * embed(coeffsDec(src[b])_i); src over index r, dst over index s, Pow basis."""
    f.apply(src, dst, count)


def pt_rescale(src: Buf, dst: Buf, count: int) -> bool:
    """div2_ = rescalePow to a modulus p' | p: dst = src / (p/p').  False when some coefficient was not divisible (dst then holds the
    floor quotients)."""
    return _check(load_library().alch_pt_rescale(src._h, dst._h, count)) != ALCH_NOT_DIVISIBLE


def add_bcast(dst: Buf, src: Buf, one: Buf, index: int, count: int):
    """dst[e] = src[e] + one[index] (addLit_ on a batch)."""
    _check(load_library().alch_buf_add_bcast(dst._h, src._h, one._h, index, count))


def tree_literals(p: int):
    """The leaves' literals z (1 - z), z = 1 .. p/4, of rescaleTreePow2 for p = 2^(k+1) (Language/RescaleTree.hs:69)."""
    return [z * (1 - z) for z in range(1, p // 4 + 1)]


def ring_round_plain(x: Buf, count: int, linears, lift: Ring, p: int, tree: bool = True):
    """`eval ringRound` on a resident batch (examples/HomomRLWR.hs:45-50,67), the plaintext twin of alchemy_amd.ringround: the hops
    `linears` (PtLinear, applied in order to x, a batch over the first hop's source index), then rescaleTreePow2 over the last index
    m -- y = x (1 + x), the leaves div2 (y + z_j), and pairwise products each followed by div2 down to Z_2.  `lift`: the lifting ring
    of index m.  tree=False stops after y.  Returns (result buffer, every div2 operand was even)."""
    cur = x
    for f in linears:
        nxt = Ring(f.lift.m, [p], nocrt=True).alloc(count)
        f.apply(cur, nxt, count)
        cur = nxt
    r = cur.ring
    assert r.m == lift.m and r.qs == [p]
    zs = tree_literals(p) if tree else []
    lits = np.zeros((1 + len(zs), r.n, 1), dtype=np.int64)
    lits[0, 0, 0] = 1
    for j, z in enumerate(zs):
        lits[1 + j, 0, 0] = z % p
    lit = r.upload(lits)
    y = r.alloc(count)
    add_bcast(y, cur, lit, 0, count)
    pt_mul(lift, y, cur, y, count)
    if not tree:
        return y, True
    even, mod = True, p // 2
    half = Ring(r.m, [mod], nocrt=True)
    t, tmp = [], r.alloc(count)
    for j in range(len(zs)):
        add_bcast(tmp, y, lit, 1 + j, count)
        h = half.alloc(count)
        even &= pt_rescale(tmp, h, count)
        t.append(h)
    while len(t) > 1:
        mod //= 2
        nxt_ring = Ring(r.m, [mod], nocrt=True)
        nx = []
        for i in range(0, len(t) - 1, 2):
            pt_mul(lift, t[i], t[i], t[i + 1], count)
            h = nxt_ring.alloc(count)
            even &= pt_rescale(t[i], h, count)
            nx.append(h)
        t = nx
    return t[0], even
