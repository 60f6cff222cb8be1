"""Slot-wise linear maps on device-resident ciphertext batches: an n x n matrix over Z_p applied to the CRT slots of the plaintexts
(include/alchemy_hip.h, "Weighted sums of hoisted rotations": alch_ct_automorph_lincomb).

The plaintext ring has index m | m' (m' the ciphertext ring's index) and a prime modulus p = 1 (mod m), so R_p splits into n = phi(m)
slots, slot(u) holding x(omega_m^u) in the header's slot order.  sigma_j moves slots, crt(sigma_j x)[slot(u)] = crt(x)[slot(u j)], so
with the diagonals a_j[slot(u)] = M[slot(u), slot(u j mod m)] the element sum_j a_j (.) sigma_j(x) has the slot vector M . slots(x).
With a subgroup `baby` of (Z/m)^* and one `giant` per coset every unit is h g exactly once, and

    sum_j a_j sigma_j(x) = sum_g sigma_g( sum_(h in baby) sigma_(1/g)(a_(h g)) (.) sigma_h(x) )

-- the inner sums are ONE alch_ct_automorph_lincomb call with a row per giant (the baby rotations are decomposed and accumulated once,
in registers), or the composition of older calls where that measured faster (rows_route), the outer sum is one alch_ct_automorph per
giant g != 1 and alch_ct_add.  slot_diagonals, unit_split and lift_unit are
host only; SlotLinear builds hints and weights on the device (set-up work, like every hint) and `apply` is the hot path."""
from __future__ import annotations

import math

import numpy as np

from .automorph import (Automorph, AutomorphSet, automorph_hint, automorph_set_hints, automorph_table, ct_automorph,
                        ct_automorph_hoisted, ct_automorph_lincomb)
from .capi import ALCH_BASIS_POW, ALCH_GAD_TRIV, Buf, Ring
from .ctadd import ct_add_raw

MAX_BABY = 32                                                    # units per alch_automorph_set
LINCOMB_ROWS = 4                                                 # rows per launch (kernel_lincomb.hpp; tests/test_gpu_slot_linear.py compares)


def rows_route(pow2_engine: bool, digits: int, limbs: int, n_rows: int) -> str:
    """Which way SlotLinear.apply makes its rows, from the measured table of DESIGN section 24 (profiles/slot_linear.jsonl; 64
    ciphertexts, four 31-bit limbs).  With as many digits as limbs (TrivGad) the lincomb call won every line, 1.2x to 3.5x, rows beyond
    LINCOMB_ROWS included.  With more digits (BaseBGad: the digit and hint reads dominate) it lost where the rows exceed one launch
    and every row block redoes the inner products (0.70x / 0.77x at 8 rows), and by 3-4 % at ONE row on the radix-16 engine; it won
    5-17 % at 4 rows on both engines and 8-13 % at one row on the general engine.  2 and 3 rows were not measured and go with 4."""
    if digits <= limbs:
        return "lincomb"
    if n_rows > LINCOMB_ROWS or (n_rows == 1 and pow2_engine):
        return "composition"
    return "lincomb"


def _units(m: int):
    return [j for j in range(1, m) if math.gcd(j, m) == 1] if m > 1 else [1]


def slot_diagonals(m: int, p: int, M) -> dict:
    """{j: a_j} for every unit j of Z/m: a_j[k] = M[k, src_j[k]] mod p with src_j = automorph_table(m, j), i.e.
    a_j[slot(u)] = M[slot(u), slot(u j mod m)].  M: n x n integers in the slot order of index m."""
    M = np.asarray(M, dtype=object)
    n = len(automorph_table(m, 1))
    if M.shape != (n, n):
        raise ValueError(f"slot_diagonals: M must be {n} x {n} for index {m}")
    out = {}
    for j in _units(m):
        src = automorph_table(m, j)
        out[j] = [int(M[k, int(src[k])]) % p for k in range(n)]
    return out


def unit_split(m: int, baby):
    """(baby, giant): `baby` reduced and sorted -- it must be a subgroup of (Z/m)^* of at most 32 elements -- and the smallest
    representative of each of its cosets, ascending (giant[0] = 1).  Every unit of Z/m is h g for exactly one (h, g)."""
    hs = sorted({int(h) % m for h in baby})
    if len(hs) > MAX_BABY:
        raise ValueError(f"unit_split: the baby set holds {len(hs)} units, a set takes at most {MAX_BABY}")
    if not hs or any(math.gcd(h, m) != 1 for h in hs):
        raise ValueError("unit_split: the baby set must consist of units mod m")
    hset = set(hs)
    if any(a * b % m not in hset for a in hs for b in hs):
        raise ValueError("unit_split: the baby set is not closed under multiplication mod m")
    giants, seen = [], set()
    for u in _units(m):                                          # ascending: the first unit of a new coset is its smallest
        if u not in seen:
            giants.append(u)
            seen.update(h * u % m for h in hs)
    return hs, giants


def lift_unit(j: int, m: int, m_big: int) -> int:
    """The smallest unit of Z/m_big that is congruent to j mod m (j a unit mod m; one exists for every m_big: a prime of m_big that
    divides m does not divide j, the others are avoided by Chinese remaindering).  With m | m_big, sigma_u restricts to sigma_j."""
    if math.gcd(j, m) != 1:
        raise ValueError("lift_unit: j must be a unit mod m")
    u = j % m
    while math.gcd(u, m_big) != 1:
        u += m
    return u


class SlotLinear:
    """The matrix M (n x n over Z_p, slot order of index m) as an operator on linear ciphertexts of `ring` (index m', m | m') whose
    plaintexts live in the ring of index m mod p.  sk: the secret key (CRT basis, one element); baby: a subgroup of (Z/m)^* of at
    most 32 units; gadget, svar, seed: as for automorph_set_hints."""

    def __init__(self, ring: Ring, m: int, p: int, M, sk: Buf, baby, gadget: int = ALCH_GAD_TRIV, svar: float = 1.0, seed: int = 0):
        if ring.m % m or (p - 1) % m:
            raise ValueError("SlotLinear: m must divide the ring's index and p must be 1 mod m")
        self.ring, self.m, self.p, self.gadget = ring, m, p, gadget
        self.baby, self.giant = unit_split(m, baby)
        R, G = len(self.baby), len(self.giant)
        D = ring.gadget_digits(gadget)
        self.route = rows_route(ring.m >= 32 and ring.m & (ring.m - 1) == 0, D, ring.L, G)
        lift = lambda j: lift_unit(j, m, ring.m)
        hints = automorph_set_hints(ring, sk, [lift(h) for h in self.baby], gadget, svar, seed)
        self.aset = AutomorphSet(ring, [lift(h) for h in self.baby], hints, gadget)
        self.autos = []                                          # one key switch per giant g != 1 (giant[0] = 1)
        for i, g in enumerate(self.giant[1:]):
            hint = automorph_hint(ring, sk, lift(g), gadget, svar, seed + 2 * (R + i))
            self.autos.append(Automorph(ring, lift(g), hint, gadget))
            hint.free()
        assert hints.n_elems == 2 * D * R
        hints.free()                                             # copied into the set at create time
        # the G R weights: row g, rotation h holds sigma_(1/g)(a_(h g)), slot vector a_(h g)[src_(1/g)[k]]
        diag = slot_diagonals(m, p, M)
        n = len(diag[1])
        slots = np.zeros((G * R, n, 1), dtype=np.int64)
        for gi, g in enumerate(self.giant):
            src = automorph_table(m, pow(g, -1, m))
            for hi, h in enumerate(self.baby):
                a = diag[h * g % m]
                slots[gi * R + hi, :, 0] = [a[int(src[k])] for k in range(n)]
        zp = Ring(m, [p])                                        # slots mod p -> powerful basis: p = 1 mod m, so R_p has a CRT basis
        pw = zp.upload(slots)
        pw.crtinv()
        pow_p = pw.download()[:, :, 0]
        centred = np.where(2 * pow_p >= p, pow_p - p, pow_p)     # embed(reduce(liftPow a)): mulPublic's convention
        small = Ring(m, ring.qs)
        sw = small.upload(np.stack([centred % q for q in ring.qs], axis=2))
        self.weights = ring.alloc(G * R)
        self.weights.embed_from(sw, G * R, ALCH_BASIS_POW)
        self.weights.crt()
        small.sync()
        ring.sync()
        pw.free()                                                # before their rings go
        sw.free()
        zp.close()
        small.close()

    def _rows_composed(self, ct: Buf, batch: int, s_pre) -> Buf:
        """The G rows from calls older than alch_ct_automorph_lincomb: the R rotations stored once, then a public product and a sum
        per (row, rotation).  Word for word the rows of the lincomb call."""
        R, G = len(self.baby), len(self.giant)
        rot = ct_automorph_hoisted(self.aset, ct, batch, s_pre=s_pre)
        rows, tmp = self.ring.alloc(2 * batch * G), self.ring.alloc(2 * batch)
        for g in range(G):
            row = rows.view(2 * batch * g, 2 * batch)
            for r in range(R):
                dst = row if r == 0 else tmp
                dst.mul_public(rot.view(2 * batch * r, 2 * batch), self.weights, g * R + r, 2 * batch)
                if r:
                    row.add(row, tmp, 2 * batch)
        return rows

    def apply(self, ct: Buf, batch: int, s_pre=None, route: str | None = None) -> Buf:
        """2 * batch elements: ciphertext b encrypts the plaintext whose slot vector is M . slots(pt_b).  `ct` as for
        ct_automorph_lincomb (k = 0, CRT basis); s_pre reaches the baby step only.  route: "lincomb" or "composition" for the rows
        (the same words either way); None takes self.route, the faster one by DESIGN section 24's table.  The result is a view of a
        fresh buffer."""
        route = self.route if route is None else route
        if route == "lincomb":
            rows = ct_automorph_lincomb(self.aset, self.weights, ct, batch, n_out=len(self.giant), s_pre=s_pre)
        elif route == "composition":
            rows = self._rows_composed(ct, batch, s_pre)
        else:
            raise ValueError("SlotLinear.apply: route is 'lincomb' or 'composition'")
        acc = rows.view(0, 2 * batch)
        for i, auto in enumerate(self.autos):
            moved = ct_automorph(auto, rows.view(2 * batch * (i + 1), 2 * batch), batch)
            ct_add_raw(acc, batch, acc, 1, None, 0, moved, 1, None, 0)
        return acc

    def free(self):
        for a in getattr(self, "autos", []):
            a.free()
        self.autos = []
        if getattr(self, "aset", None):
            self.aset.free()
            self.aset = None
        if getattr(self, "weights", None):
            self.weights.free()
            self.weights = None
