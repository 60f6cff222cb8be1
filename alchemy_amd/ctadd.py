"""SymmSHE (+), (-) and negate on device-resident ciphertext batches whose operands are not aligned (include/alchemy_hip.h:
alch_ct_add).

add_ = pureE (+) and neg_ = pureE negate (Crypto/Alchemy/Interpreter/Eval.hs:59-60, PT2CT.hs:117-118).  SymmSHE's (+) owes its operands
an alignment: the g-power k, the Z_p scalar l, the MSD / LSD encoding and the degree.  `align` is that rule on the metadata alone
(host-only, no library call); the device applies its result -- two per-limb scalars and two g-powers -- in one element-wise pass.

Conventions (oracle/model_gen.py): a ciphertext with metadata (enc, k, l) decrypts to l * g^-k * c(s) mod p in its LSD form; toMSD
multiplies every limb by p^-1 mod q_j and l by -Q mod p, Q = the product of the moduli."""
from __future__ import annotations

from dataclasses import dataclass

from .capi import Buf, _check, _pu64, load_library

LSD, MSD = "LSD", "MSD"


@dataclass(frozen=True)
class CtMeta:
    """What SymmSHE's CT carries beside its polynomial: encoding ("LSD" / "MSD", the model's spellings), g-power k, Z_p scalar l, plaintext modulus p,
    degree (1: (c0, c1); 2: (c0, c1, c2))."""
    enc: str
    k: int
    l: int
    p: int
    degree: int = 1


def _centred(x: int, p: int) -> int:
    """The representative of x mod p in [-p/2, p/2)."""
    x %= p
    return x - p if 2 * x >= p else x


def align(meta_a: CtMeta, meta_b: CtMeta, qs, sub: bool = False):
    """(s_a, g_a, s_b, g_b, meta_out) with  a + b  (a - b with `sub`)  =  s_a g^g_a a + s_b g^g_b b  under meta_out:
      encoding  equal encodings are kept; otherwise the LSD operand goes to MSD (scalar p^-1 mod q_j, l <- l (-Q) mod p)
      g-power   K = max(k_a, k_b); operand x is multiplied by g^(K - k_x)
      l         the result keeps l_a; b is multiplied by the integer u = centred(l_b l_a^-1 mod p), negated for a subtraction
      degree    the larger one; a missing c2 counts as zero
    s_x is a list of residues, one per modulus of qs, or None where the scalar is 1."""
    if meta_a.p != meta_b.p:
        raise ValueError("align: the operands have different plaintext moduli")
    for m in (meta_a, meta_b):
        if m.enc not in (LSD, MSD) or m.degree not in (1, 2) or m.k < 0:
            raise ValueError(f"align: malformed metadata {m}")
    p, qs = meta_a.p, [int(q) for q in qs]
    Q = 1
    for q in qs:
        Q *= q
    enc = meta_a.enc if meta_a.enc == meta_b.enc else MSD

    def to_enc(m):
        """(multiply by p^-1?, l in the common encoding)"""
        if m.enc == enc:
            return False, m.l % p
        return True, m.l * ((-Q) % p) % p

    msd_a, l_a = to_enc(meta_a)
    msd_b, l_b = to_enc(meta_b)
    K = max(meta_a.k, meta_b.k)
    u = _centred(l_b * pow(l_a, -1, p), p)
    if sub:
        u = -u

    def scalar(to_msd, z):
        if not to_msd and z == 1:
            return None
        return [(pow(p, -1, q) if to_msd else 1) * z % q for q in qs]

    out = CtMeta(enc, K, l_a, p, max(meta_a.degree, meta_b.degree))
    return scalar(msd_a, 1), K - meta_a.k, scalar(msd_b, u), K - meta_b.k, out


def ct_add_raw(out: Buf, batch: int, a: Buf, deg_a: int, s_a, g_a: int, b: Buf | None, deg_b: int, s_b, g_b: int, flags: int = 0):
    """alch_ct_add as the header states it: out = s_a g^g_a a + s_b g^g_b b (b None: the unary form); scalars are lists of residues
    or None."""
    _check(load_library().alch_ct_add(out._h, batch, a._h, deg_a, _pu64(s_a) if s_a is not None else None, g_a,
                                      b._h if b is not None else None, deg_b, _pu64(s_b) if s_b is not None else None, g_b, flags))


def ct_add(a: Buf, meta_a: CtMeta, b: Buf, meta_b: CtMeta, batch: int, flags: int = 0, out: Buf | None = None, sub: bool = False):
    """a + b on `batch` ciphertexts of one ring (a ciphertext of degree d is elements (d + 1) i .. (d + 1) i + d): the aligned sum
    and its metadata, (Buf, CtMeta).  flags: 0 = CRT basis in and out, ALCH_POW_IN | ALCH_POW_OUT = Pow basis in and out.  out: a
    buffer of the result's degree; it may be `a` or `b` when that operand has it.  The other operands are left untouched."""
    s_a, g_a, s_b, g_b, meta = align(meta_a, meta_b, a.ring.qs, sub)
    if out is None:
        out = a.ring.alloc(max(1, (meta.degree + 1) * batch))
    ct_add_raw(out, batch, a, meta_a.degree, s_a, g_a, b, meta_b.degree, s_b, g_b, flags)
    return out, meta


def ct_sub(a: Buf, meta_a: CtMeta, b: Buf, meta_b: CtMeta, batch: int, flags: int = 0, out: Buf | None = None):
    """a - b: ct_add with the sign folded into b's scalar."""
    return ct_add(a, meta_a, b, meta_b, batch, flags, out, sub=True)


def ct_neg(a: Buf, meta_a: CtMeta, batch: int, flags: int = 0, out: Buf | None = None):
    """negate: every component times -1 (the unary form of alch_ct_add); the metadata do not change."""
    if out is None:
        out = a.ring.alloc(max(1, (meta_a.degree + 1) * batch))
    ct_add_raw(out, batch, a, meta_a.degree, [q - 1 for q in a.ring.qs], 0, None, 0, None, 0, flags)
    return out, meta_a
