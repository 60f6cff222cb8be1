"""PT2CT's mul_ one SHE operation at a time on device-resident ciphertext batches (include/alchemy_hip.h: alch_ct_mul,
alch_ct_key_switch_quad, alch_ct_mod_switch_deg).

PT2CT emits a multiplication as  modSwitch_ . keySwitchQuad_ hint . modSwitch_ $ x *: y  (Crypto/Alchemy/Interpreter/PT2CT.hs:160-177)
and the ErrorRateWriter logs an error rate after each of the four operations (ErrorRateWriter.hs:122,194,197).  The fused entry
points (alch_ct_mul_relin, alch_ct_mul_full) never let the quadratic ciphertext exist; these do: quadratic ciphertext b of a buffer
is elements (3b, 3b+1, 3b+2) = (c0, c1, c2), the layout error_rates / decrypt_batch read for degree = 2."""
from __future__ import annotations

from .capi import ALCH_POW_IN, ALCH_POW_OUT, Buf, Hint, Ring, _check, _pu64, load_library
from .decrypt import error_rates


def ct_mul(a: Buf, b: Buf, batch: int, s_pre=None, flags: int = 0, out: Buf | None = None) -> Buf:
    """SymmSHE (*) on linear ciphertexts: out[b] = s_pre * mulG(a[b] (x) b[b]), a quadratic ciphertext (a new buffer of 3 * batch
    elements unless `out` is given).  CRT basis in and out unless ALCH_POW_IN / ALCH_POW_OUT; the operands are left untouched."""
    ring = a.ring
    if out is None:
        out = ring.alloc(max(1, 3 * batch))
    sp = _pu64(s_pre) if s_pre is not None else None
    _check(load_library().alch_ct_mul(ring._h, a._h, b._h, out._h, batch, sp, flags))
    return out


def key_switch_quad(hint: Hint, cts: Buf, batch: int, s_pre=None, flags: int = 0, out: Buf | None = None) -> Buf:
    """keySwitchQuadCirc hint on quadratic ciphertexts of the hint's ring: (c0, c1) + sum_d crt(digit_d(c2)) * hint_d, everything
    times toMSD's per-limb scalar `s_pre` first.  Returns linear ciphertexts (2 * batch elements)."""
    if out is None:
        out = hint.ring.alloc(max(1, 2 * batch))
    sp = _pu64(s_pre) if s_pre is not None else None
    _check(load_library().alch_ct_key_switch_quad(hint._h, cts._h, out._h, batch, sp, flags))
    return out


def mod_switch(cts: Buf, ring_out: Ring, batch: int, degree: int = 1, flags: int = 0, out: Buf | None = None) -> Buf:
    """SymmSHE modSwitch of ciphertexts of degree 1 or 2 to `ring_out` (more limbs: up; fewer: down, c0 on the decoding basis and
    every higher component on the powerful basis)."""
    if out is None:
        out = ring_out.alloc(max(1, (degree + 1) * batch))
    _check(load_library().alch_ct_mod_switch_deg(cts._h, out._h, batch, degree, flags))
    return out


def mul_steps(hint: Hint, a: Buf, b: Buf, ring_in: Ring, ring_h: Ring, ring_out: Ring, sk_by_ring=None, batch: int | None = None,
              s_pre=None, p: int | None = None, flags: int = 0):
    """PT2CT's four steps of one mul_ on a resident batch: (*) on ring_in, modSwitch_ to ring_h (skipped when ring_h is ring_in),
    keySwitchQuad_ hint, modSwitch_ to ring_out (skipped when ring_out is ring_h).
    s_pre: the operands' toLSD scalars, folded into (*).  p: the plaintext modulus; the product is then taken to be in LSD form, as
    SymmSHE's (*) leaves it, toMSD's scalar p^-1 is applied where the next step needs the MSD form (alch_buf_scale before a
    modSwitch_, keySwitchQuad_'s own scalar otherwise), and the rates of MSD ciphertexts are taken after toLSD's scalar p, as
    errorTermUnrestricted takes them.  p = None: no encoding scalar anywhere.  flags: ALCH_POW_OUT for the result.
    With p^-1 as s_pre, alch_ct_mul_full computes the same words in one call.

    sk_by_ring: {ring: Buf holding the secret key in that ring's CRT basis (element 0)} for ring_in, ring_h and ring_out.  With it
    the result comes with the ErrorRateWriter's log for the batch,
        [("mul_", rates), ("modSwitch_", rates), ("keySwitchQuad_", rates), ("modSwitch_", rates)],
    rates = alchemy_amd.error_rates of every ciphertext after that step (degree 2 for the first two entries); a skipped
    modSwitch_ logs the rates of the ciphertexts it passes on unchanged."""
    if a.ring is not ring_in or b.ring is not ring_in or hint.ring is not ring_h:
        raise ValueError("mul_steps: a and b belong to ring_in, the hint to ring_h")
    batch = a.n_elems // 2 if batch is None else batch
    pow_out = flags & ALCH_POW_OUT
    log = []

    def rate(name, cts, degree, msd, pow_basis=False):
        if sk_by_ring is not None:
            to_lsd = [p % q for q in cts.ring.qs] if (msd and p is not None) else None
            log.append((name, error_rates(cts, batch, sk_by_ring[cts.ring], degree=degree, s_pre=to_lsd,
                                          flags=ALCH_POW_IN if pow_basis else 0)))

    to_msd = [pow(p, -1, q) for q in ring_in.qs] if p is not None else None
    quad = ct_mul(a, b, batch, s_pre)
    rate("mul_", quad, 2, False)
    switched = ring_h is not ring_in
    if switched:
        if to_msd is not None:
            quad.scale(quad, 3 * batch, to_msd)
        quad = mod_switch(quad, ring_h, batch, degree=2)
    rate("modSwitch_", quad, 2, switched)
    last = ring_out is ring_h
    lin = key_switch_quad(hint, quad, batch, s_pre=None if switched else to_msd, flags=pow_out if last else 0)
    rate("keySwitchQuad_", lin, 1, True, bool(last and pow_out))
    if not last:
        lin = mod_switch(lin, ring_out, batch, degree=1, flags=pow_out)
    rate("modSwitch_", lin, 1, True, bool(pow_out))
    return (lin, log) if sk_by_ring is not None else lin
