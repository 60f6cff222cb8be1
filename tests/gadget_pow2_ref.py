"""Test-side reference for the BaseBGad 2^w gadget (ALCH_GAD_BASEPOW2(w)): a numpy decomposition by Lol's divModCent, walked digit
after digit (not the closed form the kernels use), and the key-switch and tunnel compositions of helpers.py with the decomposition
passed in.  Pinned to oracle.model.decompose_baseb and helpers.decompose_base2 by tests/test_oracle_gadget_pow2.py."""
import math

import numpy as np


def digit_counts(qs, w):
    """k_i = ceil(ceil(log2 q_i) / w): the smallest k with 2^(w k) >= q_i."""
    return [-(-(q - 1).bit_length() // w) for q in qs]


def decompose_pow2(elem, qs, w):
    """BaseBGad 2^w decompose + reduce of one Pow-basis element ((n, L) residues), index-agnostic: per limb i the centred lift is split
    into k_i digits base b = 2^w, least significant first, remainders in [-b/2, b/2), the top digit absorbing the rest; limb 0's digits
    first; every digit is returned reduced into all limbs.  int64 holds every intermediate for q < 2^62."""
    out, b = [], 1 << w
    for i, q in enumerate(qs):
        v = np.asarray(elem)[:, i].astype(np.int64)
        v = np.where(v > (q - 1) // 2, v - q, v)
        k = digit_counts([q], w)[0]
        for t in range(k):
            if t + 1 < k:
                r = np.mod(v, b)                                   # in [0, b)
                d = np.where(2 * r >= b, r - b, r)
                v = (v - d) // b
            else:
                d = v
            out.append(np.ascontiguousarray(np.stack([np.mod(d, qj) for qj in qs], axis=1).astype(np.int64)))
    return out


def gadget_pow2(qs, w):
    """[(limb, exponent)] of every gadget entry in hint order: entry t of limb i is 2^(w t) on limb i, 0 elsewhere."""
    return [(i, t) for i, k in enumerate(digit_counts(qs, w)) for t in range(k)]


def mul_relin_pow2(ring, qs, w, hint_crt, a0, a1, b0, b1, s_pre=None, pow_out=False, mulg=False):
    """keySwitchQuadCirc hint (a * b) with a BaseBGad 2^w hint from the C restatement's primitives (helpers.oracle_mul_relin_base2 with
    the decomposition passed in).  ring: cref.Ring or cref.GenRing (mulg: the general index's mulG on the product)."""
    o = ring
    s = list(s_pre) if s_pre is not None else [1] * len(qs)
    g = (lambda x: o.mulg_crt(x)) if mulg else (lambda x: x)
    c0 = o.scale(g(o.mul(a0, b0)), s)
    c1 = o.scale(g(o.add(o.mul(a0, b1), o.mul(a1, b0))), s)
    c2 = o.scale(g(o.mul(a1, b1)), s)
    digs = decompose_pow2(o.crtinv(c2), qs, w)
    assert 2 * len(digs) == len(hint_crt)
    for i, d in enumerate(digs):
        dc = o.crt(d)
        c0 = o.add(c0, o.mul(dc, hint_crt[2 * i]))
        c1 = o.add(c1, o.mul(dc, hint_crt[2 * i + 1]))
    return (o.crtinv(c0), o.crtinv(c1)) if pow_out else (c0, c1)


def tunnel_pow2(oracle_lib, r_p, s_p, qs, w, lin_crt, ks_crt, c0, c1, s_pre=None, pow_out=False):
    """SymmSHE.tunnel on one linear ciphertext with a BaseBGad 2^w hint: helpers.oracle_tunnel with the decomposition passed in."""
    from oracle import model_gen as G
    e_p = math.gcd(r_p, s_p)
    ie, ir, isx = G.Index(e_p), G.Index(r_p), G.Index(s_p)
    Or, Os, Oe = oracle_lib.GenRing(r_p, qs), oracle_lib.GenRing(s_p, qs), oracle_lib.GenRing(e_p, qs)
    L = len(qs)
    s = list(s_pre) if s_pre is not None else [1] * L
    c0p, c1p = Or.scale(Or.crtinv(c0), s), Or.scale(Or.crtinv(c1), s)
    c0d = Or.linv(c0p)
    rows, emb = np.array(G.coeffs_indices(ie, ir)), np.array(G.embed_indices(ie, isx))
    acc0, acc1 = np.zeros((isx.n, L), dtype=np.int64), np.zeros((isx.n, L), dtype=np.int64)
    for i, row in enumerate(rows):
        x = np.zeros((isx.n, L), dtype=np.int64)
        x[emb] = Oe.l(np.ascontiguousarray(c0d[row]))
        acc0 = Os.add(acc0, Os.mul(Os.crt(x), lin_crt[i]))
        x1 = np.zeros((isx.n, L), dtype=np.int64)
        x1[emb] = c1p[row]
        digs = decompose_pow2(x1, qs, w)
        for t, d in enumerate(digs):
            dc = Os.crt(d)
            acc0 = Os.add(acc0, Os.mul(dc, ks_crt[(i * len(digs) + t) * 2]))
            acc1 = Os.add(acc1, Os.mul(dc, ks_crt[(i * len(digs) + t) * 2 + 1]))
    return (Os.crtinv(acc0), Os.crtinv(acc1)) if pow_out else (acc0, acc1)


# ---- the exact model (oracle.model) with the base passed in ------------------------------------------------------------------------
def model_hint_pow2(sk, qs, r, rng, w):
    """oracle.model.ks_quad_circ_hint with the gadget gadget_baseb(qs, 2^w)."""
    from oracle import model as M
    n = len(sk)
    sq = M.rns_reduce(sk, qs)
    s2 = M.rns_mul(sq, sq, qs)
    hint = M.KSHint("basepow2")
    for g in M.gadget_baseb(qs, 1 << w):
        e = M.rns_reduce(M.gaussian_poly(n, r, rng), qs)
        h1 = [[rng.randrange(q) for _ in range(n)] for q in qs]
        h0 = M.rns_add(M.rns_add(M.rns_scale(s2, g, qs), e, qs), M.rns_neg(M.rns_mul(h1, sq, qs), qs), qs)
        hint.h.append([h0, h1])
    return hint


def model_key_switch_pow2(hint, ct, w):
    """oracle.model.key_switch_quad_circ with decompose_baseb(c2, qs, 2^w)."""
    from oracle import model as M
    ct = M.to_msd(ct)
    assert len(ct.c) == 3
    qs = ct.qs
    digs = M.decompose_baseb(ct.c[2], qs, 1 << w)
    assert len(digs) == len(hint.h)
    c0, c1 = ct.c[0], ct.c[1]
    for d, (h0, h1) in zip(digs, hint.h):
        dr = M.rns_reduce(d, qs)
        c0 = M.rns_add(c0, M.rns_mul(dr, h0, qs), qs)
        c1 = M.rns_add(c1, M.rns_mul(dr, h1, qs), qs)
    return M.CT(M.MSD, ct.k, ct.l, [c0, c1], ct.p, qs)


def full_mul_pow2(oracle_lib, n, qs_h, l_in, l_out, w, hint_crt, a0, a1, b0, b1, s_pre=None, pow_out=False):
    """helpers.oracle_full_mul (two-power index, hint on at least as many limbs as the operands) with the BaseBGad 2^w decomposition."""
    L = len(qs_h)
    dup = L - l_in
    o_in, o_h = oracle_lib.Ring(n, qs_h[dup:]), oracle_lib.Ring(n, qs_h)
    s = list(s_pre) if s_pre is not None else [1] * l_in
    c = [o_in.mul(a0, b0), o_in.add(o_in.mul(a0, b1), o_in.mul(a1, b0)), o_in.mul(a1, b1)]
    c = [o_in.scale(x, s) for x in c]
    mult = 1
    for q in qs_h[:dup]:
        mult *= q
    up = []
    for x in c:
        scaled = o_in.scale(x, [mult % q for q in qs_h[dup:]])
        up.append(np.ascontiguousarray(np.concatenate([np.zeros((n, dup), dtype=np.int64), scaled], axis=1)))
    digs = decompose_pow2(o_h.crtinv(up[2]), qs_h, w)
    assert 2 * len(digs) == len(hint_crt)
    ks = [up[0], up[1]]
    for i, d in enumerate(digs):
        dc = o_h.crt(d)
        ks[0] = o_h.add(ks[0], o_h.mul(dc, hint_crt[2 * i]))
        ks[1] = o_h.add(ks[1], o_h.mul(dc, hint_crt[2 * i + 1]))
    out = []
    for x in ks:
        cur = o_h.crtinv(x)
        for k in range(L, l_out, -1):
            cur = oracle_lib.Ring(n, qs_h[L - k:]).rescale_drop0(cur)
        out.append(cur if pow_out else oracle_lib.Ring(n, qs_h[L - l_out:]).crt(cur))
    return out[0], out[1]


def full_mul_pow2_down(oracle_lib, n, qs_in, l_h, l_out, w, hint_crt, a0, a1, b0, b1, s_pre=None, pow_out=False, m=None):
    """helpers.oracle_full_mul_base2_down (hint on FEWER limbs than the operands; general index m) with the BaseBGad 2^w decomposition."""
    L = len(qs_in)
    ring = (lambda qs: oracle_lib.GenRing(m, qs)) if m else (lambda qs: oracle_lib.Ring(n, qs))
    o_in, o_h, o_out = ring(qs_in), ring(qs_in[L - l_h:]), ring(qs_in[L - l_out:])
    s = list(s_pre) if s_pre is not None else [1] * L
    c = [o_in.mul(a0, b0), o_in.add(o_in.mul(a0, b1), o_in.mul(a1, b0)), o_in.mul(a1, b1)]
    c = [o_in.scale(o_in.mulg_crt(x) if m else x, s) for x in c]

    def down(x_pow, l_from, l_to, dec):
        cur = ring(qs_in[L - l_from:]).linv(x_pow) if dec else x_pow
        for k in range(l_from, l_to, -1):
            cur = ring(qs_in[L - k:]).rescale_drop0(cur)
        return ring(qs_in[L - l_to:]).l(cur) if dec else cur

    dec0 = bool(m)
    low = [down(o_in.crtinv(x), L, l_h, dec0 and comp == 0) for comp, x in enumerate(c)]
    digs = decompose_pow2(low[2], qs_in[L - l_h:], w)
    assert 2 * len(digs) == len(hint_crt)
    ks = [o_h.crt(low[0]), o_h.crt(low[1])]
    for i, d in enumerate(digs):
        dc = o_h.crt(d)
        ks[0] = o_h.add(ks[0], o_h.mul(dc, hint_crt[2 * i]))
        ks[1] = o_h.add(ks[1], o_h.mul(dc, hint_crt[2 * i + 1]))
    out = []
    for comp, x in enumerate(ks):
        cur = down(o_h.crtinv(x), l_h, l_out, dec0 and comp == 0)
        out.append(cur if pow_out else o_out.crt(cur))
    return out[0], out[1]
