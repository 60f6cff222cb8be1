"""CPU: the identity behind tests/test_gpu_automorph_hoisted.py restated in Python integers, so that the GPU test's reference does not
rest on the library alone.  No library call: the oracle's by-definition crt / crtInv (oracle/model_gen.py), the slot table restated from
the header's rule (tests/automorph_model.py), and the two gadget decompositions written out below.

    hoisted_j(ct).c0[k] = s_pre c0[src_j[k]] + sum_t crt(d_t)[src_j[k]] b_t[k],   .c1[k] = sum_t crt(d_t)[src_j[k]] a_t[k]
    d_t = the gadget digits of s_pre c1 (decomposed ONCE, before any permutation)

  identity:   hoisted_j(ct) under the hint h  =  sigma_j( keySwitch(ct) under the hint sigma_(1/j) h ),  every unit j, both gadgets
  corollary:  on a two-power ring with TrivGad, hoisted_j(ct) = keySwitch(sigma_j ct) under h -- alch_ct_automorph's definition --
              because sigma_j permutes the powerful-basis coefficients up to sign and the centred lift is odd for odd q
  j = 1:      both sides are keySwitch(ct) for every gadget."""
import random

import pytest

import automorph_model as M
from helpers import primes_1_mod
from oracle import model_gen as G


def decompose(x_pow, qs, gadget):
    """Digits of a Pow-basis element given per limb ([L][n] residues): each digit a list [L][n], reduced into every limb.
    triv: digit i is the centred lift of limb i.  base2: per limb the centred lift in balanced binary digits, least significant first,
    remainder 1 taken as -1, the top digit absorbing the rest (Lol's divModCent), ceil(log2 q_i) digits; limb 0's digits first."""
    out = []
    for i, q in enumerate(qs):
        v = [x - q if x > (q - 1) // 2 else x for x in x_pow[i]]
        if gadget == "triv":
            out.append([[c % p for c in v] for p in qs])
            continue
        kd = (q - 1).bit_length()
        for t in range(kd):
            if t + 1 < kd:
                d = [-(c & 1) for c in v]
                v = [(c - e) // 2 for c, e in zip(v, d)]
            else:
                d = v
            out.append([[c % p for c in d] for p in qs])
    return out


def gadget_check(x_pow, qs, gadget):
    """sum_t g_t d_t = x on every limb: g_t = 1 (triv) or 2^t on the digit's own limb, 0 on the others."""
    digs = decompose(x_pow, qs, gadget)
    t = 0
    for i, q in enumerate(qs):
        kd = 1 if gadget == "triv" else (q - 1).bit_length()
        acc = [0] * len(x_pow[i])
        for s in range(kd):
            acc = [(a + (1 << s if gadget == "base2" else 1) * d) % q for a, d in zip(acc, digs[t + s][i])]
        assert acc == x_pow[i]
        t += kd
    assert t == len(digs)
    return digs


def digits_crt(c1, s_pre, idx, qs, gadget):
    """crt of the digits of s_pre c1, per digit [L][n]."""
    pw = [G.crtinv_def([x * s % q for x in c1[l]], idx, q) for l, (q, s) in enumerate(zip(qs, s_pre))]
    return [[G.crt_def(d[l], idx, q) for l, q in enumerate(qs)] for d in gadget_check(pw, qs, gadget)]


def key_switch(ct, hint, s_pre, idx, qs, gadget):
    """(s_pre c0, 0) + sum_t crt(d_t) (b_t, a_t): the tunnel from the ring to itself with lin = crt(1)."""
    c0, c1 = ct
    dc = digits_crt(c1, s_pre, idx, qs, gadget)
    assert 2 * len(dc) == len(hint)
    n = idx.n
    o0 = [[(c0[l][k] * s_pre[l] + sum(d[l][k] * hint[2 * t][l][k] for t, d in enumerate(dc))) % q for k in range(n)] for l, q in enumerate(qs)]
    o1 = [[sum(d[l][k] * hint[2 * t + 1][l][k] for t, d in enumerate(dc)) % q for k in range(n)] for l, q in enumerate(qs)]
    return o0, o1


def hoisted(ct, hint, s_pre, idx, qs, gadget, src):
    c0, c1 = ct
    dc = digits_crt(c1, s_pre, idx, qs, gadget)
    n = idx.n
    o0 = [[(c0[l][src[k]] * s_pre[l] + sum(d[l][src[k]] * hint[2 * t][l][k] for t, d in enumerate(dc))) % q for k in range(n)]
          for l, q in enumerate(qs)]
    o1 = [[sum(d[l][src[k]] * hint[2 * t + 1][l][k] for t, d in enumerate(dc)) % q for k in range(n)] for l, q in enumerate(qs)]
    return o0, o1


def perm(elem, src):
    return [[limb[s] for s in src] for limb in elem]


def setup(m, gadget, seed):
    idx = G.Index(m)
    qs = primes_1_mod(m, 2, 1 << 9)
    rnd = random.Random(seed)
    D = len(qs) if gadget == "triv" else sum((q - 1).bit_length() for q in qs)
    elem = lambda: [[rnd.randrange(q) for _ in range(idx.n)] for q in qs]
    ct = (elem(), elem())
    hint = [elem() for _ in range(2 * D)]
    return idx, qs, ct, hint


@pytest.mark.parametrize("m", [16, 9])
@pytest.mark.parametrize("gadget", ["triv", "base2"])
@pytest.mark.parametrize("neg", [False, True])
def test_hoisted_is_sigma_of_the_key_switch_under_the_moved_hint(m, gadget, neg):
    idx, qs, ct, hint = setup(m, gadget, 100 + m)
    s_pre = [q - 1 for q in qs] if neg else [1] * len(qs)
    for j in M.units(m):
        src, src_inv = M.table(m, j), M.table(m, pow(j, -1, m))
        assert [src_inv[s] for s in src] == list(range(idx.n))
        moved = [perm(h, src_inv) for h in hint]                               # sigma_(1/j) of the hint for j
        want = tuple(perm(x, src) for x in key_switch(ct, moved, s_pre, idx, qs, gadget))
        assert hoisted(ct, hint, s_pre, idx, qs, gadget, src) == want, (m, gadget, j)
    # j = 1: the key switch itself
    assert hoisted(ct, hint, s_pre, idx, qs, gadget, list(range(idx.n))) == key_switch(ct, hint, s_pre, idx, qs, gadget)


@pytest.mark.parametrize("neg", [False, True])
def test_trivgad_on_a_two_power_ring_equals_permute_then_switch(neg):
    m = 16
    idx, qs, ct, hint = setup(m, "triv", 7)
    s_pre = [q - 1 for q in qs] if neg else [1] * len(qs)
    for j in M.units(m):
        src = M.table(m, j)
        rotated = (perm(ct[0], src), perm(ct[1], src))                         # (sigma_j c0, sigma_j c1)
        assert hoisted(ct, hint, s_pre, idx, qs, "triv", src) == key_switch(rotated, hint, s_pre, idx, qs, "triv"), j
        # why: sigma_j moves powerful-basis coefficients up to sign, and the centred lift commutes with a sign
        for l, q in enumerate(qs):
            pw = G.crtinv_def(ct[1][l], idx, q)
            assert G.crtinv_def(rotated[1][l], idx, q) == M.sigma_pow_twopower(pw, j, q)


def test_elsewhere_the_digits_differ_and_both_are_key_switches():
    """BaseBGad 2 on m = 16 and TrivGad on m = 9: decompose-then-permute and permute-then-decompose give different words for some unit
    (no equality with alch_ct_automorph is claimed there), yet the gadget identity holds for both, which is all a key switch needs."""
    for m, gadget in ((16, "base2"), (9, "triv")):
        idx, qs, ct, hint = setup(m, gadget, 11)
        s_pre = [1] * len(qs)
        differs = False
        for j in M.units(m):
            src = M.table(m, j)
            rotated = (perm(ct[0], src), perm(ct[1], src))
            differs = differs or hoisted(ct, hint, s_pre, idx, qs, gadget, src) != key_switch(rotated, hint, s_pre, idx, qs, gadget)
        assert differs, (m, gadget)
