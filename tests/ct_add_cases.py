"""Model instances shared by tests/test_ct_add_host.py and tests/test_gpu_ct_add.py: valid SymmSHE ciphertexts from oracle/model_gen.py
whose sums need every kind of alignment (encoding, g-power, Z_p scalar, degree), and the word-level formula of alch_ct_add in pure
Python on the Pow basis,

    out_i = s_a mulG^g_a (a_i) + s_b mulG^g_b (b_i)   (mod q_j),   a missing c2 = 0.

Built once per ring (lru_cache) and never modified."""
import functools
import math
import random

from alchemy_amd.ctadd import CtMeta
from helpers import primes_1_mod
from oracle import model_gen as G

RINGS = [(32, 16, 8), (45, 9, 7), (27, 3, 5)]                       # (m', m, p)


def meta_of(ct) -> CtMeta:
    return CtMeta(ct.enc, ct.k, ct.l, ct.p, len(ct.c) - 1)


def bump_k(ct, t):
    """The same plaintext with g-power k + t: every component times g^t (decrypt divides it out again)."""
    c = ct.c
    for _ in range(t):
        c = [[G.mulg_pow_def(cl, ct.big, q) for cl, q in zip(comp, ct.qs)] for comp in c]
    return G.GCT(ct.enc, ct.k + t, ct.l, c, ct.p, ct.qs, ct.big, ct.small)


def with_l(ct, v):
    """The same polynomial with l multiplied by the unit v: decrypts to v * plaintext."""
    return G.GCT(ct.enc, ct.k, ct.l * v % ct.p, ct.c, ct.p, ct.qs, ct.big, ct.small)


def pt_scale(pt, v, p):
    return [x * v % p for x in pt]


def term(ct, s, g):
    """s * mulG^g of every component, limb-major Pow words."""
    out = []
    for comp in ct.c:
        limbs = []
        for j, (cl, q) in enumerate(zip(comp, ct.qs)):
            for _ in range(g):
                cl = G.mulg_pow_def(cl, ct.big, q)
            sj = 1 if s is None else s[j]
            limbs.append([v * sj % q for v in cl])
        out.append(limbs)
    return out


def formula(ct_a, s_a, g_a, ct_b, s_b, g_b):
    """Components of s_a g^g_a a + s_b g^g_b b (ct_b None: the unary form)."""
    ta = term(ct_a, s_a, g_a)
    if ct_b is None:
        return ta
    tb = term(ct_b, s_b, g_b)
    out = []
    for i in range(max(len(ta), len(tb))):
        if i >= len(ta):
            out.append(tb[i])
        elif i >= len(tb):
            out.append(ta[i])
        else:
            out.append([[(u + v) % q for u, v in zip(al, bl)] for al, bl, q in zip(ta[i], tb[i], ct_a.qs)])
    return out


def as_gct(comps, meta, like):
    return G.GCT(meta.enc, meta.k, meta.l, comps, meta.p, like.qs, like.big, like.small)


@functools.lru_cache(maxsize=None)
def instances(mp, m, p):
    """(sk, cases): cases = [(name, ct_a, pt_a, ct_b, pt_b)], plaintexts as Pow coefficients mod p of the index m."""
    rng = random.Random(mp * 1000 + m * 10 + p)
    small, big = G.Index(m), G.Index(mp)
    qs = primes_1_mod(mp, 3, 1 << 29)
    sk = G.g_gen_sk(big, rng)
    pts = [[rng.randrange(p) for _ in range(small.n)] for _ in range(4)]
    x, y, z, w = pts
    cx, cy, cz, cw = [G.g_encrypt(sk, t, small, big, p, qs, rng) for t in pts]
    xy, zw, xx = G.g_ct_mul(cx, cy), G.g_ct_mul(cz, cw), G.g_ct_mul(cx, cx)
    pxy, pzw, pxx = [G.ring_mul_def(u, v, small, p) for u, v in ((x, y), (z, w), (x, x))]
    units = [v for v in range(2, p) if math.gcd(v, p) == 1]
    v1, v2 = units[0], units[-1]
    # modSwitch down one limb, back to LSD: l picks up (-Q)(-Q')^-1; the partner is a fresh encryption on the remaining limbs
    down = G.g_to_lsd(G.g_mod_switch_down(G.g_to_msd(cx), 1))
    fresh2 = G.g_encrypt(sk, z, small, big, p, qs[1:], rng)
    cases = [
        ("fresh+fresh", cx, x, cz, z),                                             # LSD/LSD, k (0,0), degree (1,1)
        ("xy+z", xy, pxy, cz, z),                                                  # LSD/LSD, k (1,0), degree (2,1)
        ("z+toMSD(xy)", cz, z, G.g_to_msd(xy), pxy),                               # LSD/MSD, k (0,1), degree (1,2)
        ("toMSD(z),xy", G.g_to_msd(cz), z, xy, pxy),                               # MSD/LSD, k (0,1), degree (1,2)
        ("toMSD(xy)+toMSD(zw)", G.g_to_msd(xy), pxy, G.g_to_msd(zw), pzw),         # MSD/MSD, k (1,1), degree (2,2)
        ("g^2 x+z", bump_k(cx, 2), x, cz, z),                                      # k (2,0), degree (1,1)
        ("l-scaled", with_l(cx, v1), pt_scale(x, v1, p), with_l(cz, v2), pt_scale(z, v2, p)),
        ("l-scaled xy, toMSD(z)", with_l(xy, v2), pt_scale(pxy, v2, p), G.g_to_msd(with_l(cz, v1)), pt_scale(z, v1, p)),
        ("modSwitch", down, x, fresh2, z),                                         # l = (-Q)(-Q')^-1 against 1, two limbs
        ("x*x+b", xx, pxx, cw, w),
    ]
    return sk, cases
