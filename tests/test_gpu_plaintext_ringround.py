"""GPU: the reference's acceptance check with BOTH halves resident (examples/HomomRLWR.hs:64-75), on the miniature indices of
tests/test_gpu_homomrlwr_mini.py (R = O_8 -> S = O_12, R' = O_40 -> S' = O_60, p = 8): `ring_round_plain` on a batch equals the
model's plaintext evaluation, and equals `decrypt_batch` of the device pipeline on encryptions of the same inputs."""
import math
import random

import numpy as np
import pytest

import alchemy_amd as A
from alchemy_amd import capi
from helpers import primes_1_mod, to_aos
from oracle import model_gen as G

pytestmark = pytest.mark.gpu

R_, S_, RP, SP, P, B = 8, 12, 40, 60, 8, 3


def up(ring, elems):
    return ring.upload(np.stack([to_aos(e) for e in elems]))


def zp_up(ring, elems):
    return ring.upload(np.asarray(elems, dtype=np.int64).reshape(len(elems), ring.n, 1))


def model_tree(y, idx, p):
    """rescaleTreePow2 on one plaintext (Language/RescaleTree.hs:64-87) with Python integers.  div2 takes the floor quotient, which is
    what alch_pt_rescale writes for an operand that is not even (the random y_i below are no CRT set, so some are odd): every word of
    the tree is defined and compared.  Returns (result, its modulus, every operand was even)."""
    even = [True]

    def div2(v, mod):
        even[0] = even[0] and all(c % 2 == 0 for c in v)
        return [c // 2 for c in v]
    t = [div2([(c + (z * (1 - z) if i == 0 else 0)) % p for i, c in enumerate(y)], p) for z in range(1, p // 4 + 1)]
    mod = p // 2
    while len(t) > 1:
        t = [div2(G.ring_mul_def(t[i], t[i + 1], idx, mod), mod) for i in range(0, len(t), 2)]
        mod //= 2
    return t[0], mod, even[0]


def test_plain_ring_round_equals_the_model_and_the_device_decryption():
    rng = random.Random(2026)
    T = G.tunnel_indices(R_, S_, RP, SP)
    p = P
    qs = primes_1_mod(RP * SP // math.gcd(RP, SP), 4, 1 << 29)
    q_ct = qs[1:]
    sk_in, sk_out = G.g_gen_sk(T.rp, rng), G.g_gen_sk(T.sp, rng)
    ys = [[rng.randrange(p) for _ in range(T.s.n)] for _ in range(T.r.n // T.e.n)]
    lin_q, thints = G.g_tunnel_hint(ys, T, p, sk_in, sk_out, qs, rng)
    qhint = G.g_ks_hint(sk_out, T.sp, qs, rng)
    secrets = [[rng.randrange(p) for _ in range(T.r.n)] for _ in range(B)]
    a_pub = [rng.randrange(p) for _ in range(T.r.n)]

    # ---- plaintext half, resident: x = s * a, the hop, x (1 + x), the tree
    zr = A.Ring(R_, [p], nocrt=True)
    lift_r, lift_s = A.Ring(R_, primes_1_mod(R_, 2, 1 << 30)), A.Ring(S_, primes_1_mod(S_, 2, 1 << 30))
    f = A.pt_linear(lift_s, zp_up(A.Ring(S_, [p], nocrt=True), ys), R_)
    x = zr.alloc(B)
    A.pt_mul(lift_r, x, zp_up(zr, secrets), zp_up(zr, [a_pub] * B), B)
    y_dev, _ = A.ring_round_plain(x, B, [f], lift_s, p, tree=False)
    res_dev, even = A.ring_round_plain(x, B, [f], lift_s, p)
    want_y, want_res = [], []
    for sv in secrets:
        t = G.eval_lin_dec(ys, G.linv_def(G.ring_mul_def(sv, a_pub, T.r, p), T.r, p), T.e, T.r, T.s, p)
        y = G.ring_mul_def(t, [(v + (1 if i == 0 else 0)) % p for i, v in enumerate(t)], T.s, p)
        want_y.append(y)
        want_res.append(model_tree(y, T.s, p))
    assert y_dev.download()[:, :, 0].tolist() == want_y
    assert res_dev.ring.qs == [want_res[0][1]] == [2]
    assert res_dev.download()[:, :, 0].tolist() == [w[0] for w in want_res]          # leaves, products and div2 chain, word for word
    assert even == all(w[2] for w in want_res)

    # ---- ciphertext half: the device pipeline of tests/test_gpu_homomrlwr_mini.py on encryptions of the same inputs
    cts = [G.g_encrypt(sk_in, sv, T.r, T.rp, p, q_ct, rng) for sv in secrets]
    R3, R4 = A.Ring(RP, q_ct), A.Ring(RP, qs)
    S4, S3, S2 = A.Ring(SP, qs), A.Ring(SP, q_ct), A.Ring(SP, qs[2:])
    lin = up(S4, lin_q); lin.crt()
    tks = up(S4, [e for hint_i in thints for pair in hint_i for e in pair]); tks.crt()
    tunnel = A.Tunnel(R4, S4, lin, tks)
    qh = up(S4, [e for pair in qhint for e in pair]); qh.crt()
    quad = S4.hint_from_buf(qh)
    c = up(R3, [e for ct in cts for e in ct.c]); c.crt()
    a_emb = G.embed_pow([G.centred(v, p) for v in a_pub], T.r, T.rp)
    pub = up(R3, [[[v % q for v in a_emb] for q in q_ct]]); pub.crt()
    x1 = R3.alloc(2 * B)
    x1.mul_public(c, pub, 0, 2 * B)
    x1.crtinv()
    x1.scale(x1, 2 * B, [pow(p, -1, q) for q in q_ct])
    x2 = R4.alloc(2 * B)
    capi.ct_mod_switch(x1, x2, B)
    yy = S4.alloc(2 * B)
    tunnel.apply(x2, yy, B, flags=capi.ALCH_POW_IN | capi.ALCH_POW_OUT)
    y3 = S3.alloc(2 * B)
    capi.ct_mod_switch(yy, y3, B, flags=capi.ALCH_POW_IN | capi.ALCH_POW_OUT)
    # the model's view of the same stages, for the (k, l) metadata of the result
    m1 = [G.g_mul_public(a_pub, ct) for ct in cts]
    m4 = [G.g_mod_switch_down(G.g_tunnel(lin_q, thints, G.g_mod_switch_up(ct, qs[:1]), T), 1) for ct in m1]
    one = [1] + [0] * (T.s.n - 1)
    m5 = [G.g_add_public(one, ct) for ct in m4]
    y3.scale(y3, 2 * B, [p % q for q in q_ct])
    lsd = G.g_to_lsd(m4[0])
    pub1 = G.embed_pow([G.centred(v * pow(lsd.l, -1, p) % p, p) for v in one], T.s, T.sp)
    pb = up(S3, [[[v % q for v in pub1] for q in q_ct]])
    y_lsd = S3.alloc(2 * B)
    y_lsd.scale(y3, 2 * B, [1] * len(q_ct))
    y3.add_public(pb, 0, B)
    y_lsd.crt(); y3.crt()
    z = S2.alloc(2 * B)
    capi.ct_mul_full(quad, y_lsd, y3, z, B, s_pre=[pow(p, -1, q) for q in q_ct])
    m6 = G.g_mod_switch_down(G.g_key_switch(qhint, G.g_mod_switch_up(G.g_ct_mul(G.g_to_lsd(m4[0]), m5[0]), qs[:1])), 2)
    m6l = G.g_to_lsd(m6)
    sk = up(S2, [[[v % q for v in sk_out] for q in qs[2:]]]); sk.crt()
    dec = A.decrypt_batch(z, B, sk, A.Ring(SP, [p], nocrt=True), A.Ring(S_, [p], nocrt=True), m6l.k, m6l.l,
                          s_pre=[p % q for q in qs[2:]])
    assert dec.download()[:, :, 0].tolist() == y_dev.download()[:, :, 0].tolist()        # the reference's PASS, both halves resident
