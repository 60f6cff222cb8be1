"""GPU: key-switch and tunnel hints generated on resident buffers -- alch_ct_ks_hint / alch_ct_ks_hint_part (k_ct_ks_hint,
alchemy_amd/csrc/kernel_rlwe.hpp) against Python integers word for word, and ks_quad_circ_hint / tunnel_hint (alchemy_amd/hints.py)
closed by the operations they exist for: a product relinearised with the generated hint decrypts to the product of the plaintexts, a
batch tunnelled with the generated hints decrypts to f of the plaintexts.

On the parent commit the package has no `hints` module: this module does not import there."""
import numpy as np
import pytest

import alchemy_amd as A
import gauss_model as GM
from alchemy_amd import capi
from alchemy_amd import encrypt as E
from alchemy_amd import hints as H
from helpers import assert_reduced, primes_1_mod, primes_below, to_aos
from oracle import model_gen as G

pytestmark = pytest.mark.gpu

TRIV, BASE2 = capi.ALCH_GAD_TRIV, capi.ALCH_GAD_BASE2


def gadget_entries(qs, gadget):
    """[(limb, exponent)] of every gadget entry, in the order of alch_hint_load."""
    if gadget == TRIV:
        return [(i, 0) for i in range(len(qs))]
    return [(i, d) for i, q in enumerate(qs) for d in range((q - 1).bit_length())]


def ints(a):
    return np.asarray(a).astype(object)


def expected_pairs(qs, gadget, v, err, s, uni_odd):
    """Python integers, CRT basis (the ring product is slot-wise): [(b, a)] for every value of v ((n_v, n, L)) and gadget entry;
    err (n_v D, n, L), s (n, L), uni_odd(e) -> the (n, L) uniform words of entry e."""
    ent, q = gadget_entries(qs, gadget), ints(qs)
    out = []
    for i in range(v.shape[0]):
        for t, (limb, d) in enumerate(ent):
            e = i * len(ent) + t
            a = ints(uni_odd(e))
            g = np.zeros(len(qs), dtype=object)
            g[limb] = 1 << d
            out.append(((ints(err[e]) - a * ints(s) + g * ints(v[i])) % q, a))
    return out


def same(got, want):
    return np.array_equal(ints(got), want)


@pytest.mark.parametrize("gadget", [TRIV, BASE2])
@pytest.mark.parametrize("word", [32, 64])
@pytest.mark.parametrize("m", [16, 64, 21, 45])
def test_ct_ks_hint_equals_python_integers(m, word, gadget):
    qs = primes_1_mod(m, 2, 1 << 29) if word == 32 else primes_below(m, 2, 1 << 62)
    D = check_ks_hint(m, qs, gadget)
    if (m, word, gadget) == (45, 64, BASE2):
        assert D == 124


def upload_words(words, seed, bufs, qs):
    """Replace what fill_uniform wrote: words(rng, count, n, qs) for every buffer of bufs."""
    rng = np.random.default_rng(seed)
    for b in bufs:
        b.upload(words(rng, b.n_elems, b.ring.n, qs))


def check_ks_hint(m, qs, gadget, words=None, word_bytes=None):
    """alch_ct_ks_hint with n_v = 2 and a nonzero offset on every buffer against expected_pairs; returns the digit count D.
    words(rng, count, n, qs): the values, error terms and key (default: alch_buf_fill_uniform)."""
    ring = A.Ring(m, qs)
    assert word_bytes is None or ring.word_bytes == word_bytes
    D = ring.gadget_digits(gadget)
    assert D == len(gadget_entries(qs, gadget))
    n_v, out_first, v_first, err_first, sk_index, ct0, seed = 2, 3, 1, 2, 1, 3, 0xA5A5 + m
    total = n_v * D
    out, v, err, sk = ring.alloc(out_first + 2 * total), ring.alloc(v_first + n_v), ring.alloc(err_first + total), ring.alloc(2)
    uni = ring.alloc(2 * (ct0 + total))
    out.fill_uniform(1); v.fill_uniform(2); err.fill_uniform(3); sk.fill_uniform(4); uni.fill_uniform(seed)
    if words is not None:
        upload_words(words, m + gadget, (v, err, sk), qs)
    keep = out.download(0, out_first)
    H.ct_ks_hint(out, gadget, n_v, v, err, sk, seed, out_first=out_first, v_first=v_first, err_first=err_first, sk_index=sk_index, ct0=ct0)
    got, u = out.download(), uni.download()
    assert_reduced(got, qs)
    assert np.array_equal(got[:out_first], keep)
    want = expected_pairs(qs, gadget, v.download()[v_first:], err.download()[err_first:], sk.download()[sk_index],
                          lambda e: u[2 * (ct0 + e) + 1])
    for e, (b, a) in enumerate(want):
        assert same(got[out_first + 2 * e + 1], a), (m, e)
        assert same(got[out_first + 2 * e], b), (m, e)
    return D


def check_cut(m, qs, gadget, n_v, cut, words=None):
    """One call against two parts cut at entry `cut`, with ct0 advanced, in another buffer behind an offset."""
    ring = A.Ring(m, qs)
    D = ring.gadget_digits(gadget)
    total, ct0, seed = n_v * D, (1 << 64) - 2, 0xC07 + m                 # the pair counter wraps mod 2^64 inside the hint
    assert 0 < cut < total
    whole, parts, v, err, sk = ring.alloc(2 * total), ring.alloc(1 + 2 * total), ring.alloc(n_v), ring.alloc(total), ring.alloc(1)
    v.fill_uniform(5); err.fill_uniform(6); sk.fill_uniform(7); parts.fill_uniform(8)
    if words is not None:
        upload_words(words, m + cut, (v, err, sk), qs)
    H.ct_ks_hint(whole, gadget, n_v, v, err, sk, seed, ct0=ct0)
    H.ct_ks_hint_part(parts, gadget, 0, cut, v, err, sk, seed, out_first=1, ct0=ct0)
    H.ct_ks_hint_part(parts, gadget, cut, total - cut, v, err, sk, seed, out_first=1 + 2 * cut, err_first=cut, ct0=ct0 + cut)
    one = whole.download()
    assert np.array_equal(parts.download(1), one)
    return ring, one, v, err, sk, seed, ct0


def test_ct_ks_hint_in_two_parts_is_word_identical():
    m, qs = 21, primes_1_mod(21, 2, 1 << 29)
    D = sum((q - 1).bit_length() for q in qs)
    assert (D + 5) % D != 0
    check_cut(m, qs, BASE2, 2, D + 5)                                    # the cut falls inside value 1, inside limb 0's digits
    check_cut(m, qs, BASE2, 2, D - 3)                                    # inside value 0, inside limb 1's digits
    check_cut(m, primes_below(m, 2, 1 << 62), TRIV, 3, 1)


def test_ct_ks_hint_at_a_split_size():
    m = 1 << 17                                                          # n = 2^16: the largest 32-bit ring, 16-byte packs
    qs = primes_1_mod(m, 1, 1 << 29)
    ring, one, v, err, sk, seed, ct0 = check_cut(m, qs, TRIV, 3, 1)
    q, n = np.uint64(qs[0]), ring.n
    vv, ee, ss = (b.download()[..., 0] for b in (v, err, sk))
    for e in range(3):
        pos = (seed + (2 * (ct0 + e) + 1) * n) % (1 << 64)
        with np.errstate(over="ignore"):
            a = (GM.splitmix64(np.uint64(pos) + np.arange(n, dtype=np.uint64)) % q).astype(np.int64)
        assert np.array_equal(one[2 * e + 1][:, 0], a), e
        b = (ints(ee[e]) - ints(a) * ints(ss[0]) + ints(vv[e])) % qs[0]
        assert same(one[2 * e][:, 0], b), e


def test_ct_ks_hint_statuses():
    lib = capi.load_library()
    fn, part = lib.alch_ct_ks_hint, lib.alch_ct_ks_hint_part
    qs = primes_1_mod(64, 2, 1 << 29)
    ring, other, zp = A.Ring(64, qs), A.Ring(64, qs[:1]), A.Ring(64, [8], nocrt=True)
    out, v, err, sk = ring.alloc(9), ring.alloc(2), ring.alloc(4), ring.alloc(1)          # TrivGad: D = 2
    for b in (out, v, err, sk):
        b.fill_uniform(3)
    v_other, err_other, sk_other = other.alloc(2), other.alloc(4), other.alloc(1)
    before = out.download()
    o, V, Er, S = out._h, v._h, err._h, sk._h
    assert fn(o, 0, TRIV, 0, V, 0, Er, 0, S, 0, 1, 0) == 0 and fn(o, 9, TRIV, 0, V, 2, Er, 4, S, 0, 1, 0) == 0   # n_v = 0: nothing queued
    assert part(o, 0, TRIV, 5, 0, V, 0, Er, 0, S, 0, 1, 0) == 0
    assert np.array_equal(out.download(), before)
    bad = [
        (None, 0, TRIV, 2, V, 0, Er, 0, S, 0, 1, 0),                       # null buffers
        (o, 0, TRIV, 2, None, 0, Er, 0, S, 0, 1, 0),
        (o, 0, TRIV, 2, V, 0, None, 0, S, 0, 1, 0),
        (o, 0, TRIV, 2, V, 0, Er, 0, None, 0, 1, 0),
        (o, 0, TRIV, 2, v_other._h, 0, Er, 0, S, 0, 1, 0),                 # values of another ring
        (o, 0, TRIV, 2, V, 0, err_other._h, 0, S, 0, 1, 0),                # error terms of another ring
        (o, 0, TRIV, 2, V, 0, Er, 0, sk_other._h, 0, 1, 0),                # key of another ring
        (o, 0, 2, 2, V, 0, Er, 0, S, 0, 1, 0),                             # unknown gadget
        (o, 0, -1, 2, V, 0, Er, 0, S, 0, 1, 0),
        (o, 2, TRIV, 2, V, 0, Er, 0, S, 0, 1, 0),                          # output range: 2 + 8 of 9
        (o, 0, TRIV, 3, V, 0, Er, 0, S, 0, 1, 0),                          # output range: 12 of 9
        (o, 0, TRIV, (1 << 63) + 1, V, 0, Er, 0, S, 0, 1, 0),              # 2 * n_v * D wraps
        (o, 0, TRIV, 2, V, 1, Er, 0, S, 0, 1, 0),                          # value range
        (o, 0, TRIV, 2, V, 0, Er, 1, S, 0, 1, 0),                          # error-term range
        (o, 0, TRIV, 2, V, 0, Er, 0, S, 1, 1, 0),                          # key index
        (o, 0, TRIV, 1, o, 3, Er, 0, S, 0, 1, 0),                          # the value lies in the output
        (o, 0, TRIV, 1, V, 0, o, 2, S, 0, 1, 0),                           # the error terms overlap the output
        (o, 1, TRIV, 1, V, 0, Er, 0, o, 4, 1, 0),                          # the key lies in the output
    ]
    for args in bad:
        assert fn(*args) == capi.ALCH_E_INVALID, args
        assert lib.alch_last_error().decode().startswith("alch_ct_ks_hint:"), args
    bad_part = [
        (o, 0, TRIV, 0, 5, V, 0, Er, 0, S, 0, 1, 0),                       # entries 0 .. 4: 10 of 9 output elements, 5 of 4 error terms
        (o, 0, TRIV, 3, 2, V, 0, Er, 0, S, 0, 1, 0),                       # entry 4 belongs to value 2 of 2
        (o, 0, TRIV, (1 << 64) - 1, 2, V, 0, Er, 0, S, 0, 1, 0),           # e_first + e_count wraps
        (o, 7, TRIV, 0, 2, V, 0, Er, 0, S, 0, 1, 0),                       # output range
        (o, 0, 7, 0, 2, V, 0, Er, 0, S, 0, 1, 0),                          # unknown gadget
    ]
    for args in bad_part:
        assert part(*args) == capi.ALCH_E_INVALID, args
        assert lib.alch_last_error().decode().startswith("alch_ct_ks_hint_part:"), args
    zo, zv, ze, zs = zp.alloc(6), zp.alloc(1), zp.alloc(3), zp.alloc(1)
    assert fn(zo._h, 0, TRIV, 1, zv._h, 0, ze._h, 0, zs._h, 0, 1, 0) == capi.ALCH_E_NO_CRT
    assert lib.alch_last_error().decode().startswith("alch_ct_ks_hint:")
    assert np.array_equal(out.download(), before)


def centred_pow(ring, sk_crt):
    """The integer Pow coefficients of a short key held on the CRT basis."""
    t = ring.alloc(1)
    t.copy_from(sk_crt, 1)
    t.crtinv()
    w = t.download()[0]
    z = [int(x) if 2 * int(x) < ring.qs[0] else int(x) - ring.qs[0] for x in w[:, 0]]
    assert all((zi - int(x)) % q == 0 for j, q in enumerate(ring.qs) for zi, x in zip(z, w[:, j]))
    return z


@pytest.mark.parametrize("gadget", [TRIV, BASE2])
def test_ks_quad_circ_hint_relinearises(gadget):
    """gen_sk -> ks_quad_circ_hint -> encrypt two batches -> alch_ct_mul_relin -> decrypt: the negacyclic products of the plaintexts.

    Margin.  The same flow on the CPU with the oracle's own g_ks_hint / g_key_switch / g_decrypt (TrivGad, uniform errors in [-2, 2],
    these moduli, 5 products) has a worst error rate of 1.23e-15 (2^-49.5) after the key switch; the bound asserted here is 0.5."""
    mp, p, batch, seed = 64, 8, 5, 991
    qs = primes_1_mod(mp, 3, 1 << 28)
    assert all(q.bit_length() == 29 for q in qs)
    idx = G.Index(mp)
    svar = 3.0 / np.sqrt(float(idx.n))
    ring, zp = A.Ring(mp, qs), A.Ring(mp, [p], nocrt=True)
    sk = E.gen_sk(ring, svar, seed)
    hint = H.ks_quad_circ_hint(ring, gadget, sk, svar, seed + 1)
    rng = np.random.default_rng(seed)
    pa, pb = (rng.integers(0, p, size=(batch, idx.n, 1), dtype=np.int64) for _ in range(2))
    ca = E.encrypt_batch(ring, sk, zp.upload(pa), zp, zp, svar, seed + 2)
    cb = E.encrypt_batch(ring, sk, zp.upload(pb), zp, zp, svar, seed + 3)
    prod = ring.alloc(2 * batch)
    ring.ct_mul_relin(hint, ca, cb, prod, batch, s_pre=[pow(p, -1, q) for q in qs])     # both operands LSD: toMSD's scalar
    # the product: MSD, k = 0 + 0 + 1, l = 1 * 1 in LSD terms (CtMeta / mul_steps: rates and decrypt after toLSD's scalar p)
    to_lsd = [p % q for q in qs]
    rates = A.error_rates(prod, batch, sk, s_pre=to_lsd)
    assert max(rates) < 0.5, rates
    back = A.decrypt_batch(prod, batch, sk, zp, zp, 1, 1, s_pre=to_lsd).download(0, batch)
    for b in range(batch):
        want = G.ring_mul_def([int(x) for x in pa[b, :, 0]], [int(x) for x in pb[b, :, 0]], idx, p)
        assert back[b, :, 0].tolist() == want, b
    # the defining equation, bit for bit: h0 + h1 s - g_t s^2 = crt(l(e_t)), e_t the model's rounded samples of the Gaussian stream
    D = ring.gadget_digits(gadget)
    s2 = ring.alloc(1)
    s2.mul(sk, sk, 1)
    h = H.ks_hint(ring, gadget, sk, s2, 1, svar, seed + 1).download()
    assert_reduced(h, qs)
    s, ss, q = ints(sk.download()[0]), ints(s2.download()[0]), ints(qs)
    resid = []
    for t, (limb, d) in enumerate(gadget_entries(qs, gadget)):
        g = np.zeros(len(qs), dtype=object)
        g[limb] = 1 << d
        resid.append(((ints(h[2 * t]) + ints(h[2 * t + 1]) * s - g * ss) % q).astype(np.int64))
    e_pow = ring.upload(np.stack(resid))
    e_pow.crtinv()
    z = GM.gauss_dec(mp, float(svar), E.splitmix64(seed + 1), 0, D)
    want = np.stack([np.stack([np.array(G.l_def([int(x) for x in z[t]], idx, q_), dtype=np.int64) % q_ for q_ in qs], axis=1)
                     for t in range(D)])
    assert np.array_equal(e_pow.download(), want)


TUNNEL_HS_QS = [537264001, 539884801, 555609601]                                         # examples/Tunnel.hs:34-39, the first three


@pytest.mark.parametrize("r,s,rp,sp,qs,gadget", [
    (8, 12, 40, 60, TUNNEL_HS_QS, TRIV),
    (8, 12, 40, 60, TUNNEL_HS_QS, BASE2),
    (128, 64, 128, 64, None, TRIV),                                                      # two-power, down: d_rel = 2, p_i = X^i
    (64, 128, 64, 128, None, TRIV),                                                      # two-power, up: d_rel = 1, p_0 = 1
])
def test_tunnel_hint_tunnels(r, s, rp, sp, qs, gadget):
    import random
    p, batch, seed = 8, 3, 5150 + rp
    qs = qs or primes_1_mod(128, 3, 1 << 28)
    assert all(q.bit_length() in (29, 30) and (q - 1) % rp == 0 and (q - 1) % sp == 0 for q in qs)
    T = G.tunnel_indices(r, s, rp, sp)
    gr, gs = A.Ring(rp, qs), A.Ring(sp, qs)
    ep, d_rel = A.Tunnel.info(gr, gs)
    assert ep == T.ep.m and d_rel == T.rp.n // T.ep.n == T.r.n // T.e.n
    sk_in = E.gen_sk(gr, 3.0 / np.sqrt(float(T.rp.n)), seed)
    sk_out = E.gen_sk(gs, 3.0 / np.sqrt(float(T.sp.n)), seed + 1)
    rng = random.Random(seed)
    ys = [[rng.randrange(p) for _ in range(T.s.n)] for _ in range(d_rel)]
    ysz = [G.embed_pow([G.centred(x, p) for x in y], T.s, T.sp) for y in ys]
    lin = gs.upload(np.stack([to_aos([[x % q for x in y] for q in qs]) for y in ysz]))
    lin.crt()
    # the values the hints encrypt, against the model's line `val = eval_lin_dec(...)` of g_tunnel_hint
    v = H.tunnel_values(gr, gs, lin, sk_in).download()
    s_in = centred_pow(gr, sk_in)
    rows = G.coeffs_indices(T.ep, T.rp)
    assert len(rows) == d_rel
    for i, row in enumerate(rows):
        pi = [0] * T.rp.n
        pi[row[0]] = 1
        x = G.ring_mul_def(s_in, pi, T.rp, None)
        val = G.eval_lin_dec(ysz, G.linv_def(x, T.rp, None), T.ep, T.rp, T.sp, None)
        assert np.array_equal(v[i], gs.crt(to_aos([[x % q for x in val] for q in qs]))), i
    # encrypt under s_in -> tunnel -> decrypt under s_out
    svar = 3.0 / np.sqrt(float(T.sp.n))
    tun = H.tunnel_hint(gr, gs, gadget, lin, sk_out, sk_in, svar, seed + 2)
    zr_big, zs_big = A.Ring(rp, [p], nocrt=True), A.Ring(sp, [p], nocrt=True)
    zr = zr_big if r == rp else A.Ring(r, [p], nocrt=True)
    zs = zs_big if s == sp else A.Ring(s, [p], nocrt=True)
    pts = np.array([[[rng.randrange(p)] for _ in range(T.r.n)] for _ in range(batch)], dtype=np.int64)
    cts = E.encrypt_batch(gr, sk_in, zr.upload(pts), zr, zr_big, 3.0 / np.sqrt(float(T.rp.n)), seed + 3)
    out = gs.alloc(2 * batch)
    tun.apply(cts, out, batch, s_pre=[pow(p, -1, q) for q in qs])                        # LSD in: toMSD's scalar; MSD out, k = 0
    to_lsd = [p % q for q in qs]
    rates = A.error_rates(out, batch, sk_out, s_pre=to_lsd)
    assert max(rates) < 0.5, rates
    back = A.decrypt_batch(out, batch, sk_out, zs_big, zs, 0, 1, s_pre=to_lsd).download(0, batch)
    for b in range(batch):
        pt = [int(x) for x in pts[b, :, 0]]
        assert back[b, :, 0].tolist() == G.eval_lin_dec(ys, G.linv_def(pt, T.r, p), T.e, T.r, T.s, p), b
