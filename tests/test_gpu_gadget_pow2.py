"""GPU: the BaseBGad 2^w gadget (ALCH_GAD_BASEPOW2(w), 1 <= w <= 16) through every entry point that takes a gadget code or serves a
hint made with one: alch_decompose_baseb against the exact model, alch_ct_mul_relin / alch_ct_mul_full / alch_ct_tunnel against the C
restatement's compositions with the decomposition of tests/gadget_pow2_ref.py, alch_ct_ks_hint against Python integers, and the
generated hints closed by decryption.  Everything bit for bit, every stored word below its modulus.

On the parent commit every gadget code above 1 is refused and alch_decompose_baseb / alch_gadget_digits do not exist."""
import ctypes as C
import random

import numpy as np
import pytest

import alchemy_amd as A
import gadget_pow2_ref as R
from alchemy_amd import capi
from alchemy_amd import encrypt as E
from alchemy_amd import hints as H
from conftest import ARITH_QS, CFG3_QS
from helpers import assert_parent_unchanged, assert_reduced, carve, extreme_words, primes_1_mod, primes_below
from oracle import model_gen as G

pytestmark = pytest.mark.gpu

P2 = capi.ALCH_GAD_BASEPOW2
Q60 = [1152921504606748673, 1152921504606683137]                  # 60-bit primes, 1 mod 2^11


def rand(rng, count, n, qs):
    return np.ascontiguousarray(np.stack([rng.integers(0, q, size=(count, n), dtype=np.int64) for q in qs], axis=2))


def ints(a):
    return np.asarray(a).astype(object)


# ---- decompose -----------------------------------------------------------------------------------------------------------------------
def _decompose_rings():
    return [(32, [primes_1_mod(32, 1, 1 << 13)[0], primes_1_mod(32, 1, 1 << 16)[0], primes_below(32, 1, 1 << 31)[0]], 4),
            (32, [primes_1_mod(32, 1, 1 << 16)[0], primes_below(32, 1, 1 << 62)[0]], 8),
            (9, primes_1_mod(9, 2, 1 << 20), 4)]


@pytest.mark.parametrize("w", [1, 2, 3, 5, 8, 16])
def test_decompose_baseb_equals_the_model(w):
    from oracle import model as M
    rng = np.random.default_rng(40 + w)
    for m, qs, word in _decompose_rings():
        ring = A.Ring(m, qs)
        assert ring.word_bytes == word
        assert ring.gadget_digits(P2(w)) == sum(R.digit_counts(qs, w)) == sum(M.baseb_digits(q, 1 << w) for q in qs)
        for elem in list(extreme_words(rng, 1, ring.n, qs)) + list(rand(rng, 1, ring.n, qs)):
            got = ring.decompose_baseb(elem, P2(w))
            want = M.decompose_baseb([[int(x) for x in elem[:, i]] for i in range(len(qs))], qs, 1 << w)
            assert len(got) == len(want)
            assert_reduced(np.stack(got), qs)
            for t, (g, d) in enumerate(zip(got, want)):
                assert np.array_equal(ints(g), ints(np.stack([[x % q for x in d] for q in qs], axis=1))), (m, w, t)
            if w == 1:                                       # BASEPOW2(1) means exactly ALCH_GAD_BASE2
                assert ring.gadget_digits(capi.ALCH_GAD_BASE2) == len(got)
                for g, b in zip(got, ring.decompose_base2(elem)):
                    assert np.array_equal(g, b)
                for g, b in zip(got, ring.decompose_baseb(elem, capi.ALCH_GAD_BASE2)):
                    assert np.array_equal(g, b)


# ---- alch_ct_mul_relin ----------------------------------------------------------------------------------------------------------------
def check_mul_relin(oracle_lib, m, qs, w, batch, general=False, flags=0, scratch_mib=None, seed=0, check_cts=None):
    g = A.Ring(m, qs)
    n = g.n
    o = oracle_lib.GenRing(m, qs) if general else oracle_lib.Ring(n, qs)
    rng = np.random.default_rng(7000 + m % 1000 + 17 * w + seed)
    D = g.gadget_digits(P2(w))
    assert D == sum(R.digit_counts(qs, w))
    hint, a, b = rand(rng, 2 * D, n, qs), rand(rng, 2 * batch, n, qs), rand(rng, 2 * batch, n, qs)
    s_pre = [pow(7, -1, q) for q in qs]
    gh = g.hint_load(hint, gadget=P2(w))
    src_a, src_b = a, b
    if flags & capi.ALCH_POW_IN:
        src_a, src_b = np.stack([o.crtinv(np.ascontiguousarray(x)) for x in a]), np.stack([o.crtinv(np.ascontiguousarray(x)) for x in b])
    gout = g.alloc(2 * batch)
    g.ct_mul_relin(gh, g.upload(src_a), g.upload(src_b), gout, batch, s_pre=s_pre, flags=flags)
    got = gout.download()
    assert_reduced(got, qs)
    if scratch_mib is not None:                              # chunked, with a ragged last chunk: the same words
        g.set_option("scratch_mib", scratch_mib)
        again = g.alloc(2 * batch)
        g.ct_mul_relin(gh, g.upload(src_a), g.upload(src_b), again, batch, s_pre=s_pre, flags=flags)
        assert np.array_equal(again.download(), got)
    for ct in (range(batch) if check_cts is None else check_cts):
        w0, w1 = R.mul_relin_pow2(o, qs, w, list(hint), a[2 * ct], a[2 * ct + 1], b[2 * ct], b[2 * ct + 1], s_pre=s_pre,
                                  pow_out=bool(flags & capi.ALCH_POW_OUT), mulg=general)
        assert np.array_equal(got[2 * ct], w0) and np.array_equal(got[2 * ct + 1], w1), (m, w, ct)
    return got


@pytest.mark.parametrize("w", range(1, 17))
def test_mul_relin_every_width_at_n16(oracle_lib, w):
    check_mul_relin(oracle_lib, 32, ARITH_QS[:2], w, 3)


@pytest.mark.parametrize("logn,qs,w,batch", [
    (11, [65537, 786433, 2147352577], 3, 2), (11, [65537, 786433, 2147352577], 8, 2), (11, [65537, 786433, 2147352577], 16, 2),
    (11, [12289, 65537, 2147352577], 16, 2),                 # a target modulus below 2^(w-1): non-top digits need reducing too
    (15, CFG3_QS, 4, 1),
    (16, primes_1_mod(1 << 17, 2, 1 << 29), 8, 1),           # split ring: k_decompose_base2 + batched crt
    (10, Q60, 5, 2), (10, Q60, 16, 2),
    (15, primes_1_mod(1 << 16, 1, 1 << 59), 16, 1),           # the 8-byte split size
])
def test_mul_relin_matches_the_composition(oracle_lib, logn, qs, w, batch):
    check_mul_relin(oracle_lib, 2 << logn, qs, w, batch)


def test_mul_relin_general_index(oracle_lib):
    check_mul_relin(oracle_lib, 420, primes_1_mod(420, 2, 1 << 20), 4, 2, general=True)
    check_mul_relin(oracle_lib, 9, primes_1_mod(9, 2, 1 << 20), 3, 2, general=True)            # phi = 6: the one-word loader
    check_mul_relin(oracle_lib, 9, primes_below(9, 2, 1 << 62), 16, 2, general=True)           # 8-byte words


def test_mul_relin_pow_bases_and_chunks(oracle_lib):
    check_mul_relin(oracle_lib, 1 << 9, CFG3_QS[:2], 4, 2, flags=capi.ALCH_POW_IN | capi.ALCH_POW_OUT)
    # n = 2^10, 3 limbs, w = 4: c2 in both bases + 24 digits = 26 elements of 12 KiB per ciphertext, so scratch_mib = 1 holds chunks
    # of 3 and a batch of 7 runs as 3 + 3 + 1
    check_mul_relin(oracle_lib, 1 << 11, CFG3_QS[:3], 4, 7, scratch_mib=1, check_cts=(0, 3, 6))


def test_mul_relin_writes_its_result_range_only(oracle_lib):
    """Every range a view in the interior of one parent; every other word of the parent stays as uploaded."""
    m, qs, w, batch = 1 << 9, CFG3_QS[:2], 4, 2
    g, o = A.Ring(m, qs), oracle_lib.Ring(m // 2, qs)
    rng = np.random.default_rng(31)
    D = g.gadget_digits(P2(w))
    hint = rand(rng, 2 * D, g.n, qs)
    host = rand(rng, 3 + 2 * batch + 2 + 2 * batch + 2 + 2 * batch + 3, g.n, qs)
    ia, ib, io = 3, 3 + 2 * batch + 2, 3 + 4 * batch + 4
    parent, (va, vb, vo) = carve(g, host, (ia, 2 * batch), (ib, 2 * batch), (io, 2 * batch))
    g.ct_mul_relin(g.hint_load(hint, gadget=P2(w)), va, vb, vo, batch)
    got = assert_parent_unchanged(parent, host, [(io, 2 * batch)])
    for ct in range(batch):
        w0, w1 = R.mul_relin_pow2(o, qs, w, list(hint), host[ia + 2 * ct], host[ia + 2 * ct + 1], host[ib + 2 * ct], host[ib + 2 * ct + 1])
        assert np.array_equal(got[io + 2 * ct], w0) and np.array_equal(got[io + 2 * ct + 1], w1)


# ---- alch_ct_mul_full -----------------------------------------------------------------------------------------------------------------
def test_mul_full_with_the_hint_on_all_limbs(oracle_lib):
    n, qs_h, l_in, l_out, w, batch = 64, ARITH_QS, 3, 2, 4, 2
    L = len(qs_h)
    rng = np.random.default_rng(9101)
    rh, rin, rout = A.Ring(2 * n, qs_h), A.Ring(2 * n, qs_h[L - l_in:]), A.Ring(2 * n, qs_h[L - l_out:])
    D = rh.gadget_digits(P2(w))
    hint, a, b = rand(rng, 2 * D, n, qs_h), rand(rng, 2 * batch, n, qs_h[L - l_in:]), rand(rng, 2 * batch, n, qs_h[L - l_in:])
    s_pre = [int(rng.integers(1, q)) for q in qs_h[L - l_in:]]
    gh = rh.hint_load(hint, gadget=P2(w))
    for pow_out in (False, True):
        out = rout.alloc(2 * batch)
        capi.ct_mul_full(gh, rin.upload(a), rin.upload(b), out, batch, s_pre=s_pre, flags=capi.ALCH_POW_OUT if pow_out else 0)
        got = out.download()
        assert_reduced(got, qs_h[L - l_out:])
        for ct in range(batch):
            w0, w1 = R.full_mul_pow2(oracle_lib, n, qs_h, l_in, l_out, w, list(hint), a[2 * ct], a[2 * ct + 1], b[2 * ct], b[2 * ct + 1],
                                     s_pre, pow_out=pow_out)
            assert np.array_equal(got[2 * ct], w0) and np.array_equal(got[2 * ct + 1], w1), (ct, pow_out)


@pytest.mark.parametrize("m", [128, 420])
def test_mul_full_with_the_hint_on_fewer_limbs(oracle_lib, m):
    w, batch = 4, 2
    qs_in = ARITH_QS if m == 128 else primes_1_mod(m, 3, lo=1 << 20)
    rng = np.random.default_rng(9300 + m)
    rin, rh, rout = A.Ring(m, qs_in), A.Ring(m, qs_in[1:]), A.Ring(m, qs_in[2:])
    n = rin.n
    D = rh.gadget_digits(P2(w))
    hint, a, b = rand(rng, 2 * D, n, qs_in[1:]), rand(rng, 2 * batch, n, qs_in), rand(rng, 2 * batch, n, qs_in)
    s_pre = [int(rng.integers(1, q)) for q in qs_in]
    gh = rh.hint_load(hint, gadget=P2(w))
    for l_out, ro in ((2, rh), (1, rout)):
        out = ro.alloc(2 * batch)
        capi.ct_mul_full(gh, rin.upload(a), rin.upload(b), out, batch, s_pre=s_pre)
        got = out.download()
        assert_reduced(got, qs_in[3 - l_out:])
        for ct in range(batch):
            w0, w1 = R.full_mul_pow2_down(oracle_lib, n, qs_in, 2, l_out, w, list(hint), a[2 * ct], a[2 * ct + 1], b[2 * ct], b[2 * ct + 1],
                                          s_pre, m=None if m == 128 else m)
            assert np.array_equal(got[2 * ct], w0) and np.array_equal(got[2 * ct + 1], w1), (m, l_out, ct)


# ---- tunnels --------------------------------------------------------------------------------------------------------------------------
def check_tunnel(oracle_lib, rp, sp, qs, w, batch=5, flags=0, word_bytes=None):
    gr, gs = A.Ring(rp, qs), A.Ring(sp, qs)
    if word_bytes is not None:
        assert gr.word_bytes == gs.word_bytes == word_bytes
    _, d_rel = A.Tunnel.info(gr, gs)
    D = gs.gadget_digits(P2(w))
    assert D == sum(R.digit_counts(qs, w))
    rng = np.random.default_rng(rp * 131 + sp + w)
    lin, ks, cts = rand(rng, d_rel, gs.n, qs), rand(rng, 2 * d_rel * D, gs.n, qs), rand(rng, 2 * batch, gr.n, qs)
    s_pre = [int(rng.integers(1, q)) for q in qs]
    tun = A.Tunnel(gr, gs, gs.upload(lin), gs.upload(ks), gadget=P2(w))
    Or = oracle_lib.GenRing(rp, qs)
    src = np.stack([Or.crtinv(np.ascontiguousarray(c)) for c in cts]) if flags & capi.ALCH_POW_IN else cts
    gin, gout = gr.upload(src), gs.alloc(2 * batch)
    gout.fill_uniform(99)
    tun.apply(gin, gout, batch, s_pre=s_pre, flags=flags)
    got = gout.download()
    assert_reduced(got, qs)
    for ct in range(batch):
        w0, w1 = R.tunnel_pow2(oracle_lib, rp, sp, qs, w, list(lin), list(ks), cts[2 * ct], cts[2 * ct + 1], s_pre)
        assert np.array_equal(got[2 * ct], w0) and np.array_equal(got[2 * ct + 1], w1), (rp, sp, w, ct)
    assert np.array_equal(gin.download(), src)


@pytest.mark.parametrize("w", [4, 16])
@pytest.mark.parametrize("rp,sp", [(3, 5), (15, 20), (27, 9)])
def test_tunnel_general_index(oracle_lib, rp, sp, w):
    m = rp * sp // np.gcd(rp, sp)
    check_tunnel(oracle_lib, rp, sp, primes_1_mod(int(m), 3, 1 << 28), w, flags=capi.ALCH_POW_IN if (rp, w) == (15, 4) else 0)


@pytest.mark.parametrize("w", [4, 16])
@pytest.mark.parametrize("rp,sp", [(64, 32), (32, 64), (1 << 12, 1 << 11)])
def test_tunnel_two_power(oracle_lib, rp, sp, w):
    check_tunnel(oracle_lib, rp, sp, primes_1_mod(max(rp, sp), 3, 1 << 28), w, flags=capi.ALCH_POW_IN if (rp, w) == (32, 16) else 0)


@pytest.mark.parametrize("rp,sp", [(64, 32), (15, 20)])
def test_tunnel_on_8_byte_words(oracle_lib, rp, sp):
    m = rp * sp // int(np.gcd(rp, sp))
    check_tunnel(oracle_lib, rp, sp, primes_below(m, 3, 1 << 62), 16, word_bytes=8)


# ---- hints ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1, 4, 16])
@pytest.mark.parametrize("m,word", [(32, 32), (32, 64), (9, 32)])
def test_ct_ks_hint_equals_python_integers(m, word, w):
    """As tests/test_gpu_hints.py computes them, with the entries 2^(w t); and the same hint made in two parts."""
    qs = primes_1_mod(m, 2, 1 << 29) if word == 32 else primes_below(m, 2, 1 << 62)
    ring = A.Ring(m, qs)
    ent = R.gadget_pow2(qs, w)
    D = ring.gadget_digits(P2(w))
    assert D == len(ent)
    n_v, out_first, v_first, err_first, sk_index, ct0, seed = 2, 3, 1, 2, 1, 3, 0xB6B6 + m
    total = n_v * D
    out, v, err, sk = ring.alloc(out_first + 2 * total), ring.alloc(v_first + n_v), ring.alloc(err_first + total), ring.alloc(2)
    uni = ring.alloc(2 * (ct0 + total))
    out.fill_uniform(1); v.fill_uniform(2); err.fill_uniform(3); sk.fill_uniform(4); uni.fill_uniform(seed)
    keep = out.download(0, out_first)
    H.ct_ks_hint(out, P2(w), n_v, v, err, sk, seed, out_first=out_first, v_first=v_first, err_first=err_first, sk_index=sk_index, ct0=ct0)
    got, u = out.download(), uni.download()
    assert_reduced(got, qs)
    assert np.array_equal(got[:out_first], keep)
    vv, ee, s, q = v.download()[v_first:], err.download()[err_first:], ints(sk.download()[sk_index]), ints(qs)
    for i in range(n_v):
        for t, (limb, d) in enumerate(ent):
            e = i * D + t
            a = ints(u[2 * (ct0 + e) + 1])
            g = np.zeros(len(qs), dtype=object)
            g[limb] = 1 << (w * d)
            assert (1 << (w * d)) < qs[limb]
            assert np.array_equal(ints(got[out_first + 2 * e + 1]), a), (m, e)
            assert np.array_equal(ints(got[out_first + 2 * e]), (ints(ee[e]) - a * s + g * ints(vv[i])) % q), (m, e)
    # two parts, cut inside value 1
    cut = D + 1
    parts = ring.alloc(1 + 2 * total)
    H.ct_ks_hint_part(parts, P2(w), 0, cut, v, err, sk, seed, out_first=1, v_first=v_first, err_first=err_first, sk_index=sk_index, ct0=ct0)
    H.ct_ks_hint_part(parts, P2(w), cut, total - cut, v, err, sk, seed, out_first=1 + 2 * cut, v_first=v_first, err_first=err_first + cut,
                      sk_index=sk_index, ct0=ct0 + cut)
    assert np.array_equal(parts.download(1), got[out_first:])
    if w == 1:
        base2 = ring.alloc(2 * total)
        H.ct_ks_hint(base2, capi.ALCH_GAD_BASE2, n_v, v, err, sk, seed, v_first=v_first, err_first=err_first, sk_index=sk_index, ct0=ct0)
        assert np.array_equal(base2.download(), got[out_first:])


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1, 4, 8, 16])
def test_generated_hint_relinearises_and_decrypts(w):
    """gen_sk -> ks_quad_circ_hint(gadget) -> encrypt_batch -> alch_ct_mul_relin -> decrypt_batch at n = 64 on the ARITH moduli: the
    plaintext products.  The error rates after the key switch are the price of the base; they are printed, not asserted (DESIGN
    section 20 records them)."""
    mp, p, batch, seed = 128, 8, 4, 1991 + w
    qs = ARITH_QS
    assert all((q - 1) % mp == 0 for q in qs)
    idx = G.Index(mp)
    svar = 3.0 / np.sqrt(float(idx.n))
    ring, zp = A.Ring(mp, qs), A.Ring(mp, [p], nocrt=True)
    sk = E.gen_sk(ring, svar, seed)
    hint = H.ks_quad_circ_hint(ring, P2(w), sk, svar, seed + 1)
    rng = np.random.default_rng(seed)
    pa, pb = (rng.integers(0, p, size=(batch, idx.n, 1), dtype=np.int64) for _ in range(2))
    ca = E.encrypt_batch(ring, sk, zp.upload(pa), zp, zp, svar, seed + 2)
    cb = E.encrypt_batch(ring, sk, zp.upload(pb), zp, zp, svar, seed + 3)
    prod = ring.alloc(2 * batch)
    ring.ct_mul_relin(hint, ca, cb, prod, batch, s_pre=[pow(p, -1, q) for q in qs])
    to_lsd = [p % q for q in qs]
    print("error rates after the key switch on the ARITH moduli, w = %d, D = %d:" % (w, ring.gadget_digits(P2(w))),
          A.error_rates(prod, batch, sk, s_pre=to_lsd))
    back = A.decrypt_batch(prod, batch, sk, zp, zp, 1, 1, s_pre=to_lsd).download(0, batch)
    for b in range(batch):
        want = G.ring_mul_def([int(x) for x in pa[b, :, 0]], [int(x) for x in pb[b, :, 0]], idx, p)
        assert back[b, :, 0].tolist() == want, b


def test_generated_tunnel_hint_decrypts_to_the_linear_function():
    r, s, rp, sp, p, batch, seed, w = 3, 4, 15, 20, 8, 3, 6150, 4
    qs = primes_1_mod(60, 3, 1 << 28)
    T = G.tunnel_indices(r, s, rp, sp)
    gr, gs = A.Ring(rp, qs), A.Ring(sp, qs)
    _, d_rel = A.Tunnel.info(gr, gs)
    sk_in = E.gen_sk(gr, 3.0 / np.sqrt(float(T.rp.n)), seed)
    sk_out = E.gen_sk(gs, 3.0 / np.sqrt(float(T.sp.n)), seed + 1)
    rng = random.Random(seed)
    ys = [[rng.randrange(p) for _ in range(T.s.n)] for _ in range(d_rel)]
    ysz = [G.embed_pow([G.centred(x, p) for x in y], T.s, T.sp) for y in ys]
    lin = gs.upload(np.stack([np.ascontiguousarray(np.array([[x % q for x in y] for q in qs], dtype=np.int64).T) for y in ysz]))
    lin.crt()
    tun = H.tunnel_hint(gr, gs, P2(w), lin, sk_out, sk_in, 3.0 / np.sqrt(float(T.sp.n)), seed + 2)
    zr_big, zs_big = A.Ring(rp, [p], nocrt=True), A.Ring(sp, [p], nocrt=True)
    zr, zs = A.Ring(r, [p], nocrt=True), A.Ring(s, [p], nocrt=True)
    pts = np.array([[[rng.randrange(p)] for _ in range(T.r.n)] for _ in range(batch)], dtype=np.int64)
    cts = E.encrypt_batch(gr, sk_in, zr.upload(pts), zr, zr_big, 3.0 / np.sqrt(float(T.rp.n)), seed + 3)
    out = gs.alloc(2 * batch)
    tun.apply(cts, out, batch, s_pre=[pow(p, -1, q) for q in qs])
    to_lsd = [p % q for q in qs]
    back = A.decrypt_batch(out, batch, sk_out, zs_big, zs, 0, 1, s_pre=to_lsd).download(0, batch)
    for b in range(batch):
        pt = [int(x) for x in pts[b, :, 0]]
        assert back[b, :, 0].tolist() == G.eval_lin_dec(ys, G.linv_def(pt, T.r, p), T.e, T.r, T.s, p), b


# ---- statuses -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gadget", [P2(0), P2(17), 2, 0x200, -1])
def test_unknown_codes_are_invalid_on_every_entry_point(gadget):
    lib = capi.load_library()
    qs = primes_1_mod(64, 2, 1 << 28)
    ring, small = A.Ring(64, qs), A.Ring(32, qs)
    n = ring.n
    vp, nd, out = C.c_void_p(), C.c_int(), C.c_void_p()
    host = np.zeros((400, n, 2), dtype=np.int64)
    buf, v, err, sk = ring.alloc(400), ring.alloc(2), ring.alloc(200), ring.alloc(1)
    p64 = host.ctypes.data_as(C.POINTER(C.c_int64))
    calls = {
        "alch_hint_load": lambda: lib.alch_hint_load(ring._h, gadget, p64, C.byref(out)),
        "alch_hint_from_buf": lambda: lib.alch_hint_from_buf(ring._h, gadget, buf._h, C.byref(out)),
        "alch_tunnel_create": lambda: lib.alch_tunnel_create(small._h, ring._h, gadget, buf._h, buf._h, C.byref(out)),
        "alch_ct_ks_hint": lambda: lib.alch_ct_ks_hint(buf._h, 0, gadget, 1, v._h, 0, err._h, 0, sk._h, 0, 1, 0),
        "alch_ct_ks_hint_part": lambda: lib.alch_ct_ks_hint_part(buf._h, 0, gadget, 0, 1, v._h, 0, err._h, 0, sk._h, 0, 1, 0),
        "alch_gadget_digits": lambda: lib.alch_gadget_digits(ring._h, gadget, C.byref(nd)),
        "alch_decompose_baseb": lambda: lib.alch_decompose_baseb(ring._h, gadget, None, None, C.byref(nd)),
    }
    for name, call in calls.items():
        assert call() == capi.ALCH_E_INVALID, name
        assert name in lib.alch_last_error().decode(), (name, lib.alch_last_error())
    with pytest.raises(A.AlchemyError) as e:
        capi.select_limbs(qs, 0, capi.ALCH_OP_MUL, gadget)
    assert e.value.code == capi.ALCH_E_INVALID


def test_a_hint_source_one_element_short_is_refused():
    qs = primes_1_mod(64, 2, 1 << 28)
    ring = A.Ring(64, qs)
    D = ring.gadget_digits(P2(4))
    assert D == 16
    with pytest.raises(A.AlchemyError) as e:
        ring.hint_from_buf(ring.alloc(2 * D - 1), gadget=P2(4))
    assert e.value.code == capi.ALCH_E_INVALID
    ring.hint_from_buf(ring.alloc(2 * D), gadget=P2(4))
    # TrivGad is no BaseBGad code for the decomposition
    assert capi.load_library().alch_decompose_baseb(ring._h, capi.ALCH_GAD_TRIV, None, None, C.byref(C.c_int())) == capi.ALCH_E_INVALID
