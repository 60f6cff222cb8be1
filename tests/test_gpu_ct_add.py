"""GPU: SymmSHE (+), (-), negate on resident batches with unaligned operands -- alch_ct_add / k_ct_add through alchemy_amd/ctadd.py.

Every comparison is exact.  Three references: the model (oracle/model_gen.py instances of tests/ct_add_cases.py, word for word against
the pure-Python formula and through alchemy_amd.decrypt_batch against the plaintext sums), the existing entry points on uniform words
(alch_buf_scale, alch_buf_mulg, alch_buf_add / alch_buf_sub, alch_buf_copy -- none of them changed by this feature), and Python integers
with the model's CRT image of g for the worst-case words.

On the parent commit the package has no `ctadd` module and the library no alch_ct_add: the module does not import there."""
import numpy as np
import pytest

import alchemy_amd as A
from alchemy_amd import capi
from alchemy_amd.capi import ALCH_BASIS_CRT, ALCH_BASIS_POW, ALCH_POW_IN, ALCH_POW_OUT
from alchemy_amd.ctadd import CtMeta, align, ct_add, ct_add_raw, ct_neg, ct_sub
import ct_add_cases as K
from helpers import assert_reduced, primes_1_mod, primes_below, to_aos
from oracle import model_gen as G

pytestmark = pytest.mark.gpu

POW = ALCH_POW_IN | ALCH_POW_OUT
BATCHES = (1, 3, 37)
G_PAIRS = [(0, 0), (1, 0), (0, 3), (2, 1)]
DEG_PAIRS = [(1, 1), (1, 2), (2, 1), (2, 2)]


# ---- against the model -------------------------------------------------------------------------------------------------------------
def host_cts(comps, batch):
    """limb-major Pow components of one ciphertext -> (batch * (degree + 1), n, L) int64, the ciphertext `batch` times over."""
    return np.stack([to_aos(c) for c in comps] * batch)


@pytest.mark.parametrize("mp,m,p", K.RINGS)
def test_model_instances(mp, m, p):
    """ct_add / ct_sub / ct_neg on the model's ciphertexts: CRT basis (crt, call, crtInv) and Pow basis give the Python formula word
    for word, the returned metadata are the rule's, and decrypt_batch of the result is the sum / difference / negation of the
    plaintexts (degree 1 and 2)."""
    sk, cases = K.instances(mp, m, p)
    batch = 2
    zp_big, zp_small = A.Ring(mp, [p], nocrt=True), A.Ring(m, [p], nocrt=True)
    rings = {}
    for name, ca, pa, cb, pb in cases:
        qs = tuple(ca.qs)
        if qs not in rings:
            ring = A.Ring(mp, list(qs))
            gsk = ring.upload(np.stack([to_aos([[v % q for v in sk] for q in qs])]))
            gsk.crt()
            rings[qs] = (ring, gsk)
        ring, gsk = rings[qs]
        ma, mb = K.meta_of(ca), K.meta_of(cb)
        ha, hb = host_cts(ca.c, batch), host_cts(cb.c, batch)

        def decrypted(buf, meta):
            lsd = G.g_to_lsd(K.as_gct([], meta, ca))                # the metadata of the LSD form
            s_pre = None if meta.enc == "LSD" else [p % q for q in qs]
            pt = A.decrypt_batch(buf, batch, gsk, zp_big, zp_small, lsd.k, lsd.l, degree=meta.degree, s_pre=s_pre, flags=ALCH_POW_IN)
            return pt.download(0, batch)[:, :, 0].tolist()

        for op in ("add", "sub", "neg"):
            if op == "neg":
                want_meta = ma
                want = K.formula(ca, [q - 1 for q in qs], 0, None, None, 0)
                want_pt = [(-u) % p for u in pa]
            else:
                s_a, g_a, s_b, g_b, want_meta = align(ma, mb, qs, op == "sub")
                want = K.formula(ca, s_a, g_a, cb, s_b, g_b)
                want_pt = [(u - v) % p if op == "sub" else (u + v) % p for u, v in zip(pa, pb)]
            want_host = host_cts(want, batch)
            for flags in (0, POW):
                ga, gb = ring.upload(ha), ring.upload(hb)
                if not flags:
                    ga.crt()
                    gb.crt()
                if op == "neg":
                    out, meta = ct_neg(ga, ma, batch, flags)
                else:
                    out, meta = (ct_sub if op == "sub" else ct_add)(ga, ma, gb, mb, batch, flags)
                assert meta == want_meta, (name, op)
                if not flags:
                    out.crtinv(0, (meta.degree + 1) * batch)
                got = out.download(0, (meta.degree + 1) * batch)
                assert np.array_equal(got, want_host), (name, op, flags)
                assert decrypted(out, meta) == [want_pt] * batch, (name, op, flags)
                del ga, gb, out


# ---- against the existing entry points, on uniform words ---------------------------------------------------------------------------
def uniform_rings():
    return [
        ("m32", 32, primes_1_mod(32, 2, 1 << 28), 4, 4),                                                   # VW = 4, no g
        ("m45", 45, primes_1_mod(45, 3, 1 << 29), 4, 4),                                                   # VW = 4, g table
        ("m27", 27, primes_1_mod(27, 2, 1 << 29), 4, 1),                                                   # n = 18: one word per lane
        ("m45w64", 45, [primes_below(45, 1, 1 << 60)[0], primes_1_mod(45, 1, 1 << 28)[0]], 8, 2),           # 8-byte words, VW = 2
        ("m2048", 1 << 11, primes_1_mod(1 << 11, 2, 1 << 29), 4, 4),                                       # n = 1024: several workgroups per row
    ]


def scalars(rng, qs):
    return [int(rng.integers(1, q)) for q in qs]


def reference_term(ring, src, deg, batch, s, g, basis):
    """s * g^g * src on a copy, from alch_buf_scale and alch_buf_mulg."""
    count = (deg + 1) * batch
    t = ring.alloc(count)
    t.copy_from(src, count)
    if s is not None:
        t.scale(t, count, s)
    for _ in range(g):
        t.mulg(basis, 0, count)
    return t


def reference_sum(ring, ta, da, tb, db, batch, n, L, sub=False):
    """(batch, max degree + 1, n, L) words of ta + tb: alch_buf_add / alch_buf_sub on the shared components (gathered with
    alch_buf_copy when the degrees differ), the odd c2 as it is."""
    if da == db:
        out = ring.alloc((da + 1) * batch)
        (out.sub if sub else out.add)(ta, tb, (da + 1) * batch)
        return out.download().reshape(batch, da + 1, n, L)
    sa, sb, out = ring.alloc(2 * batch), ring.alloc(2 * batch), ring.alloc(2 * batch)
    for ct in range(batch):
        sa.copy_from(ta, 2, dst_first=2 * ct, src_first=(da + 1) * ct)
        sb.copy_from(tb, 2, dst_first=2 * ct, src_first=(db + 1) * ct)
    (out.sub if sub else out.add)(sa, sb, 2 * batch)
    shared = out.download().reshape(batch, 2, n, L)
    hi = (ta if da == 2 else tb).download(0, 3 * batch).reshape(batch, 3, n, L)[:, 2:]
    if sub and db == 2:                                                  # 0 - c2
        qv = np.array(ring.qs, dtype=object)
        hi = np.array((qv - hi.astype(object)) % qv, dtype=np.int64)
    return np.concatenate([shared, hi], axis=1)


@pytest.mark.parametrize("tag,m,qs,word,vw", uniform_rings(), ids=[r[0] for r in uniform_rings()])
def test_against_scale_mulg_add(tag, m, qs, word, vw):
    """out = s_a g^g_a a + s_b g^g_b b equals scale + mulG x d + add of the existing entry points: batches 1, 3, 37, the four g-power
    pairs, the four degree pairs, scalars on both sides or NULL on either, the subtraction through alch_buf_sub, the unary form, out
    aliasing a and aliasing b; operands that are not the output keep their checksums."""
    ring = A.Ring(m, qs)
    n, L = ring.n, ring.L
    assert ring.word_bytes == word and (n % (16 // word) == 0) == (vw > 1)
    rng = np.random.default_rng(m + word)
    combo = 0
    for batch in BATCHES:
        a = {d: ring.alloc((d + 1) * batch) for d in (1, 2)}
        b = {d: ring.alloc((d + 1) * batch) for d in (1, 2)}
        for d in (1, 2):
            a[d].fill_uniform(100 * batch + d)
            b[d].fill_uniform(200 * batch + d)
        sums = {("a", d): a[d].checksum() for d in (1, 2)}
        sums.update({("b", d): b[d].checksum() for d in (1, 2)})
        for da, db in DEG_PAIRS:
            do = max(da, db)
            for g_a, g_b in G_PAIRS:
                combo += 1
                s_a, s_b = [(scalars(rng, qs), scalars(rng, qs)), (None, scalars(rng, qs)), (scalars(rng, qs), None)][combo % 3]
                ta = reference_term(ring, a[da], da, batch, s_a, g_a, ALCH_BASIS_CRT)
                tb = reference_term(ring, b[db], db, batch, s_b, g_b, ALCH_BASIS_CRT)
                want = reference_sum(ring, ta, da, tb, db, batch, n, L)
                out = ring.alloc((do + 1) * batch)
                out.fill_uniform(7)
                ct_add_raw(out, batch, a[da], da, s_a, g_a, b[db], db, s_b, g_b)
                got = out.download().reshape(batch, do + 1, n, L)
                assert np.array_equal(got, want), (batch, da, db, g_a, g_b)
                assert_reduced(got, qs)
                # out aliasing an operand of the result's degree: the same words
                if da == do:
                    alias = ring.alloc((da + 1) * batch)
                    alias.copy_from(a[da], (da + 1) * batch)
                    ct_add_raw(alias, batch, alias, da, s_a, g_a, b[db], db, s_b, g_b)
                    assert np.array_equal(alias.download().reshape(got.shape), want), ("out = a", batch, da, db, g_a, g_b)
                if db == do:
                    alias = ring.alloc((db + 1) * batch)
                    alias.copy_from(b[db], (db + 1) * batch)
                    ct_add_raw(alias, batch, a[da], da, s_a, g_a, alias, db, s_b, g_b)
                    assert np.array_equal(alias.download().reshape(got.shape), want), ("out = b", batch, da, db, g_a, g_b)
                # the subtraction: -s_b as b's scalar against alch_buf_sub of the same terms
                if s_b is not None and combo % 2:
                    ct_add_raw(out, batch, a[da], da, s_a, g_a, b[db], db, [q - v for q, v in zip(qs, s_b)], g_b)
                    want_sub = reference_sum(ring, ta, da, tb, db, batch, n, L, sub=True)
                    assert np.array_equal(out.download().reshape(got.shape), want_sub), ("sub", batch, da, db, g_a, g_b)
        # the unary form, both degrees: scalar and g-power, g-power alone, scalar alone, neither (a copy)
        for d in (1, 2):
            for s, g in ((scalars(rng, qs), 2), (None, 3), (scalars(rng, qs), 0), (None, 0)):
                want = reference_term(ring, a[d], d, batch, s, g, ALCH_BASIS_CRT).download()
                out = ring.alloc((d + 1) * batch)
                ct_add_raw(out, batch, a[d], d, s, g, None, 7, [1] * L, 99)        # deg_b, s_b, g_b are ignored without b
                assert np.array_equal(out.download(), want), ("unary", batch, d, g)
        assert sums == {**{("a", d): a[d].checksum() for d in (1, 2)}, **{("b", d): b[d].checksum() for d in (1, 2)}}


@pytest.mark.parametrize("batch,mib", [(37, None), (1500, 1)])
def test_pow_basis_with_g_powers(batch, mib):
    """ALCH_POW_IN | ALCH_POW_OUT on m' = 45 with g-powers: the operands go through the batched mulG of the Pow basis into the ring's
    scratch, then the pass.  Reference: alch_buf_scale, alch_buf_mulg(Pow), alch_buf_add.  batch 37 fits one chunk at any accepted
    "scratch_mib" (its smallest value is 1 MiB, and a quadratic ciphertext here is 864 bytes), so the chunk walk is run at batch
    1500 with 1 MiB: 606 ciphertexts per chunk when both operands are quadratic and both carry a g-power, three chunks."""
    qs = primes_1_mod(45, 3, 1 << 29)
    ring = A.Ring(45, qs)
    if mib is not None:
        ring.set_option("scratch_mib", mib)
        assert batch * 6 * ring.n * ring.L * 4 > 2 * (mib << 20)
    n, L = ring.n, ring.L
    rng = np.random.default_rng(batch)
    for (da, db), (g_a, g_b) in zip(DEG_PAIRS + [(2, 2)], G_PAIRS + [(1, 2)]):
        a, b = ring.alloc((da + 1) * batch), ring.alloc((db + 1) * batch)
        a.fill_uniform(11 + da)
        b.fill_uniform(13 + db)
        before = (a.checksum(), b.checksum())
        s_a, s_b = scalars(rng, qs), scalars(rng, qs)
        ta = reference_term(ring, a, da, batch, s_a, g_a, ALCH_BASIS_POW)
        tb = reference_term(ring, b, db, batch, s_b, g_b, ALCH_BASIS_POW)
        if da == db or batch <= 37:
            want = reference_sum(ring, ta, da, tb, db, batch, n, L)
        else:                                                            # large batch: gather the components on the host
            xa, xb = ta.download().reshape(batch, da + 1, n, L), tb.download().reshape(batch, db + 1, n, L)
            lo = (xa[:, :2] + xb[:, :2]) % np.array(qs, dtype=np.int64)
            want = np.concatenate([lo, (xa if da == 2 else xb)[:, 2:]], axis=1)
        out = ring.alloc((max(da, db) + 1) * batch)
        ct_add_raw(out, batch, a, da, s_a, g_a, b, db, s_b, g_b, POW)
        assert np.array_equal(out.download().reshape(want.shape), want), (da, db, g_a, g_b)
        if da >= db:                                                     # out = a through the scratch copy
            ct_add_raw(a, batch, a, da, s_a, g_a, b, db, s_b, g_b, POW)
            assert np.array_equal(a.download().reshape(want.shape), want), ("out = a", da, db)
            assert b.checksum() == before[1]
        else:
            assert (a.checksum(), b.checksum()) == before
    # the unary form on the Pow basis: mulGCT of quadratic ciphertexts
    a = ring.alloc(3 * batch)
    a.fill_uniform(5)
    want = reference_term(ring, a, 2, batch, None, 2, ALCH_BASIS_POW).download()
    out = ring.alloc(3 * batch)
    ct_add_raw(out, batch, a, 2, None, 2, None, 0, None, 0, POW)
    assert np.array_equal(out.download(), want)


# ---- worst-case words --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,qs", [(45, primes_1_mod(45, 3, 1 << 29)),
                                  (45, [primes_below(45, 1, 1 << 60)[0], primes_1_mod(45, 1, 1 << 28)[0]]),
                                  (32, primes_1_mod(32, 2, 1 << 28))], ids=["m45", "m45w64", "m32"])
def test_worst_case_words(m, qs):
    """Every operand word q - 1, every scalar q - 1: the result is s_a G^g_a a + s_b G^g_b b in Python integers, G = the model's CRT
    image of g (1 on a two-power index), and every stored word is below its modulus."""
    ring = A.Ring(m, qs)
    n, L, batch = ring.n, ring.L, 3
    idx = G.Index(m)
    gimg = [G.g_crt(idx, q) for q in qs]                                 # [limb][slot]
    top = np.ascontiguousarray(np.broadcast_to(np.array([q - 1 for q in qs], dtype=np.int64), (3 * batch, n, L)))
    s = [q - 1 for q in qs]
    for da, db in DEG_PAIRS:
        a, b = ring.upload(top[:(da + 1) * batch]), ring.upload(top[:(db + 1) * batch])
        for g_a, g_b in G_PAIRS:
            out = ring.alloc((max(da, db) + 1) * batch)
            ct_add_raw(out, batch, a, da, s, g_a, b, db, s, g_b)
            got = out.download().reshape(batch, max(da, db) + 1, n, L)
            assert_reduced(got, qs)
            for j, q in enumerate(qs):
                fa = [(q - 1) * pow(gv, g_a, q) * (q - 1) % q for gv in gimg[j]]
                fb = [(q - 1) * pow(gv, g_b, q) * (q - 1) % q for gv in gimg[j]]
                both = [(u + v) % q for u, v in zip(fa, fb)]
                for i in range(max(da, db) + 1):
                    want = both if i <= min(da, db) else (fa if da > db else fb)
                    assert all(got[ct, i, :, j].tolist() == want for ct in range(batch)), (da, db, g_a, g_b, j, i)


# ---- statuses and the empty batch --------------------------------------------------------------------------------------------------
def test_statuses_and_the_empty_batch():
    qs = primes_1_mod(45, 2, 1 << 29)
    ring, other = A.Ring(45, qs), A.Ring(45, qs)
    nocrt = A.Ring(45, [7], nocrt=True)
    a, b, out, small = ring.alloc(6), ring.alloc(6), ring.alloc(6), ring.alloc(3)
    foreign, zn = other.alloc(6), nocrt.alloc(6)
    a.fill_uniform(1)
    b.fill_uniform(2)
    out.fill_uniform(3)
    before = out.checksum()

    def status(*args):
        with pytest.raises(capi.AlchemyError) as e:
            ct_add_raw(*args)
        return e.value.code

    def still_answers():
        """After an error the ring still gives the right words."""
        got = ring.alloc(4)
        ct_add_raw(got, 2, a, 1, None, 0, b, 1, None, 0)
        want = ring.alloc(4)
        want.add(a, b, 4)
        assert np.array_equal(got.download(), want.download())

    INV, UNS, NOCRT = capi.ALCH_E_INVALID, capi.ALCH_E_UNSUPPORTED, capi.ALCH_E_NO_CRT
    checks = [
        ((out, 2, a, 1, None, 0, foreign, 1, None, 0), INV),             # buffers of different rings
        ((foreign, 2, a, 1, None, 0, b, 1, None, 0), INV),
        ((out, 2, a, 0, None, 0, b, 1, None, 0), INV),                   # a degree outside {1, 2}
        ((out, 2, a, 1, None, 0, b, 3, None, 0), INV),
        ((out, 2, a, 1, None, 0, b, 1, None, 0, 4), INV),                # unknown flag
        ((out, 2, a, 1, None, 17, b, 1, None, 0), INV),                  # g-power above 16
        ((out, 2, a, 1, None, 0, b, 1, None, 17), INV),
        ((out, 4, a, 1, None, 0, b, 1, None, 0), INV),                   # batch larger than a buffer holds
        ((out, 3, a, 2, None, 0, b, 2, None, 0), INV),
        ((small, 2, a, 1, None, 0, b, 1, None, 0), INV),
        ((out, (1 << 63) + 1, a, 1, None, 0, b, 1, None, 0), INV),
        ((a, 2, a, 1, None, 0, b, 2, None, 0), INV),                     # out = a, but the result is quadratic
        ((a.view(1, 5), 2, a, 1, None, 0, b, 1, None, 0), INV),          # a shifted overlap
        ((out, 2, a, 1, None, 0, b, 1, None, 0, ALCH_POW_IN), UNS),      # one basis flag alone
        ((out, 2, a, 1, None, 0, b, 1, None, 0, ALCH_POW_OUT), UNS),
        ((zn, 2, zn, 1, None, 1, None, 0, None, 0), NOCRT),              # no CRT basis, a g-power on it
        ((zn, 2, zn, 1, None, 0, zn, 1, None, 0), UNS),                  # as alch_buf_scale answers such a ring
    ]
    for args, code in checks:
        assert status(*args) == code, args[1:]
        assert out.checksum() == before
        still_answers()
    # the empty batch: ALCH_OK, nothing written -- also with buffers that hold nothing to spare
    for flags in (0, POW):
        ct_add_raw(out, 0, a, 2, [1, 1], 3, b, 1, None, 0, flags)
        ct_add_raw(out, 0, a, 1, None, 0, None, 0, None, 0, flags)
    assert out.checksum() == before
    # errors come before the empty batch
    assert status(out, 0, a, 1, None, 0, foreign, 1, None, 0) == INV
    still_answers()


def test_metadata_wrappers_allocate_and_alias():
    """ct_add / ct_sub / ct_neg allocate the result at the result's degree, accept `out`, and return the rule's metadata."""
    qs = primes_1_mod(45, 2, 1 << 29)
    ring = A.Ring(45, qs)
    batch = 3
    a, b = ring.alloc(3 * batch), ring.alloc(2 * batch)
    a.fill_uniform(1)
    b.fill_uniform(2)
    ma, mb = CtMeta("LSD", 1, 3, 7, 2), CtMeta("MSD", 0, 1, 7, 1)
    out, meta = ct_add(a, ma, b, mb, batch)
    s_a, g_a, s_b, g_b, want_meta = align(ma, mb, qs)
    assert meta == want_meta and out.n_elems == 3 * batch and (g_a, g_b) == (0, 1) and s_a is not None
    ref = ring.alloc(3 * batch)
    ct_add_raw(ref, batch, a, 2, s_a, g_a, b, 1, s_b, g_b)
    assert np.array_equal(out.download(), ref.download())
    same, _ = ct_sub(a, ma, b, mb, batch, out=a)
    assert same is a
    neg, meta_n = ct_neg(b, mb, batch)
    assert meta_n == mb and neg.n_elems == 2 * batch
    back, _ = ct_neg(neg, mb, batch, out=neg)
    assert np.array_equal(back.download(), b.download())
