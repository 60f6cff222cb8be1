"""GPU: PT2CT's mul_ one SHE operation at a time on resident ciphertext batches -- alch_ct_mul, alch_ct_key_switch_quad and
alch_ct_mod_switch_deg through alchemy_amd/mulsteps.py (kernels k_ct_tensor3 and k_ct_split3, the composed key-switch stage with a
ready c2, modSwitch with three elements per ciphertext).

Every comparison of ring elements is exact.  Two references: the model (oracle/model_gen.py: g_ct_mul, g_mod_switch_up / _down,
g_key_switch on ciphertexts of any degree) for the conventions, and the fused entry points alch_ct_mul_relin / alch_ct_mul_full --
which this feature does not touch -- for every shape and code path, on uniform words.  Error rates are compared with `==`: both
sides are one correctly rounded division of the same two integers.

The package has no `mulsteps` module and the library none of the three symbols before this feature, so this module does not import on
the parent commit and every test in it fails there.

Not exercised: ALCH_E_NO_CRT of alch_ct_key_switch_quad.  It is checked after the ring comparison, and the ring is the hint's; a hint
on a ring without CRT basis is not something the library's own hint constructors are specified for, so no test builds one."""
import random

import numpy as np
import pytest

import alchemy_amd as A
from alchemy_amd import capi
from alchemy_amd import mulsteps as MS
from helpers import primes_1_mod, to_aos

pytestmark = pytest.mark.gpu

TRIV, BASE2 = capi.ALCH_GAD_TRIV, capi.ALCH_GAD_BASE2
POW_IN, POW_OUT = capi.ALCH_POW_IN, capi.ALCH_POW_OUT


def uniform(ring, n_elems, seed):
    b = ring.alloc(n_elems)
    b.fill_uniform(seed)
    return b


def make_hint(ring, gadget, seed):
    hb = uniform(ring, 2 * ring.gadget_digits(gadget), seed)
    return ring.hint_from_buf(hb, gadget=gadget)


def scalars(qs, seed):
    rnd = random.Random(seed)
    return [rnd.randrange(1, q) for q in qs]


def same(x, y, count):
    return np.array_equal(x.download(0, count), y.download(0, count))


class Untouched:
    """Checksums of input buffers, taken at construction and compared by check()."""

    def __init__(self, *bufs):
        self.bufs = bufs
        self.sums = [b.checksum() for b in bufs]

    def check(self):
        assert [b.checksum() for b in self.bufs] == self.sums, "an input buffer was modified"


# ---- the model -------------------------------------------------------------------------------------------------------------------
def model_chain(m, mp, p, direction, seed):
    """A valid model instance over three limbs and PT2CT's four steps on it.  direction "up": the hint on four limbs (TrivGad's extra
    limb), result on three; "down": the hint on two limbs, result on one.  Returns (G, sk, plaintext product, hint, steps), steps =
    [(name, model ciphertext)] for the operands' product, its MSD form, the switched quadratic ciphertext, the key-switched and the
    closing one."""
    from oracle import model_gen as G
    rng = random.Random(seed)
    small, big = G.Index(m), G.Index(mp)
    qs4 = primes_1_mod(mp, 4, 1 << 29)
    qs = qs4[1:]
    sk = G.g_gen_sk(big, rng)
    pa = [rng.randrange(p) for _ in range(small.n)]
    pb = [rng.randrange(p) for _ in range(small.n)]
    ca, cb = G.g_encrypt(sk, pa, small, big, p, qs, rng), G.g_encrypt(sk, pb, small, big, p, qs, rng)
    prod = G.g_ct_mul(ca, cb)
    msd = G.g_to_msd(prod)
    if direction == "up":
        switched = G.g_mod_switch_up(msd, qs4[:1])
    else:
        switched = G.g_mod_switch_down(msd, 1)
    hint = G.g_ks_hint(sk, big, switched.qs, rng)
    ks = G.g_key_switch(hint, switched)
    last = G.g_mod_switch_down(ks, 1)
    want_pt = G.ring_mul_def(pa, pb, small, p)
    return G, sk, want_pt, hint, ca, cb, [("mul_", prod), ("toMSD", msd), ("modSwitch_", switched), ("keySwitchQuad_", ks), ("modSwitch_", last)]


def ct_host(ct, batch):
    """The model ciphertext `batch` times over: (len(c) * batch, n, L) Pow-basis residues."""
    return np.stack([to_aos(c) for c in ct.c] * batch)


def model_rate(G, sk, ct):
    """errorRate_ of a model ciphertext: max |liftDec(c(s))| of its LSD form over Q, as (worst, Q)."""
    lsd = G.g_to_lsd(ct)
    qs = ct.qs
    acc = [[0] * ct.big.n for _ in qs]
    for comp in reversed(lsd.c):
        acc = [[(u + v) % q for u, v in zip(G.ring_mul_def(al, sk, ct.big, q), cl)] for al, cl, q in zip(acc, comp, qs)]
    Q = 1
    for q in qs:
        Q *= q
    return max(abs(v) for v in G.lift_dec(acc, ct.big, qs)), Q


MODEL_CASES = [(16, 32, 8, "up"), (16, 32, 8, "down"), (9, 45, 4, "up"), (9, 45, 7, "down")]
_model_cache = {}


def model_case(case):
    if case not in _model_cache:
        m, mp, p, direction = case
        _model_cache[case] = model_chain(m, mp, p, direction, seed=mp * 100 + p)
    return _model_cache[case]


def sk_buf(ring, sk):
    b = ring.upload(np.stack([to_aos([[v % q for v in sk] for q in ring.qs])]))
    b.crt()
    return b


@pytest.mark.parametrize("case", MODEL_CASES)
def test_every_step_equals_the_model(case):
    """(*), toMSD, modSwitch up or down of the quadratic ciphertext, keySwitchQuadCirc, modSwitch down: every intermediate buffer
    equals the model's, with Pow-basis input and output (ALCH_POW_IN | ALCH_POW_OUT against the model's values directly) and
    CRT-basis in and out (crtInv of a copy against the model); decrypt_batch(degree = 2) of both quadratic intermediates is the
    product of the plaintexts."""
    m, mp, p, direction = case
    G, sk, want_pt, hint, ca, cb, steps = model_case(case)
    batch = 3
    prod, msd, switched, ks, last = [ct for _, ct in steps]
    r_in, r_h, r_out = A.Ring(mp, prod.qs), A.Ring(mp, switched.qs), A.Ring(mp, last.qs)
    ghint = r_h.hint_load(np.stack([x for h0, h1 in hint for x in (sk_crt_elem(r_h, h0), sk_crt_elem(r_h, h1))]))
    inv_p = [pow(p, -1, q) for q in r_in.qs]
    zp_big, zp_small = A.Ring(mp, [p], nocrt=True), A.Ring(m, [p], nocrt=True)

    for pow_basis in (True, False):
        fin, fout = (POW_IN, POW_OUT) if pow_basis else (0, 0)

        def put(ring, ct):
            b = ring.upload(ct_host(ct, batch))
            if not pow_basis:
                b.crt()
            return b

        def check(buf, ct, what):
            want = ct_host(ct, batch)
            if pow_basis:
                got = buf.download(0, want.shape[0])
            else:
                c = buf.ring.alloc(want.shape[0])
                c.copy_from(buf, want.shape[0])
                c.crtinv()
                got = c.download()
            assert np.array_equal(got, want), (case, pow_basis, what)

        a, b = put(r_in, ca), put(r_in, cb)
        keep = Untouched(a, b)
        quad = MS.ct_mul(a, b, batch, flags=fin | fout)
        check(quad, prod, "mul_")
        quad_msd = r_in.alloc(3 * batch)
        quad_msd.scale(quad, 3 * batch, inv_p)
        check(quad_msd, msd, "toMSD")
        keep2 = Untouched(quad_msd)
        sw = MS.mod_switch(quad_msd, r_h, batch, degree=2, flags=fin | fout)
        check(sw, switched, "modSwitch_ (degree 2)")
        keep3 = Untouched(sw)
        lin = MS.key_switch_quad(ghint, sw, batch, flags=fin | fout)
        check(lin, ks, "keySwitchQuad_")
        keep4 = Untouched(lin)
        res = MS.mod_switch(lin, r_out, batch, degree=1, flags=fin | fout)
        check(res, last, "modSwitch_")
        for k in (keep, keep2, keep3, keep4):
            k.check()
        for ring, buf, ct in ((r_in, quad, prod), (r_h, sw, switched)):
            lsd = G.g_to_lsd(ct)
            s_pre = None if ct.enc == G.LSD else [p % q for q in ring.qs]
            pt = A.decrypt_batch(buf, batch, sk_buf(ring, sk), zp_big, zp_small, lsd.k, lsd.l, degree=2, s_pre=s_pre, flags=fin)
            got = pt.download(0, batch)
            for i in range(batch):
                assert got[i, :, 0].tolist() == want_pt, (case, pow_basis, i)


def sk_crt_elem(ring, elem_pow):
    """One model ring element (limb-major Pow residues) as a CRT-basis (n, L) array, transformed by the library itself."""
    b = ring.upload(np.stack([to_aos(elem_pow)]))
    b.crt()
    return b.download()[0]


@pytest.mark.parametrize("case", MODEL_CASES)
def test_mul_steps_error_rates(case):
    """mul_steps on a valid instance: the same result as the step calls, and the ErrorRateWriter's four entries, each equal to the rate
    computed from the model's intermediate by lift_dec.  Monotone where the arithmetic says so, and only there:
      up    modSwitch_ to more limbs multiplies error and modulus by the same q_a: the rate is unchanged, exactly.  Nothing is asserted
            about keySwitchQuad_ here -- with TrivGad's extra limb its noise (about n q / Q) lies BELOW the product's own error.
      down  modSwitch_ of the quadratic ciphertext to fewer limbs adds a rounding term of order 1 / Q' to an error of order
            10^-24 Q: the rate rises; keySwitchQuad_ on two limbs then adds digits of size q / 2 times the hint's errors, about
            n q / Q' ~ 10^-8 against ~ 10^-15: the rate rises again.  Nothing is asserted about the closing modSwitch_: its rounding
            term and the key switch's noise are of the same order."""
    m, mp, p, direction = case
    G, sk, want_pt, hint, ca, cb, steps = model_case(case)
    batch = 3
    prod, msd, switched, ks, last = [ct for _, ct in steps]
    r_in, r_h, r_out = A.Ring(mp, prod.qs), A.Ring(mp, switched.qs), A.Ring(mp, last.qs)
    ghint = r_h.hint_load(np.stack([x for h0, h1 in hint for x in (sk_crt_elem(r_h, h0), sk_crt_elem(r_h, h1))]))
    a, b = r_in.upload(ct_host(ca, batch)), r_in.upload(ct_host(cb, batch))
    a.crt()
    b.crt()
    keys = {r: sk_buf(r, sk) for r in (r_in, r_h, r_out)}
    res, log = A.mul_steps(ghint, a, b, r_in, r_h, r_out, sk_by_ring=keys, p=p, flags=POW_OUT)
    assert np.array_equal(res.download(0, 2 * batch), ct_host(last, batch))
    assert [name for name, _ in log] == ["mul_", "modSwitch_", "keySwitchQuad_", "modSwitch_"]
    for (name, rates), ct in zip(log, (prod, switched, ks, last)):
        worst, Q = model_rate(G, sk, ct)
        assert rates == [worst / Q] * batch, (case, name, rates, worst / Q)
    r = [rates[0] for _, rates in log]
    if direction == "up":
        assert r[1] == r[0]
    else:
        assert r[0] < r[1] < r[2]
    assert A.mul_steps(ghint, a, b, r_in, r_h, r_out, p=p, flags=POW_OUT).checksum(0, 2 * batch) == res.checksum(0, 2 * batch)


# ---- step chain == fused entry points -----------------------------------------------------------------------------------------------
# (id, m, modulus bits, limbs of the largest ring, batch, {gadget: (L_in, L_h, L_out) of the mul_full comparison}, options tried on every ring)
SHAPES = [
    ("n1024", 1 << 11, 30, 4, 3, {TRIV: (3, 4, 2), BASE2: (4, 3, 2)}, [{}]),                 # fused kernels on the reference side
    ("n65536", 1 << 17, 30, 3, 3, {TRIV: (2, 3, 2)}, [{}, {"split_fused": 1}, {"split_fused": 0}]),   # split transforms, 32-bit words
    ("n32768_64", 1 << 16, 59, 3, 3, {TRIV: (2, 3, 1)}, [{}, {"split_fused": 0}]),           # split transforms, 64-bit words
    ("H0", 11648, 30, 4, 4, {TRIV: (3, 4, 2), BASE2: (4, 3, 2)}, [{}, {"gen_fused": 0, "rs_lin": 0}]),   # H0' of the reference, n = 4608
    ("m45", 45, 30, 4, 3, {TRIV: (2, 4, 3), BASE2: (4, 2, 1)}, [{}, {"rs_lin": 0}]),         # general index, two limbs added (dup = 2)
    ("m27", 27, 30, 3, 3, {TRIV: (2, 3, 1), BASE2: (3, 2, 1)}, [{}]),                        # n = 18: one word per lane
    ("ragged", 1 << 13, 30, 4, 5, {TRIV: (3, 4, 2), BASE2: (4, 3, 2)}, [{"scratch_mib": 1}]),  # batch 5 over chunks of 1, 2 or 4
]


def shape_rings(m, bits, L):
    qs = primes_1_mod(m, L, 1 << (bits - 1))
    return qs, [A.Ring(m, qs[L - k:]) for k in range(1, L + 1)]                              # rings[k - 1]: the last k limbs


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_chain_equals_mul_relin(shape):
    """key_switch_quad(mul(a, b, s)) == mul_relin(a, b, s), also with s split between the two calls, both gadgets where listed,
    under every listed option set; operands untouched."""
    _, m, bits, L, batch, gadgets, optsets = shape
    qs, rings = shape_rings(m, bits, L)
    ring = rings[-1]
    a, b = uniform(ring, 2 * batch, 11), uniform(ring, 2 * batch, 12)
    keep = Untouched(a, b)
    s, s1 = scalars(qs, 5), scalars(qs, 6)
    s2 = [x * pow(y, -1, q) % q for x, y, q in zip(s, s1, qs)]
    for gadget in gadgets:
        hint = make_hint(ring, gadget, 13 + gadget)
        for s_pre in (None, s):
            want = ring.alloc(2 * batch)
            ring.ct_mul_relin(hint, a, b, want, batch, s_pre=s_pre)
            for opts in optsets:
                for k, v in opts.items():
                    ring.set_option(k, v)
                quad = MS.ct_mul(a, b, batch, s_pre=s_pre)
                kq = Untouched(quad)
                assert same(MS.key_switch_quad(hint, quad, batch), want, 2 * batch), (shape[0], gadget, s_pre is None, opts)
                kq.check()
                if s_pre is not None:
                    quad = MS.ct_mul(a, b, batch, s_pre=s1)
                    assert same(MS.key_switch_quad(hint, quad, batch, s_pre=s2), want, 2 * batch), (shape[0], gadget, "split s", opts)
    keep.check()


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_chain_equals_mul_full(shape):
    """TrivGad: mod_switch(key_switch_quad(mod_switch_deg(mul, up, 2))) == mul_full over L_in -> L_h -> L_out limbs.  BaseBGad 2 where
    listed: the hint on fewer limbs than the product, mod_switch(key_switch_quad(mod_switch_deg(mul, down, 2))) == mul_full."""
    name, m, bits, L, batch, gadgets, optsets = shape
    qs, rings = shape_rings(m, bits, L)
    s = scalars(qs, 7)
    for gadget, (l_in, l_h, l_out) in gadgets.items():
        r_in, r_h, r_out = rings[l_in - 1], rings[l_h - 1], rings[l_out - 1]
        a, b = uniform(r_in, 2 * batch, 21), uniform(r_in, 2 * batch, 22)
        keep = Untouched(a, b)
        hint = make_hint(r_h, gadget, 23 + gadget)
        s_pre = s[L - r_in.L:]
        want = r_out.alloc(2 * batch)
        capi.ct_mul_full(hint, a, b, want, batch, s_pre=s_pre)
        for opts in optsets:
            for r in rings:
                for k, v in opts.items():
                    r.set_option(k, v)
            quad = MS.ct_mul(a, b, batch, s_pre=s_pre)
            kq = Untouched(quad)
            sw = MS.mod_switch(quad, r_h, batch, degree=2)
            ksw = Untouched(sw)
            lin = MS.key_switch_quad(hint, sw, batch)
            got = r_out.alloc(2 * batch)
            capi.ct_mod_switch(lin, got, batch)
            assert same(got, want, 2 * batch), (name, gadget, opts)
            kq.check()
            ksw.check()
        keep.check()


def test_flags_on_uniform_words():
    """ALCH_POW_IN / ALCH_POW_OUT of alch_ct_mul and alch_ct_key_switch_quad against the CRT-basis calls and the library's own batched
    transforms, on a split ring (in-place transforms, copies first), an LDS-resident and a general one, chunked by scratch_mib."""
    for m, bits, L, batch in ((1 << 17, 30, 2, 3), (1 << 13, 30, 4, 5), (45, 30, 3, 5)):
        qs = primes_1_mod(m, L, 1 << (bits - 1))
        ring = A.Ring(m, qs)
        if m != 1 << 17:
            ring.set_option("scratch_mib", 1)                             # n = 4096: (*) in chunks of 4, the key switch one at a time
        hint = make_hint(ring, TRIV, 3)
        a, b = uniform(ring, 2 * batch, 1), uniform(ring, 2 * batch, 2)
        ap, bp = ring.alloc(2 * batch), ring.alloc(2 * batch)
        ap.copy_from(a, 2 * batch)
        bp.copy_from(b, 2 * batch)
        ap.crtinv()
        bp.crtinv()
        keep = Untouched(a, b, ap, bp)
        quad = MS.ct_mul(a, b, batch)
        assert same(MS.ct_mul(ap, bp, batch, flags=POW_IN), quad, 3 * batch), m
        qp = MS.ct_mul(ap, bp, batch, flags=POW_IN | POW_OUT)
        kq = Untouched(quad)
        lin = MS.key_switch_quad(hint, quad, batch)
        assert same(MS.key_switch_quad(hint, qp, batch, flags=POW_IN), lin, 2 * batch), m
        lp = MS.key_switch_quad(hint, qp, batch, flags=POW_IN | POW_OUT)
        qp.crt()
        assert same(qp, quad, 3 * batch), m
        lp.crt()
        assert same(lp, lin, 2 * batch), m
        keep.check()
        kq.check()


# ---- degree 1 == alch_ct_mod_switch -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1 << 11, 45])
def test_degree_one_is_alch_ct_mod_switch(m):
    """alch_ct_mod_switch_deg(degree = 1) against alch_ct_mod_switch word for word: up, down by one and by two limbs, every flag
    combination, on a two-power and a general ring."""
    batch = 3
    qs, rings = shape_rings(m, 30, 4)
    for l_from, l_to in ((2, 4), (3, 4), (4, 3), (4, 2), (3, 1)):
        r_from, r_to = rings[l_from - 1], rings[l_to - 1]
        src = uniform(r_from, 2 * batch, 40 + l_from)
        keep = Untouched(src)
        for flags in (0, POW_IN, POW_OUT, POW_IN | POW_OUT):
            want, got = r_to.alloc(2 * batch), r_to.alloc(2 * batch)
            capi.ct_mod_switch(src, want, batch, flags)
            MS.mod_switch(src, r_to, batch, degree=1, flags=flags, out=got)
            assert same(got, want, 2 * batch), (m, l_from, l_to, flags)
        keep.check()


# ---- statuses ------------------------------------------------------------------------------------------------------------------------
def test_statuses_and_empty_batches():
    lib = capi.load_library()
    mul, ksq, msd = lib.alch_ct_mul, lib.alch_ct_key_switch_quad, lib.alch_ct_mod_switch_deg
    qs = primes_1_mod(64, 3, 1 << 29)
    ring, low, other = A.Ring(64, qs), A.Ring(64, qs[1:]), A.Ring(64, qs[:2])                # low: a suffix of ring; other: not
    twin, r32 = A.Ring(64, qs), A.Ring(32, primes_1_mod(32, 2, 1 << 29))
    zp2, zp1 = A.Ring(64, [8, 7], nocrt=True), A.Ring(64, [7], nocrt=True)
    batch = 2
    a, b, quad, lin = uniform(ring, 2 * batch, 1), uniform(ring, 2 * batch, 2), uniform(ring, 3 * batch, 3), uniform(ring, 2 * batch, 4)
    big = uniform(ring, 3 * batch, 5)
    lowq, lowl = uniform(low, 3 * batch, 6), uniform(low, 2 * batch, 7)
    hint = make_hint(ring, TRIV, 8)
    za, zq, zl = zp2.alloc(3 * batch), zp2.alloc(3 * batch), zp1.alloc(3 * batch)
    keep = Untouched(a, b, quad, lin, big, lowq, lowl)
    R, H = ring._h, hint._h
    tmp = {"twin": twin.alloc(2 * batch), "low3": low.alloc(3 * batch), "view": a.view(0, 2 * batch), "short": ring.alloc(2 * batch - 1),
           "other": other.alloc(3 * batch), "r32": r32.alloc(3 * batch)}                       # handles outlive the calls below

    # batch 0: success, nothing written
    assert mul(R, a._h, b._h, quad._h, 0, None, 0) == 0
    assert ksq(H, quad._h, lin._h, 0, None, 0) == 0
    assert msd(quad._h, lowq._h, 0, 2, 0) == 0 and msd(lowl._h, lin._h, 0, 1, 0) == 0
    keep.check()

    invalid = [
        (mul, (None, a._h, b._h, quad._h, batch, None, 0)), (mul, (R, None, b._h, quad._h, batch, None, 0)),
        (mul, (R, a._h, None, quad._h, batch, None, 0)), (mul, (R, a._h, b._h, None, batch, None, 0)),      # null handles
        (mul, (twin._h, a._h, b._h, quad._h, batch, None, 0)),                                               # another ring handle
        (mul, (R, tmp["twin"]._h, b._h, quad._h, batch, None, 0)),                                 # operand of another ring
        (mul, (R, a._h, b._h, tmp["low3"]._h, batch, None, 0)),                                     # output of another ring
        (mul, (R, a._h, b._h, quad._h, batch + 1, None, 0)),                                                 # operands too small
        (mul, (R, a._h, b._h, lin._h, batch, None, 0)),                                                      # out holds 2*batch only
        (mul, (R, a._h, b._h, quad._h, batch, None, 4)),                                                     # unknown flag
        (mul, (R, big._h, b._h, big._h, batch, None, 0)),                                                    # out aliases an operand
        (mul, (R, a._h, b._h, tmp["view"]._h, 1, None, 0)),                                         # ... through a view
        (ksq, (None, quad._h, lin._h, batch, None, 0)), (ksq, (H, None, lin._h, batch, None, 0)), (ksq, (H, quad._h, None, batch, None, 0)),
        (ksq, (H, lowq._h, lin._h, batch, None, 0)),                                                         # input not on the hint's ring
        (ksq, (H, quad._h, lowl._h, batch, None, 0)),                                                        # output not on the hint's ring
        (ksq, (H, lin._h, a._h, batch, None, 0)),                                                            # input holds 2*batch only
        (ksq, (H, quad._h, tmp["short"]._h, batch, None, 0)),                                   # output too small
        (ksq, (H, quad._h, lin._h, batch, None, 8)),                                                         # unknown flag
        (ksq, (H, big._h, big._h, batch, None, 0)),                                                          # out aliases the input
        (msd, (None, lowq._h, batch, 2, 0)), (msd, (quad._h, None, batch, 2, 0)),
        (msd, (quad._h, lowq._h, batch, 2, 4)),                                                              # unknown flag
        (msd, (quad._h, lowq._h, batch, 0, 0)), (msd, (quad._h, lowq._h, batch, 3, 0)),                      # degree
        (msd, (quad._h, big._h, batch, 2, 0)),                                                               # same number of limbs
        (msd, (quad._h, tmp["other"]._h, batch, 2, 0)),                                            # not the LAST limbs
        (msd, (quad._h, tmp["r32"]._h, batch, 2, 0)),                                              # another index
        (msd, (lin._h, lowq._h, batch, 2, 0)),                                                               # input holds 2*batch only
        (msd, (quad._h, lowl._h, batch, 2, 0)),                                                              # output holds 2*batch only
        (msd, (lowl._h, tmp["short"]._h, batch, 1, 0)),                                         # up, output too small
    ]
    for fn, args in invalid:
        rc = fn(*args)
        msg = lib.alch_last_error().decode()
        assert rc == capi.ALCH_E_INVALID and msg, (fn.__name__, args, rc, msg)
    # rings created with alch_ring_create_nocrt: everything else about the call is valid
    for fn, args in [(mul, (zp2._h, za._h, za._h, zq._h, batch, None, 0)), (msd, (zq._h, zl._h, batch, 2, 0)),
                     (msd, (zl._h, zq._h, batch, 2, 0)), (msd, (zq._h, zl._h, batch, 1, 0))]:
        rc = fn(*args)
        assert rc == capi.ALCH_E_NO_CRT and lib.alch_last_error().decode(), (fn.__name__, rc)
    keep.check()
    assert lib.alch_version() == (1 << 16) | 8                                                               # added within 1.8
