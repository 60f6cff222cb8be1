"""GPU: ring tunnels between TWO-POWER rings of the radix-16 engine (r', s' >= 32) through the C ABI and the ctypes binding
(alch_tunnel_info / alch_tunnel_create / alch_ct_tunnel -> do_tunnel_pow2).  Every comparison is bit-exact, against the C
restatement's composition (helpers.oracle_tunnel, the general-index oracle, which knows nothing of the closed-form index maps the
device uses) or against the model-generated fixture tests/golden/tunnel_twopower_small.json.

Before this path existed alch_tunnel_create answered ALCH_E_UNSUPPORTED ("tunnelling runs on general-index rings with a CRT basis") for
every pair used here, so the fixture test and the parity tests fail on the parent commit with that status."""
import numpy as np
import pytest

import alchemy_amd as A
from alchemy_amd import capi
from helpers import assert_reduced, load_golden, oracle_tunnel, primes_1_mod, to_aos

pytestmark = pytest.mark.gpu

GADGETS = {"triv": capi.ALCH_GAD_TRIV, "base2": capi.ALCH_GAD_BASE2}
PAIRS = [(32, 64), (64, 32), (64, 512), (512, 64), (1 << 12, 1 << 13), (1 << 14, 1 << 11), (1 << 16, 1 << 17), (1 << 17, 1 << 16)]
SMALL = 512                                   # pairs up to this index also run every ALCH_POW_IN / ALCH_POW_OUT combination


def rand_elems(rng, count, n, qs):
    return np.stack([np.stack([rng.integers(0, q, size=n, dtype=np.int64) for q in qs], axis=1) for _ in range(count)])


_SERVED = []


def need_twopower_tunnels():
    """First line of every test here: one tiny (32 -> 64) tunnel, created once per session.  Where alch_tunnel_create refuses it the
    test fails at once with the library's status and message -- before it has made a ring or a buffer of its own.  A failing test's
    frames stay alive in pytest's exception cycle until the garbage collector finalizes what they hold in any order, and the
    binding's buffers must be freed before their ring is destroyed; here everything is freed by reference counting, in that order."""
    if not _SERVED:
        qs = primes_1_mod(64, 1, 1 << 29)
        gr, gs = A.Ring(32, qs), A.Ring(64, qs)
        lin, ks = gs.alloc(1), gs.alloc(2)
        try:
            A.Tunnel(gr, gs, lin, ks).free()
            _SERVED.append("")
        except A.AlchemyError as e:
            _SERVED.append("alch_tunnel_create on two-power rings (32 -> 64): status %d, %s" % (e.code, e))
    if _SERVED[0]:
        pytest.fail(_SERVED[0])


def check_parity(oracle_lib, rp, sp, qs, gadget, batch, with_s_pre, flag_sets=(0,), scratch_mib=None, seed=0, words=rand_elems,
                 s_pre=None, word_bytes=None, operands=None):
    """Random linear function, hints and ciphertexts (parity does not need them valid) through Tunnel.apply, every ciphertext
    word for word against oracle_tunnel; every stored word below its modulus; the input buffer is left untouched.
    words(rng, count, n, qs): the word generator (uniform unless given); s_pre: a scalar vector to use instead of a random one;
    word_bytes: the word size both rings must have; operands(rng, d_rel, D, n_r, n_s) -> (lin, ks, cts): the operands themselves,
    instead of three draws from `words` (it runs before anything is uploaded)."""
    L = len(qs)
    gr, gs = A.Ring(rp, qs), A.Ring(sp, qs)
    if word_bytes is not None:
        assert gr.word_bytes == gs.word_bytes == word_bytes
    if scratch_mib is not None:
        gs.set_option("scratch_mib", scratch_mib)
    ep, d_rel = A.Tunnel.info(gr, gs)
    assert ep == min(rp, sp) and d_rel == max(1, rp // sp)
    D = gs.gadget_digits(GADGETS[gadget])
    rng = np.random.default_rng(rp * 131 + sp + 7 * L + seed)
    if operands is not None:
        lin, ks, cts = operands(rng, d_rel, D, gr.n, gs.n)
        assert lin.shape == (d_rel, gs.n, L) and ks.shape == (2 * d_rel * D, gs.n, L) and cts.shape == (2 * batch, gr.n, L)
    else:
        lin, ks = words(rng, d_rel, gs.n, qs), words(rng, 2 * d_rel * D, gs.n, qs)
        cts = words(rng, 2 * batch, gr.n, qs)
    if s_pre is None:
        s_pre = [int(rng.integers(1, q)) for q in qs] if with_s_pre else None
    want = [oracle_tunnel(oracle_lib, rp, sp, qs, list(lin), list(ks), cts[2 * ct], cts[2 * ct + 1], s_pre, gadget=gadget)
            for ct in range(batch)]
    Or, Os = oracle_lib.GenRing(rp, qs), oracle_lib.GenRing(sp, qs)
    tun = A.Tunnel(gr, gs, gs.upload(lin), gs.upload(ks), gadget=GADGETS[gadget])
    gout = gs.alloc(2 * batch)
    for flags in flag_sets:
        src = np.stack([Or.crtinv(np.ascontiguousarray(c)) for c in cts]) if flags & capi.ALCH_POW_IN else cts
        gin = gr.upload(src)
        gout.fill_uniform(99)
        tun.apply(gin, gout, batch, s_pre=s_pre, flags=flags)
        got = gout.download()
        assert_reduced(got, qs)
        for ct in range(batch):
            for comp in range(2):
                w = want[ct][comp]
                if flags & capi.ALCH_POW_OUT:
                    w = Os.crtinv(np.ascontiguousarray(w))
                assert np.array_equal(got[2 * ct + comp], w), (rp, sp, L, gadget, flags, ct, comp)
        assert np.array_equal(gin.download(), src)                  # input untouched


def test_tunnel_twopower_fixture():
    """Valid model instances (up: 32 -> 64, down: 64 -> 32; TrivGad and BaseBGad 2; three limbs) through Tunnel.apply with
    POW_IN | POW_OUT: the device's output equals the model's word for word, the input is untouched, and the model decrypts the
    DEVICE's output to f(pt)."""
    need_twopower_tunnels()
    from oracle import model_gen as G
    lm = lambda a: np.asarray(a).T.tolist()
    recs = load_golden("tunnel_twopower_small.json")
    assert sorted((r["rp"], r["sp"], r["gadget"]) for r in recs) == [(32, 64, "base2"), (32, 64, "triv"), (64, 32, "base2"), (64, 32, "triv")]
    for rec in recs:
        qs = rec["qs"]
        gr, gs = A.Ring(rec["rp"], qs), A.Ring(rec["sp"], qs)
        assert A.Tunnel.info(gr, gs) == (rec["ep"], len(rec["lin"]))
        lin = gs.upload(np.stack([to_aos(y) for y in rec["lin"]]))
        ks = gs.upload(np.stack([to_aos(x) for hint_i in rec["hints"] for pair in hint_i for x in pair]))
        lin.crt(); ks.crt()
        tun = A.Tunnel(gr, gs, lin, ks, gadget=GADGETS[rec["gadget"]])
        cin = gr.upload(np.stack([to_aos(c) for c in rec["ct_in"]]))
        cout = gs.alloc(2)
        tun.apply(cin, cout, 1, flags=capi.ALCH_POW_IN | capi.ALCH_POW_OUT)
        got = cout.download()
        assert lm(got[0]) == rec["ct_out"][0] and lm(got[1]) == rec["ct_out"][1], (rec["rp"], rec["sp"], rec["gadget"])
        assert np.array_equal(cin.download(), np.stack([to_aos(c) for c in rec["ct_in"]]))      # input untouched
        T = G.tunnel_indices(rec["r"], rec["s"], rec["rp"], rec["sp"])
        dev = G.GCT(G.MSD, 0, rec["ct_out_l"], [lm(got[0]), lm(got[1])], rec["p"], qs, T.sp, T.s)
        assert G.g_decrypt(rec["sk_out"], G.g_mod_switch_down(dev, 1)) == rec["f_of_pt"]


@pytest.mark.parametrize("with_s_pre", [False, True], ids=["no_s_pre", "s_pre"])
@pytest.mark.parametrize("gadget", ["triv", "base2"])
@pytest.mark.parametrize("L", [1, 3, 6])
@pytest.mark.parametrize("rp,sp", PAIRS)
def test_tunnel_twopower_matches_the_oracle(oracle_lib, rp, sp, L, gadget, with_s_pre):
    """Random parity on 32-bit moduli just above 2^29.  Batches of 2 .. 5 ciphertexts (a batch that is no multiple of the kernels'
    four-ciphertext tile included); the pairs up to index 512 run all four ALCH_POW_IN / ALCH_POW_OUT combinations.
    The 2^16 / 2^17 pairs (n = 2^15 / 2^16: the split transforms on the 2^17 side) run TrivGad on 2 ciphertexts and BaseBGad 2 -- D / L = 30
    times the oracle work per ciphertext at six limbs, about half a minute -- on one, at the full six limbs."""
    need_twopower_tunnels()
    qs = primes_1_mod(max(rp, sp), L, 1 << 29)
    big = max(rp, sp) > (1 << 14)
    batch = (1 if gadget == "base2" else 2) if big else 2 + (rp // 32 + sp + L) % 4
    flag_sets = (0, capi.ALCH_POW_IN, capi.ALCH_POW_OUT, capi.ALCH_POW_IN | capi.ALCH_POW_OUT) if max(rp, sp) <= SMALL else (0,)
    check_parity(oracle_lib, rp, sp, qs, gadget, batch, with_s_pre, flag_sets)


@pytest.mark.parametrize("gadget", ["triv", "base2"])
@pytest.mark.parametrize("rp,sp", [(1 << 12, 1 << 13), (1 << 13, 1 << 11)])
def test_tunnel_twopower_ragged_batch_over_several_chunks(oracle_lib, rp, sp, gadget):
    """scratch_mib = 1 leaves room for six ciphertexts (TrivGad) or one (BaseBGad 2) per chunk at three limbs: a batch of 7 runs as
    several chunks, the last one ragged."""
    need_twopower_tunnels()
    qs = primes_1_mod(max(rp, sp), 3, 1 << 29)
    check_parity(oracle_lib, rp, sp, qs, gadget, 7, True, (0, capi.ALCH_POW_IN | capi.ALCH_POW_OUT), scratch_mib=1, seed=5)


@pytest.mark.parametrize("gadget", ["triv", "base2"])
@pytest.mark.parametrize("rp,sp", [(64, 128), (128, 64), (1 << 15, 1 << 14), (1 << 14, 1 << 15)])
def test_tunnel_twopower_60_bit_moduli(oracle_lib, rp, sp, gadget):
    """64-bit words (moduli just above 2^59): the plain Montgomery form of the inner product; n = 2^14 is the largest size a 60-bit
    ring transforms whole, index 2^15 the largest pair both of whose rings alch_ring_create accepts."""
    need_twopower_tunnels()
    qs = primes_1_mod(1 << 16, 2, 1 << 59)
    small = max(rp, sp) <= SMALL
    flag_sets = (0, capi.ALCH_POW_IN, capi.ALCH_POW_OUT, capi.ALCH_POW_IN | capi.ALCH_POW_OUT) if small else (0, capi.ALCH_POW_IN)
    check_parity(oracle_lib, rp, sp, qs, gadget, 3 if small else 2, True, flag_sets)


def test_tunnel_twopower_60_bit_split_ring(oracle_lib):
    """n = 2^15 with 60-bit residues is a split ring (index 2^16): both directions against index 2^15, TrivGad, two limbs."""
    need_twopower_tunnels()
    qs = primes_1_mod(1 << 16, 2, 1 << 59)
    check_parity(oracle_lib, 1 << 15, 1 << 16, qs, "triv", 2, True, (0,))
    check_parity(oracle_lib, 1 << 16, 1 << 15, qs, "triv", 2, False, (capi.ALCH_POW_IN | capi.ALCH_POW_OUT,))


@pytest.mark.parametrize("gadget", ["triv", "base2"])
@pytest.mark.parametrize("rp,sp,L,dup", [(64, 512, 4, 1), (64, 512, 4, 2), (1 << 13, 1 << 12, 4, 1), (1 << 13, 1 << 12, 4, 2),
                                         (1 << 12, 1 << 13, 3, 1), (512, 64, 3, 2)])
def test_tunnel_twopower_below_the_hint_ring_equals_mod_switch_then_tunnel(oracle_lib, rp, sp, L, dup, gadget):
    """PT2CT's modSwitch_ .: tunnel_ hint as one call: ciphertexts on the last L - dup limbs of the tunnel's ring go straight into
    alch_ct_tunnel; same residues as alch_ct_mod_switch (up) followed by alch_ct_tunnel, and as the oracle's composition on the
    switched-up ciphertexts -- with CRT and with Pow input."""
    need_twopower_tunnels()
    qs = primes_1_mod(max(rp, sp), L, 1 << 29)
    gr, gs, gsmall = A.Ring(rp, qs), A.Ring(sp, qs), A.Ring(rp, qs[dup:])
    _, d_rel = A.Tunnel.info(gr, gs)
    rng = np.random.default_rng(rp + 3 * dup + L)
    D = gs.gadget_digits(GADGETS[gadget])
    lin, ks = rand_elems(rng, d_rel, gs.n, qs), rand_elems(rng, 2 * d_rel * D, gs.n, qs)
    batch = 3
    cts = rand_elems(rng, 2 * batch, gr.n, qs[dup:])
    s_pre = [int(rng.integers(1, q)) for q in qs]
    tun = A.Tunnel(gr, gs, gs.upload(lin), gs.upload(ks), gadget=GADGETS[gadget])
    gin, gup, g1, g2 = gsmall.upload(cts), gr.alloc(2 * batch), gs.alloc(2 * batch), gs.alloc(2 * batch)
    capi.ct_mod_switch(gin, gup, batch)
    tun.apply(gup, g1, batch, s_pre=s_pre)
    tun.apply(gin, g2, batch, s_pre=s_pre)
    two_calls, one_call = g1.download(), g2.download()
    assert np.array_equal(one_call, two_calls)
    assert np.array_equal(gin.download(), cts)               # input untouched
    up = gup.download()
    for ct in range(batch):
        w0, w1 = oracle_tunnel(oracle_lib, rp, sp, qs, list(lin), list(ks), up[2 * ct], up[2 * ct + 1], s_pre, gadget=gadget)
        assert np.array_equal(one_call[2 * ct], w0) and np.array_equal(one_call[2 * ct + 1], w1), ct
    # Pow-basis input below the hint's ring (modSwitch up commutes with crtInv: it is a per-limb scalar)
    gin.crtinv()
    g2.fill_uniform(5)
    tun.apply(gin, g2, batch, s_pre=s_pre, flags=capi.ALCH_POW_IN)
    assert np.array_equal(g2.download(), two_calls)


@pytest.mark.parametrize("gadget,l_in", [("triv", 3), ("triv", 2), ("base2", 3)])
def test_tunnel_twopower_resident_batch_of_300(oracle_lib, gadget, l_in):
    """alchemy_amd.tunnelhops_pow2.TwoPowerHop at (2^13 -> 2^14), three limbs, 300 seeded ciphertexts (l_in = 2: the input sits one limb
    below the hint's ring).
      * alch_buf_checksum of the whole batch against a second run split into two calls (137 + 163): the device against ITSELF -- it shows
        that the result does not depend on how the batch is cut into calls and chunks, not that it is right;
      * four seeded ciphertexts word for word against oracle_tunnel: THAT is the correctness check."""
    need_twopower_tunnels()
    from alchemy_amd.tunnelhops_pow2 import TwoPowerHop
    B = 300
    hop = TwoPowerHop(1 << 13, 1 << 14, B, l_hint=3, l_in=l_in, gadget=GADGETS[gadget])
    assert (hop.e_prime, hop.d_rel) == (1 << 13, 1)
    res = hop.run()
    whole = res.checksum(0, 2 * B)
    res.fill_uniform(77)
    hop.run(0, 137)
    hop.run(137, B - 137)
    hop.rs.sync()
    assert res.checksum(0, 2 * B) == whole
    qs, dup = hop.qs, hop.lh - l_in
    lin, ks = list(hop.lin_buf.download()), list(hop.ks.download())
    mult = 1
    for q in qs[:dup]:
        mult *= q
    for ct in [int(c) for c in np.random.default_rng(300).choice(B, size=4, replace=False)]:
        x = hop.x.download(2 * ct, 2)
        up = []
        for comp in range(2):                                  # modSwitch up: x -> (0, q_a x), any basis
            scaled = np.stack([(x[comp][:, j].astype(object) * mult % qs[dup + j]).astype(np.int64) for j in range(l_in)], axis=1)
            up.append(np.ascontiguousarray(np.concatenate([np.zeros((hop.rr.n, dup), dtype=np.int64), scaled], axis=1)))
        w0, w1 = oracle_tunnel(oracle_lib, hop.rp, hop.sp, qs, lin, ks, up[0], up[1], None, gadget=gadget)
        got = res.download(2 * ct, 2)
        assert np.array_equal(got[0], w0) and np.array_equal(got[1], w1), ct


def test_tunnel_twopower_hop_with_closing_mod_switch(oracle_lib):
    """TwoPowerHop with l_out < l_hint: modSwitch . tunnel . modSwitch equals the three entry points called one by one."""
    need_twopower_tunnels()
    from alchemy_amd.tunnelhops_pow2 import TwoPowerHop
    hop = TwoPowerHop(1 << 11, 1 << 10, 9, l_hint=4, l_in=3, l_out=2, gadget=capi.ALCH_GAD_TRIV)
    assert (hop.e_prime, hop.d_rel) == (1 << 10, 2)
    got = hop.run().download()
    up, mid, out = hop.rr.alloc(18), hop.rs.alloc(18), hop.ro.alloc(18)
    capi.ct_mod_switch(hop.x, up, 9)
    hop.tun.apply(up, mid, 9)
    capi.ct_mod_switch(mid, out, 9)
    assert np.array_equal(got, out.download())
    assert hop.algorithmic_bytes() == 2 * 8 * (3 * 1024 + 2 * 512)


def test_tunnel_twopower_argument_checks():
    """Different moduli -> ALCH_E_INVALID; a partner on the general engine (two-power below 32, or composite) -> ALCH_E_UNSUPPORTED
    with a message that says so; buffers on the wrong ring -> ALCH_E_INVALID.  None of them faults."""
    need_twopower_tunnels()
    qs = primes_1_mod(1 << 10, 3, 1 << 29)
    gr, gs, gs2 = A.Ring(64, qs[:2]), A.Ring(256, qs[:2]), A.Ring(256, qs[1:])
    assert A.Tunnel.info(gr, gs) == (64, 1) and A.Tunnel.info(gs, gr) == (64, 4)

    class Status:
        def __init__(self, code, text):
            self.code, self.text = code, text

        def __str__(self):
            return self.text

    def status(f):
        # Returns the status as plain values and lets the exception go: a kept exception holds its traceback, the traceback this
        # frame and the frame the exception (a cycle), and the cycle keeps rings, buffers and the tunnel of the calling test alive
        # until the garbage collector runs their finalizers in ANY order -- alch_buf_free / alch_tunnel_free after the
        # alch_ring_destroy of their ring write into freed host memory.  Without a cycle, reference counting frees a buffer and a
        # tunnel before the ring they hold.
        try:
            f()
        except A.AlchemyError as e:
            return Status(e.code, str(e))
        pytest.fail("the call was accepted")

    err = status(lambda: A.Tunnel(gr, gs2, gs2.alloc(1), gs2.alloc(4)))
    assert err.code == capi.ALCH_E_INVALID and "same moduli" in str(err)
    err = status(lambda: A.Tunnel(gr, gs, gs.alloc(1), gs.alloc(3)))                    # too few hint elements
    assert err.code == capi.ALCH_E_INVALID
    err = status(lambda: A.Tunnel(gr, gs, gr.alloc(1), gs.alloc(4)))                    # linear function on the wrong ring
    assert err.code == capi.ALCH_E_INVALID
    for m_gen in (16, 96):                                                               # two-power below 32; composite
        gen = A.Ring(m_gen, primes_1_mod(96 * 64, 2, 1 << 29))
        big = A.Ring(64, primes_1_mod(96 * 64, 2, 1 << 29))
        for a, b in ((gen, big), (big, gen)):
            err = status(lambda: A.Tunnel(a, b, b.alloc(4), b.alloc(16)))
            assert err.code == capi.ALCH_E_UNSUPPORTED and "general-index ring" in str(err), str(err)
    t = A.Tunnel(gr, gs, gs.alloc(1), gs.alloc(4))
    for src, dst in ((gs.alloc(2), gs.alloc(2)), (gr.alloc(2), gr.alloc(2)), (gs2.alloc(2), gs.alloc(2))):
        err = status(lambda: t.apply(src, dst, 1))
        assert err.code == capi.ALCH_E_INVALID
    err = status(lambda: t.apply(gr.alloc(2), gs.alloc(2), 2))                          # buffers too small for the batch
    assert err.code == capi.ALCH_E_INVALID
    t.apply(gr.alloc(2), gs.alloc(2), 0)                                                # empty batch: nothing to do
