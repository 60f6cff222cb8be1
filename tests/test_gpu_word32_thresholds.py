"""GPU: the lazy 64-bit sums of the 32-bit word path at every modulus threshold where their group size changes.

Inner products (k_tun2_mac<u32>, k_tunnel_mac_e and the composed general-index path, k_pt_mac<u32>): K = lazy_group(q) products are
summed in 64 bits between two Montgomery reductions, K = min(8, floor((2^32 - 1) / q) - 2), none below K = 2.  Every class
kmax = floor((2^32 - 1) / q) = 2 .. 11 (K = 0, 0, 2, 3, 4, 5, 6, 7, 8, 8; class 2 reaches up to 2^31 and holds the reference's own
moduli; the BaseBGad 2 and per-limb cases start at class 3) runs here on the largest primes of the class -- the least
headroom under (K + 2) q < 2^32 -- and, in the tunnels, on the smallest ones too (R mod q is largest there, and with it the
carried sum), with digit counts D on both sides of K and beyond 2K, on words from {0, 1, q-2, q-1, (q-1)/2,
(q+1)/2} and on the worst case: a ciphertext whose every TrivGad digit is the constant -1 against hint slots that hold q-1, so that
every product the kernel sums is (q-1)^2.  The oracle confirms that construction before the device runs.  The inequality is
sufficient, not tight (a group of K + 1 still stays below q 2^32 at every modulus), so these cases show a group size
that is too large by two or more and any fault in the carry or in the ragged last group; that K is the documented one is the host
harness's check.

General-index passes (dense_row): four or six products per reduction in one of three variants, chosen per ring from the constants
2^32 / 6 = 715 827 882 and 2^32 / sqrt(6) = 1 753 413 056.  Two-limb rings from the primes next to either constant, one ring with a
limb on each side of the first, and the largest primes below 2^31 run every Tensor method and the key switch on extreme words.  A
wrong dispatch constant would rarely show in these cases: whether six products of such words overflow depends on the twiddles too.
tests/test_lazy_sums_host.py is what pins the two bounds, on the kernels' own expressions against 128-bit arithmetic; the cases here
pin that both sides of each constant run on the device and agree with the oracle.

Every comparison is bit for bit against the C restatement (helpers.oracle_tunnel, cref.GenRing) or the by-definition model; every
result passes assert_reduced; every ring asserts 4-byte words.  tests/test_lazy_sums_host.py checks that every modulus used here
sits within 2^18 of its threshold, in the intended class."""
import math

import numpy as np
import pytest

from helpers import (assert_reduced, dense_level, extreme_words, group_class_primes, lazy_group, level_edge_primes, oracle_tunnel,
                     primes_1_mod, primes_below, tunnel_worst_operands)

pytestmark = pytest.mark.gpu

U32 = (1 << 32) - 1
CLASSES = list(range(3, 12))                                     # kmax; K = 0, 2, 3, 4, 5, 6, 7, 8, 8
CLASS_K = {2: 0, 3: 0, 4: 2, 5: 3, 6: 4, 7: 5, 8: 6, 9: 7, 10: 8, 11: 8}
# kmax = 2 (K = 0): every prime from 1 431 655 766 up to 2^31, the reference's own moduli (1 543 651 201 ...) among them; 2q < 2^32 has
# the least room at its top.  Run by the two tunnel engines and evalLin; the Tensor methods and the key switch run these primes as
# LEVEL_RINGS["top_of_0"] below and in tests/test_gpu_word32_edges.py.
TUNNEL_CLASSES = [2] + CLASSES


def class_ring(m, kmax, L, end="top"):
    """The L largest primes = 1 (mod m) of the class, the top of the class first; end = "bottom": the L smallest, the bottom first."""
    qs = primes_below(m, L, U32 // kmax + 1) if end == "top" else primes_1_mod(m, L, U32 // (kmax + 1))
    assert qs[0] == group_class_primes(m, kmax)[end == "bottom"]
    assert all(U32 // q == kmax and lazy_group(q) == CLASS_K[kmax] for q in qs), (m, kmax, qs)
    return qs


def _minus_one(qs):
    return [q - 1 for q in qs]


# ---- tunnels between two-power rings: k_tun2_mac<u32> --------------------------------------------------------------------------------
TP_PAIRS = {1: (64, 128), 2: (128, 64), 8: (512, 64)}             # d_rel -> (r', s')
# kmax -> (d_rel, L) with D = d_rel L: K - 1 (K >= 3), K, K + 1 and a value >= 2K that is no multiple of K; two values for K = 0.
# K = 8: a ring has at most 8 limbs and d_rel is 1, 2 or 8, so D = 9 and a non-multiple of 8 above 16 do not exist with TrivGad:
# 10 and 16 stand in (16: a full group behind a carry), the BaseBGad 2 case below has D = 29 = 3 * 8 + 5, and the general-index
# tunnels run D = 9 and 18.
TP_TRIV = {2: [(1, 2), (2, 2)],
           3: [(1, 2), (2, 2)],
           4: [(1, 2), (1, 3), (1, 5)],
           5: [(1, 2), (1, 3), (2, 2), (1, 7)],
           6: [(1, 3), (2, 2), (1, 5), (2, 5)],
           7: [(2, 2), (1, 5), (2, 3), (2, 6)],
           8: [(1, 5), (2, 3), (1, 7), (2, 7)],
           9: [(2, 3), (1, 7), (8, 1), (8, 2)],
           10: [(1, 7), (8, 1), (2, 5), (8, 2)],
           11: [(1, 7), (8, 1), (2, 5), (8, 2)]}
TP_CASES = [(kmax, d, L) for kmax in TUNNEL_CLASSES for d, L in TP_TRIV[kmax]]
TP_MODULI = (128, 512)                                           # max(r', s') of the pairs


def test_the_two_power_digit_counts_cover_each_group_size():
    for kmax in TUNNEL_CLASSES:
        K, Ds = CLASS_K[kmax], [d * L for d, L in TP_TRIV[kmax]]
        if K == 0:
            assert len(set(Ds)) == 2
            continue
        want = {K, K + 1} | ({K - 1} if K >= 3 else set())
        if K == 8:
            want = {7, 8, 10, 16}
        assert want <= set(Ds), (kmax, Ds)
        assert any(D >= 2 * K and (D % K or K == 8) for D in Ds), (kmax, Ds)
    assert {d for _, d, _ in TP_CASES} == {1, 2, 8}


@pytest.mark.parametrize("minus_one", [False, True], ids=["s_default", "s_minus_one"])
@pytest.mark.parametrize("end", ["top", "bottom"])
@pytest.mark.parametrize("kmax,d_rel,L", TP_CASES, ids=[f"kmax{k}-D{d * L}-d{d}" for k, d, L in TP_CASES])
def test_tunnel_twopower_trivgad_at_the_ends_of_each_class(oracle_lib, kmax, d_rel, L, end, minus_one):
    """TrivGad: D = d_rel L products per slot.  Ciphertexts 0 and 2 reach the bound (every product (q-1)^2 in the lower half of the
    slots, D of them on top of evalLin's constant term), 1 is extreme words throughout.  Top of the class: the largest q that gets
    K products; bottom: R mod q is within 2^18 of q there, so the carried sum t (R mod q) is as large as it gets."""
    from test_gpu_tunnel_twopower import check_parity, need_twopower_tunnels
    need_twopower_tunnels()
    rp, sp = TP_PAIRS[d_rel]
    qs = class_ring(max(rp, sp), kmax, L, end)
    check_parity(oracle_lib, rp, sp, qs, "triv", 3, False, (0,), seed=kmax, word_bytes=4, s_pre=_minus_one(qs) if minus_one else None,
                 operands=tunnel_worst_operands(oracle_lib, rp, sp, qs, 3, plus=minus_one, check_digits=True))


@pytest.mark.parametrize("end", ["top", "bottom"])
@pytest.mark.parametrize("kmax", CLASSES)
def test_tunnel_twopower_base2_runs_many_groups(oracle_lib, kmax, end):
    """BaseBGad 2 at L = 1: D = d_rel ceil(log2 q) = 29 .. 31 digits (twice that for kmax 6 and 9, which run d_rel = 2), three or more
    groups with a ragged last one.  The digits of the constant -1 are 0 / -1 (only the lowest one is set), so this gadget does not
    reach the bound; the hint rows are extreme and q-1 all the same."""
    from alchemy_amd import capi
    from test_gpu_tunnel_twopower import check_parity, need_twopower_tunnels
    need_twopower_tunnels()
    rp, sp = TP_PAIRS[2 if kmax in (6, 9) else 1]
    qs = class_ring(max(rp, sp), kmax, 1, end)
    check_parity(oracle_lib, rp, sp, qs, "base2", 2, False, (0, capi.ALCH_POW_IN | capi.ALCH_POW_OUT), seed=kmax, word_bytes=4,
                 operands=tunnel_worst_operands(oracle_lib, rp, sp, qs, 2, plus=False, check_digits=False))


MIXED_CLASSES = (3, 4, 10)


@pytest.mark.parametrize("gadget", ["triv", "base2"])
@pytest.mark.parametrize("rp,sp", [(128, 64), (512, 64)])
def test_tunnel_twopower_group_size_is_per_limb(oracle_lib, rp, sp, gadget):
    """One ring with a K = 0, a K = 2 and a K = 8 limb (D = 6 and 24 with TrivGad): every limb takes its own path."""
    from test_gpu_tunnel_twopower import check_parity, need_twopower_tunnels
    need_twopower_tunnels()
    for end, minus_one in ((0, False), (0, True), (1, True)):
        qs = [group_class_primes(max(rp, sp), kmax)[end] for kmax in MIXED_CLASSES]
        assert [lazy_group(q) for q in qs] == [0, 2, 8]
        check_parity(oracle_lib, rp, sp, qs, gadget, 3, False, (0,), seed=77, word_bytes=4, s_pre=_minus_one(qs) if minus_one else None,
                     operands=tunnel_worst_operands(oracle_lib, rp, sp, qs, 3, plus=minus_one, check_digits=gadget == "triv"))


# ---- general-index tunnels: k_tunnel_mac_e and the composed path -------------------------------------------------------------------
GEN_PAIRS = {2: (40, 60), 3: (63, 105)}                           # d_rel -> (r', s'); moduli = 1 mod lcm = 120, 315
# kmax -> (d_rel, L), D = d_rel L: the values next to K that 2 L and 3 L reach, and one >= 2K that is no multiple of K
GEN_TRIV = {2: [(2, 1), (3, 1)],
            3: [(2, 1), (3, 1)],
            4: [(2, 1), (3, 1), (3, 3)],
            5: [(2, 2), (2, 4)],
            6: [(2, 2), (3, 3)],
            7: [(3, 2), (2, 6)],
            8: [(3, 2), (3, 5)],
            9: [(2, 4), (3, 5)],
            10: [(2, 4), (3, 3), (3, 6)],
            11: [(3, 3), (3, 6)]}
GEN_CASES = [(kmax, d, L) for kmax in TUNNEL_CLASSES for d, L in GEN_TRIV[kmax]]
GEN_MODULI = (120, 315)
# (tunnel_ep, tunnel_fused, tunnel_mac) of tests/test_gpu_tunnel.py::test_tunnel_hop_matches_the_oracle
OPTION_SETS = ((1, 2, 1), (1, 4, 1), (1, 0, 1), (1, 0, 0), (0, 2, 1))


def _gen_tunnel_case(oracle_lib, rp, sp, qs, option_sets, minus_one, seed):
    import alchemy_amd as A
    L, batch = len(qs), 3
    gr, gs = A.Ring(rp, qs), A.Ring(sp, qs)
    assert gr.word_bytes == gs.word_bytes == 4
    ep, d_rel = A.Tunnel.info(gr, gs)
    assert ep == math.gcd(rp, sp)
    D = d_rel * L
    rng = np.random.default_rng(8000 + 16 * seed + minus_one)
    s_pre = _minus_one(qs) if minus_one else None
    lin, ks, cts = tunnel_worst_operands(oracle_lib, rp, sp, qs, batch, plus=minus_one, check_digits=True)(rng, d_rel, L, gr.n, gs.n)
    assert ks.shape[0] == 2 * D                                   # D products per slot and component
    want = [oracle_tunnel(oracle_lib, rp, sp, qs, list(lin), list(ks), cts[2 * ct], cts[2 * ct + 1], s_pre) for ct in range(batch)]
    gin, gout = gr.upload(cts), gs.alloc(2 * batch)
    for opts in option_sets:
        if opts is not None:
            for name, v in zip(("tunnel_ep", "tunnel_fused", "tunnel_mac"), opts):
                gs.set_option(name, v)
        tun = A.Tunnel(gr, gs, gs.upload(lin), gs.upload(ks))
        gout.fill_uniform(99)
        tun.apply(gin, gout, batch, s_pre=s_pre)
        got = gout.download()
        assert_reduced(got, qs)
        for ct in range(batch):
            assert np.array_equal(got[2 * ct], want[ct][0]) and np.array_equal(got[2 * ct + 1], want[ct][1]), (ct, opts)
        assert np.array_equal(gin.download(), cts)
        del tun


def test_the_general_digit_counts_cover_each_group_size():
    for kmax in TUNNEL_CLASSES:
        K, Ds = CLASS_K[kmax], [d * L for d, L in GEN_TRIV[kmax]]
        if K == 0:
            assert len(set(Ds)) == 2
            continue
        assert any(abs(D - K) <= 1 for D in Ds) and any(D >= 2 * K and D % K for D in Ds), (kmax, Ds)
    assert {9, 18} <= {d * L for d, L in GEN_TRIV[10]}             # K = 8: the two counts the two-power pairs cannot form


@pytest.mark.parametrize("minus_one", [False, True], ids=["s_default", "s_minus_one"])
@pytest.mark.parametrize("end", ["top", "bottom"])
@pytest.mark.parametrize("kmax,d_rel,L", GEN_CASES, ids=[f"kmax{k}-D{d * L}-d{d}" for k, d, L in GEN_CASES])
def test_tunnel_general_index_at_the_ends_of_each_class(oracle_lib, kmax, d_rel, L, end, minus_one):
    """The worst case of the two-power tunnels on (40 -> 60) and (63 -> 105).  K = 2 and K = 8 run every option set (embedded
    transforms or not, fused digit transforms or through memory, lazy groups or one product at a time).  The rest run the defaults
    (digits through memory, k_tunnel_mac_e reading E'-level digits through the slot table where the table is piece-aligned) and
    the set that transforms the digits in S' itself, where k_tunnel_mac_e runs whatever the table looks like."""
    rp, sp = GEN_PAIRS[d_rel]
    qs = class_ring(rp * sp // math.gcd(rp, sp), kmax, L, end)
    option_sets = OPTION_SETS if kmax in (4, 10) else (None, (0, 2, 1))
    _gen_tunnel_case(oracle_lib, rp, sp, qs, option_sets, minus_one, kmax * 8 + d_rel * L + 500 * (end == "bottom"))


def test_tunnel_general_index_at_the_top_of_level_1(oracle_lib):
    """(63 -> 105) on the two largest primes below 2^32 / sqrt(6): the transforms around the inner product run dense_row level 1 at
    its largest moduli (K = 0 there: one product at a time in the inner product itself)."""
    qs = level_edge_primes(315)["below1"]
    assert dense_level(qs) == 1 and all(lazy_group(q) == 0 for q in qs)
    _gen_tunnel_case(oracle_lib, 63, 105, qs, (None,), True, 999)


# ---- plaintext: k_pt_mac<u32> --------------------------------------------------------------------------------------------------------
PT_LIN_CASES = [(128, 8, 4), (28, 12, 8), (32, 128, 2)]            # d_rel = 16, 6, 1
PT_MODULI = (8, 12, 128)


@pytest.mark.parametrize("r,s,p", PT_LIN_CASES)
@pytest.mark.parametrize("kmax", TUNNEL_CLASSES)
def test_pt_eval_lin_at_the_top_of_each_class(r, s, p, kmax):
    """evalLin through a lifting ring on the two largest primes of the class: d_rel = 16 products per slot walk two or more groups
    at every K, d_rel = 6 sits at K - 1 .. K + 4."""
    import alchemy_amd as A
    import test_gpu_plaintext as TP
    assert (r, s, p) in TP.LIN_CASES
    ys, xs, want = TP.lin_case(r, s, p)
    batch = len(xs)
    lift = TP.lift_ring(s, f"class{kmax}") if kmax >= 3 else A.Ring(s, class_ring(s, kmax, 2))      # lift_ring builds classes 3 .. 11
    rr, rs = TP.zp(r, p), TP.zp(s, p)
    assert lift.word_bytes == 4 and all(lazy_group(q) == CLASS_K[kmax] for q in lift.qs)
    f = A.pt_linear(lift, TP.up(rs, ys), r)
    src, dst = TP.up(rr, xs), rs.alloc(batch)
    A.pt_eval_lin(f, src, dst, batch)
    got = dst.download()
    assert_reduced(got, [p])
    assert got[:, :, 0].tolist() == want
    assert TP.down(src) == xs


# ---- general-index passes: dense_row at both of its constants ----------------------------------------------------------------------
LEVEL_M = (7, 13, 91, 169, 637, 1820)                            # one CRT_p pass (7, 13); DFT_13 / DFT_7 passes with twiddles; 4 * 5 * 7 * 13
# name -> (moduli from level_edge_primes, the level the ring must run)
LEVEL_RINGS = {"top_of_2": (lambda e: e["below2"], 2),
               "bottom_of_1": (lambda e: e["above2"], 1),
               "straddle_2_1": (lambda e: [e["below2"][0], e["above2"][0]], 1),
               "top_of_1": (lambda e: e["below1"], 1),
               "bottom_of_0": (lambda e: e["above1"], 0),
               "top_of_0": (lambda e: e["top"], 0)}


def level_ring(m, name):
    make, level = LEVEL_RINGS[name]
    qs = make(level_edge_primes(m))
    assert len(qs) == 2 and dense_level(qs) == level and max(qs) < (1 << 31)
    return qs


def _level_cases():
    return [(m, name) for m in LEVEL_M for name in LEVEL_RINGS]


def _gen(oracle_lib, m, qs):
    import alchemy_amd as A
    g, o = A.Ring(m, qs), oracle_lib.GenRing(m, qs)
    assert g.word_bytes == 4 and g.n == o.n and g.n <= 576
    return g, o


@pytest.mark.parametrize("m,name", _level_cases(), ids=[f"m{m}-{name}" for m, name in _level_cases()])
def test_general_index_tensor_methods_at_the_level_edges(oracle_lib, m, name):
    """The checks of tests/test_gpu_word64_edges.py::test_general_index_tensor_methods on 4-byte words: crt, crtInv on extreme
    CRT-basis input, the product of two transforms, mulG / divG in the three bases, l / lInv.  m = 7 and m = 13 (one CRT_p pass: the
    inputs feed the dense rows directly) also transform the input that makes every u_j = x_j + x_{p-j} and every v_j = x_j - x_{p-j}
    of the pass equal to q-1, and its mirror image."""
    from alchemy_amd import capi
    qs = level_ring(m, name)
    g, o = _gen(oracle_lib, m, qs)
    rng = np.random.default_rng(8100 + m)
    x = extreme_words(rng, 3, g.n, qs)

    def same(buf, want):
        got = buf.download()
        assert_reduced(got, qs)
        assert np.array_equal(got, np.stack(want))

    for meth in ("crt", "crtinv", "l", "linv", "mulg_pow", "mulg_dec", "mulg_crt", "divg_crt"):
        got = getattr(g, meth)(x[0])
        assert_reduced(got, qs)
        assert np.array_equal(got, getattr(o, meth)(x[0])), meth
    for meth in ("divg_pow", "divg_dec"):
        want, got = getattr(o, meth)(x[0]), getattr(g, meth)(x[0])
        assert want is not None and got is not None, meth          # g is a unit modulo these primes
        assert_reduced(got, qs)
        assert np.array_equal(got, want), meth
    buf = g.upload(x)
    buf.crt()
    crt = [o.crt(e) for e in x]
    same(buf, crt)
    prod = g.alloc(1)
    prod.mul(buf.view(0, 1), buf.view(1, 1), 1)
    same(prod, [o.mul(crt[0], crt[1])])
    buf.mulg(capi.ALCH_BASIS_CRT, 1, 2)
    same(buf, [crt[0], o.mulg_crt(crt[1]), o.mulg_crt(crt[2])])
    assert buf.divg(capi.ALCH_BASIS_CRT, 1, 2)
    same(buf, crt)
    buf.crtinv()
    same(buf, x)
    buf.mulg(capi.ALCH_BASIS_POW, 0, 2)
    same(buf, [o.mulg_pow(x[0]), o.mulg_pow(x[1]), x[2]])
    assert buf.divg(capi.ALCH_BASIS_POW, 0, 2)
    same(buf, x)
    buf.linv(0, 2)
    same(buf, [o.linv(x[0]), o.linv(x[1]), x[2]])
    buf.mulg(capi.ALCH_BASIS_DEC, 0, 1)
    same(buf, [o.mulg_dec(o.linv(x[0])), o.linv(x[1]), x[2]])
    assert buf.divg(capi.ALCH_BASIS_DEC, 0, 1)
    buf.l(0, 2)
    same(buf, x)
    if m in (7, 13):
        h, qv = (m - 1) // 2, np.array(qs, dtype=np.int64)
        lo = np.zeros((g.n, 2), dtype=np.int64)
        lo[:h + 1, :] = qv - 1                                    # x_0 .. x_h = q-1, x_j = 0 above: u_j = v_j = q-1
        hi = np.zeros((g.n, 2), dtype=np.int64)
        hi[0, :] = qv - 1
        hi[h + 1:, :] = qv - 1                                    # the mirror image: u_j = q-1, v_j = 1 (x_{p-1} = 0 by definition)
        for e in (lo, hi):
            for meth in ("crt", "crtinv"):
                got = getattr(g, meth)(e)
                assert_reduced(got, qs)
                assert np.array_equal(got, getattr(o, meth)(e)), meth


@pytest.mark.parametrize("minus_one", [False, True], ids=["s_default", "s_minus_one"])
@pytest.mark.parametrize("m,name", _level_cases(), ids=[f"m{m}-{name}" for m, name in _level_cases()])
def test_general_index_ct_mul_relin_at_the_level_edges(oracle_lib, m, name, minus_one):
    """k_gen_tensor_inv and k_gen_ks on 4-byte words, extreme operands and hint, s_pre in {none, -1}."""
    qs = level_ring(m, name)
    g, o = _gen(oracle_lib, m, qs)
    L, batch = len(qs), 3
    rng = np.random.default_rng(8200 + m + minus_one)
    hint, a, b = extreme_words(rng, 2 * L, g.n, qs), extreme_words(rng, 2 * batch, g.n, qs), extreme_words(rng, 2 * batch, g.n, qs)
    s_pre = _minus_one(qs) if minus_one else None
    gout = g.alloc(2 * batch)
    g.ct_mul_relin(g.hint_load(hint), g.upload(a), g.upload(b), gout, batch, s_pre=s_pre)
    got = gout.download()
    assert_reduced(got, qs)
    for ct in range(batch):
        w0, w1 = o.ct_mul_relin(list(hint), a[2 * ct], a[2 * ct + 1], b[2 * ct], b[2 * ct + 1], s_pre)
        assert np.array_equal(got[2 * ct], w0) and np.array_equal(got[2 * ct + 1], w1), ct
