"""GPU: tunnels between general-index rings (alch_tunnel_create / alch_ct_tunnel: do_tunnel in alchemy_amd/csrc/alchemy_hip.hip, the
tables of gen_host.hpp::gen_tunnel_table, k_gen_tunnel_ks in kernel_gen.hpp) at every SHAPE OF THE INDEX PAIR, on 4-byte and on 8-byte
words, bit for bit against the C restatement's composition (helpers.oracle_tunnel, pinned to the by-definition model at the small
pairs of this very table in tests/test_oracle_tunnel_structure.py).  With e' = gcd(r', s') the code chooses its form by the pair,
not by the modulus; ROWS names the shapes and, for every pair, the property it was chosen for.  A form that is not eligible falls
back silently and this file cannot see which kernel ran, so tests/test_tunnel_table_host.py asserts those properties (without a
device) on what alch_tunnel_create and do_tunnel decide from the tables gen_tunnel_table really builds.

  e' = 1               no E' ring is possible (phi(e') = 1): everything is transformed in S'
  e' = s'              no E' ring; phi(s') % 4 = 2 (the one-word kernels) and 0; d_rel = 11
  e' = r' (d_rel = 1)  coeffs is the identity; both dimensions % 4 = 2, the fused form, pieces_ok = 0
  E' ring dropped      phi(e') % 4 != 0 while phi(s') % 4 = 0; e' a two-power >= 32 between composite rings
  pieces_ok = 0        E' ring, k_tunnel_lin + k_hint_mac_v's per-thread piece test; with dec_c0; d_rel 3; the prime 11
  pieces_ok = 1        the smallest fused pairs (NG 4 / NP 3); d_rel 5; dec_c0 on and off; the prime 11
  fused sizes          every change of NP (phi(s') = 6144 | 6240, 10240 | 10368) and of NG (phi(e') = 4096 | 4116), NP 6 at the fused
                       bound phi(s') = 12288 with both NG, and the first size past it (k_tunnel_mac_e through the slot table)

`fused` of do_tunnel also asks for 2 phi(e') 4 <= 65536.  Since e' is a proper divisor of s' there and phi(e') % 4 = 0 = phi(s') % 4,
phi(e') <= phi(s') / 2 <= 6144 wherever phi(s') <= 12288: that condition can never be the binding one, and no row tries to reach it.

The numbered tests are the battery of the pairs.  Everything stored is asserted reduced, every ring asserts its word size, and the
input buffer is compared with what was uploaded after every call."""
import math

import numpy as np
import pytest

import alchemy_amd as A
from alchemy_amd import capi
from helpers import (assert_reduced, extreme_words, oracle_tunnel, primes_1_mod, primes_below, resident_edge_rings, tunnel_worst_operands)

pytestmark = pytest.mark.gpu

# Property words (checked by tests/test_tunnel_table_host.py; 4-byte words, default options):
#   e:N        e' = N                              e=s / e=r   e' = s' / e' = r'
#   drel:N     d_rel = N                           phis:N / phie:N / phir:N   phi(s') / phi(e') / phi(r') = N
#   phis%4:K   phi(s') % 4 = K                     phie%4:K    phi(e') % 4 = K
#   ering / noering   alch_tunnel_create gives E' a ring of its own / does not
#   e2pow      e' is a two-power >= 32 (no general-index ring)
#   pieces:B   pieces_ok                           dec:B       dec_c0 (an lInv on c0 runs inside the call)
#   fused:G/P  the fused kernel is eligible, NG = G under tunnel_fused = 4, NP = P;  nofused: it is not
#   p11        11 divides r' s'
ROWS = {
    "e_is_1": {(3, 5): "e:1 noering drel:2 phie:1 dec:1", (4, 5): "e:1 noering drel:2 phie:1 dec:0"},
    "e_is_s": {(27, 9): "e=s noering phis%4:2 drel:3", (49, 7): "e=s noering phis%4:2 drel:7", (121, 11): "e=s noering phis%4:2 drel:11 p11",
               (15, 5): "e=s noering phis%4:0 dec:1", (63, 21): "e=s noering phis%4:0 drel:3"},
    "e_is_r": {(9, 27): "e=r drel:1 noering phis%4:2 phie%4:2", (5, 15): "e=r drel:1 ering pieces:1 fused:4/3",
               (8, 16): "e=r drel:1 ering pieces:0 nofused", (21, 63): "e=r drel:1 ering pieces:0 nofused"},
    "e_ring_dropped": {(8, 12): "noering phie%4:2 phis%4:0 dec:0", (12, 8): "noering phie%4:2 phis%4:0 dec:1",
                       (45, 63): "noering phie%4:2 phis%4:0 drel:4", (33, 44): "noering phie%4:2 phis%4:0 p11",
                       (121, 33): "noering phie%4:2 phis%4:0 drel:11 p11"},
    "e_two_power": {(96, 160): "e:32 e2pow noering phie%4:0 phis%4:0"},
    "pieces_0": {(16, 24): "ering pieces:0 nofused dec:0", (24, 16): "ering pieces:0 nofused dec:1", (36, 60): "ering pieces:0 nofused drel:3",
                 (88, 132): "ering pieces:0 nofused p11"},
    "pieces_1": {(25, 15): "ering pieces:1 fused:4/3 drel:5 phie:4", (15, 20): "ering pieces:1 fused:4/3 dec:1",
                 (99, 132): "ering pieces:1 fused:4/3 p11 dec:0", (165, 132): "ering pieces:1 fused:4/3 p11 dec:1"},
}
LARGE_ROWS = {
    "np3_np5": {(35, 23040): "fused:4/3 phis:6144 drel:6", (1183, 9295): "fused:4/5 phis:6240 drel:6"},
    "np5_last": {(175, 25600): "fused:4/5 phis:10240 phie:20", (38400, 25600): "fused:2/5 phis:10240 phie:5120"},
    "np6_first": {(35, 38880): "fused:4/6 phis:10368"},
    "np6_bound": {(35, 46080): "fused:4/6 phis:12288", (39936, 26624): "fused:2/6 phis:12288 phie:6144"},
    "past_fused": {(676, 27885): "nofused ering pieces:1 phis:12480"},
    "ng_edge": {(30720, 20480): "fused:4/5 phie:4096", (36015, 28812): "fused:2/5 phie:4116 drel:4"},
}
SMALL = [p for row in ROWS.values() for p in row]
LARGE = [p for row in LARGE_ROWS.values() for p in row]
REFUSED = [(64, 192), (192, 64)]                  # a two-power ring >= 32 against a general-index one

# (tunnel_ep, tunnel_fused, tunnel_mac) of tests/test_gpu_tunnel.py::test_tunnel_hop_matches_the_oracle
OPTION_SETS = ((1, 2, 1), (1, 4, 1), (1, 0, 1), (1, 0, 0), (0, 2, 1))
LARGE_OPTION_SETS = ((1, 2, 1), (1, 4, 1), (1, 0, 1))
DEFAULTS = (1, 0, 1)
BOTH = capi.ALCH_POW_IN | capi.ALCH_POW_OUT


def pid(p):
    return f"{p[0]}to{p[1]}"


def lcm(p):
    return p[0] * p[1] // math.gcd(*p)


def rand_elems(rng, count, n, qs):
    return np.stack([np.stack([rng.integers(0, q, size=n, dtype=np.int64) for q in qs], axis=1) for _ in range(count)])


def up_switched(oracle_lib, rp, cts, qs, dup):
    """modSwitch up by the first `dup` limbs of qs, in the CRT basis: x -> (0, q_a x)."""
    mult = math.prod(qs[:dup])
    Oin = oracle_lib.GenRing(rp, qs[dup:])
    out = []
    for c in cts:
        scaled = Oin.scale(np.ascontiguousarray(c), [mult % q for q in qs[dup:]])
        out.append(np.ascontiguousarray(np.concatenate([np.zeros((c.shape[0], dup), dtype=np.int64), scaled], axis=1)))
    return out


def check(oracle_lib, pair, qs, batch, word, gadget="triv", flags=0, option_sets=(DEFAULTS,), s_pre="random", dup=0, operands=None, seed=0,
          scratch_mib=None, per_ct=None):
    """One draw of operands, one oracle run, every option set of `option_sets` against it.  dup: the input lives on the last L - dup limbs.
    scratch_mib: the chunked call must equal the oracle AND the unchunked call; per_ct(gs, d_rel, D) -> bytes of scratch per ciphertext."""
    rp, sp = pair
    L = len(qs)
    gr, gs = A.Ring(rp, qs), A.Ring(sp, qs)
    gin_ring = A.Ring(rp, qs[dup:]) if dup else gr
    assert gr.word_bytes == gs.word_bytes == word and (not dup or gin_ring.word_bytes in (4, word))
    ep, d_rel = A.Tunnel.info(gr, gs)
    Or, Os, Oin = oracle_lib.GenRing(rp, qs), oracle_lib.GenRing(sp, qs), oracle_lib.GenRing(rp, qs[dup:])
    assert ep == math.gcd(rp, sp) and d_rel * oracle_lib.GenRing(ep, qs).n == Or.n == gr.n and Os.n == gs.n
    gad = capi.ALCH_GAD_BASE2 if gadget == "base2" else capi.ALCH_GAD_TRIV
    D = gs.gadget_digits(capi.ALCH_GAD_BASE2) if gadget == "base2" else L
    assert gadget == "triv" or D == sum((q - 1).bit_length() for q in qs)
    rng = np.random.default_rng(1000 * rp + sp + seed)
    if operands is not None:
        assert not dup
        lin, ks, cts = operands(rng, d_rel, D, gr.n, gs.n)
    else:
        lin, ks, cts = rand_elems(rng, d_rel, gs.n, qs), rand_elems(rng, 2 * d_rel * D, gs.n, qs), rand_elems(rng, 2 * batch, gr.n, qs[dup:])
    if isinstance(s_pre, str):
        s_pre = [int(rng.integers(1, q)) for q in qs]
    # the oracle takes CRT-basis ciphertexts on all L limbs
    crt_in = [Oin.crt(np.ascontiguousarray(c)) for c in cts] if flags & capi.ALCH_POW_IN else list(cts)
    if dup:
        crt_in = up_switched(oracle_lib, rp, crt_in, qs, dup)
    want = [oracle_tunnel(oracle_lib, rp, sp, qs, list(lin), list(ks), crt_in[2 * ct], crt_in[2 * ct + 1], s_pre,
                          pow_out=bool(flags & capi.ALCH_POW_OUT), gadget=gadget) for ct in range(batch)]
    gin, gout = gin_ring.upload(cts), gs.alloc(2 * batch)
    if dup:                                                       # the device's own modSwitch up gives the oracle's input
        assert not flags & capi.ALCH_POW_IN
        gup = gr.alloc(2 * batch)
        capi.ct_mod_switch(gin, gup, batch)
        assert np.array_equal(gup.download(), np.stack(crt_in))
    for opts in option_sets:
        for name, v in zip(("tunnel_ep", "tunnel_fused", "tunnel_mac"), opts):
            gs.set_option(name, v)
        tun = A.Tunnel(gr, gs, gs.upload(lin), gs.upload(ks), gadget=gad)
        runs = [None]
        if scratch_mib is not None:
            bytes_ct = per_ct(gs, d_rel, D, opts)
            chunk = (scratch_mib << 20) // bytes_ct
            assert chunk >= 1 and batch // chunk >= 2 and batch % chunk != 0, (bytes_ct, chunk, batch)
            runs = [None, scratch_mib]
        got_runs = []
        for mib in runs:
            gs.set_option("scratch_mib", 4096 if mib is None else mib)
            gout.fill_uniform(99)
            tun.apply(gin, gout, batch, s_pre=s_pre, flags=flags)
            got = gout.download()
            assert_reduced(got, qs)
            for ct in range(batch):
                assert np.array_equal(got[2 * ct], want[ct][0]) and np.array_equal(got[2 * ct + 1], want[ct][1]), (pair, ct, opts, mib)
            assert np.array_equal(gin.download(), cts), (pair, opts, mib)            # input untouched
            got_runs.append(got)
        assert all(np.array_equal(g, got_runs[0]) for g in got_runs)
        del tun


def gpu_moduli(pair, L, which):
    return primes_below(lcm(pair), L, 1 << 31) if which == "top31" else primes_1_mod(lcm(pair), L, 1 << 28)


# ---- 1. TrivGad, CRT in and out, random s_pre ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["top31", "lazy8"])
@pytest.mark.parametrize("pair", SMALL, ids=pid)
def test_1_trivgad_small_pairs_every_option_set(oracle_lib, pair, which):
    """Batch 5: one full tile of four ciphertexts and a tail.  L = 3: d_rel L is odd wherever d_rel is, so the last round of NG = 2 and
    of NG = 4 is partial.  Moduli: the largest below 2^31 (one product at a time) and the first above 2^28 (lazy groups of 8)."""
    check(oracle_lib, pair, gpu_moduli(pair, 3, which), 5, 4, option_sets=OPTION_SETS)


@pytest.mark.parametrize("pair", LARGE, ids=pid)
def test_1_trivgad_large_pairs_fused_and_composed(oracle_lib, pair):
    """L = 2, batch 2, the largest moduli below 2^31; tunnel_fused = 2, 4 and 0."""
    check(oracle_lib, pair, gpu_moduli(pair, 2, "top31"), 2, 4, option_sets=LARGE_OPTION_SETS)


# ---- 2. Pow-basis input ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [BOTH, capi.ALCH_POW_IN], ids=["pow_in_out", "pow_in"])
@pytest.mark.parametrize("pair", SMALL + LARGE, ids=pid)
def test_2_pow_basis_input_is_read_in_place(oracle_lib, pair, flags):
    """ALCH_POW_IN: c1 is read where it lies and, with dec_c0, c0 is lInv'ed out of place into the scratch; the input stays untouched.
    Batch 3 (2 on the large pairs); default options and the fused form."""
    large = pair in LARGE
    check(oracle_lib, pair, gpu_moduli(pair, 2 if large else 3, "top31"), 2 if large else 3, 4, flags=flags, option_sets=(DEFAULTS, (1, 4, 1)))


# ---- 3. BaseBGad 2 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", SMALL, ids=pid)
def test_3_base2_hints(oracle_lib, pair):
    """BaseBGad 2 at L = 2 (62 digits per E'-coefficient), batch 2: E'-level and S'-level transforms, tunnel_mac on and off."""
    check(oracle_lib, pair, gpu_moduli(pair, 2, "top31"), 2, 4, gadget="base2", option_sets=(DEFAULTS, (1, 0, 0), (0, 0, 1)))


# ---- 4. input below the hint ring ---------------------------------------------------------------------------------------------------------
DUP_PAIRS = [(25, 15), (16, 24), (8, 12), (63, 21), (1183, 9295)]
DUP_CASES = [(p, g) for p in DUP_PAIRS for g in ("triv", "base2") if g == "triv" or p in SMALL]


@pytest.mark.parametrize("pair,gadget", DUP_CASES, ids=[f"{pid(p)}-{g}" for p, g in DUP_CASES])
def test_4_input_on_the_last_two_limbs_of_three(oracle_lib, pair, gadget):
    """dup = 1: TrivGad runs the compact layout (Lx = 2, xoff = 1), BaseBGad 2 the full one with a zero limb.  Against the oracle on the
    alch_ct_mod_switch-ed-up input, which is itself compared with x -> (0, q_a x).  The BaseBGad 2 hint of 1183 -> 9295 would be 1116
    elements of 6240 x 3 words: that pair runs TrivGad only, like every large pair."""
    check(oracle_lib, pair, gpu_moduli(pair, 3, "top31"), 2, 4, gadget=gadget, dup=1,
          option_sets=OPTION_SETS if gadget == "triv" else (DEFAULTS, (0, 0, 1)))


# ---- 5. 8-byte words ---------------------------------------------------------------------------------------------------------------------
RINGS64 = ("TOP62", "LOW64", "MIX64")


@pytest.mark.parametrize("ring", RINGS64)
@pytest.mark.parametrize("pair", SMALL, ids=pid)
def test_5_word64_trivgad(oracle_lib, pair, ring):
    """do_tunnel<u64>: k_tunnel_gather, k_tunnel_lin, k_hint_mac_e / k_hint_mac_v behind the slot table, the TrivGad digit loader.  Batch 5,
    the ring's own limbs (2, or 3 on MIX64: one limb of 17 bits among them), E'-level and S'-level transforms."""
    check(oracle_lib, pair, resident_edge_rings(lcm(pair))[ring], 5, 8, option_sets=(DEFAULTS, (0, 0, 1)))


@pytest.mark.parametrize("flags", [BOTH, capi.ALCH_POW_IN], ids=["pow_in_out", "pow_in"])
@pytest.mark.parametrize("ring", RINGS64)
@pytest.mark.parametrize("pair", SMALL, ids=pid)
def test_5_word64_pow_basis_input(oracle_lib, pair, ring, flags):
    check(oracle_lib, pair, resident_edge_rings(lcm(pair))[ring], 3, 8, flags=flags)


@pytest.mark.parametrize("pair", SMALL, ids=pid)
def test_5_word64_base2_hints(oracle_lib, pair):
    """BaseBGad 2 on the two largest primes below 2^62: 124 digits per E'-coefficient through the 8-byte digit loader."""
    check(oracle_lib, pair, resident_edge_rings(lcm(pair))["TOP62"], 2, 8, gadget="base2", option_sets=(DEFAULTS, (0, 0, 1)))


@pytest.mark.parametrize("pair", [(1183, 9295), (38400, 25600)], ids=pid)
def test_5_word64_large_pairs(oracle_lib, pair):
    check(oracle_lib, pair, resident_edge_rings(lcm(pair))["TOP62"], 2, 8, option_sets=(DEFAULTS,))


@pytest.mark.parametrize("pair", [(36, 60), (165, 132), (121, 11)], ids=pid)
def test_5_word64_extreme_words(oracle_lib, pair):
    """Ciphertexts, linear function and hints from helpers.extreme_words (0, 1, q-2, q-1, the residues next to q/2), s_pre = q - 1."""
    qs = resident_edge_rings(lcm(pair))["TOP62"]

    def operands(rng, d_rel, D, n_r, n_s):
        return extreme_words(rng, d_rel, n_s, qs), extreme_words(rng, 2 * d_rel * D, n_s, qs), extreme_words(rng, 2 * 3, n_r, qs)

    check(oracle_lib, pair, qs, 3, 8, s_pre=[q - 1 for q in qs], operands=operands, option_sets=(DEFAULTS, (0, 0, 1)))


# ---- 6. worst operands -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("minus_one", [False, True], ids=["s_default", "s_minus_one"])
@pytest.mark.parametrize("pair", [(25, 15), (36, 60), (121, 11), (35, 23040)], ids=pid)
def test_6_worst_operands_at_the_top_moduli(oracle_lib, pair, minus_one):
    """helpers.tunnel_worst_operands: every product of the inner product is (q-1)^2 in the lower half of the slots of ciphertexts 0 and
    2, extreme words elsewhere; the largest moduli below 2^31."""
    large = pair in LARGE
    qs = gpu_moduli(pair, 2 if large else 3, "top31")
    check(oracle_lib, pair, qs, 3, 4, s_pre=[q - 1 for q in qs] if minus_one else None,
          operands=tunnel_worst_operands(oracle_lib, pair[0], pair[1], qs, 3, plus=minus_one, check_digits=True),
          option_sets=LARGE_OPTION_SETS if large else OPTION_SETS)


# ---- 7. more than one chunk --------------------------------------------------------------------------------------------------------------
def scratch_per_ct(rp_n, n_x, dup=0):
    """do_tunnel: `scratch per ciphertext: Pow copy of the input (2 R'-elements), x0, x1 (D coefficients each), digits (D * GD elements of
    rx)`, D = d_rel here; the fused form keeps no digits.  rx: E' with its ring, else S'."""
    def per_ct(gs, d_rel, GD, opts):
        wb, L = gs.word_bytes, gs.L
        ebr, ebx = L * rp_n * wb, L * n_x * wb
        fused = wb == 4 and opts[1] != 0 and GD == L
        return 2 * ebr + 2 * d_rel * ebx + (0 if fused else d_rel * GD * ebx)
    return per_ct


def test_7_chunked_trivgad_at_phi_10240(oracle_lib):
    """38400 -> 25600, L = 2, batch 5, scratch_mib = 1.  Per ciphertext: 2 x 81920 (input) + 2 x 2 x 40960 (x0, x1 at phi(e') = 5120) +
    2 x 2 x 40960 (digits) = 491520 bytes on the composed path -> chunks of 2, 2, 1; with k_tunnel_mac_e and with k_tunnel_lin +
    k_hint_mac_e.  (The fused form keeps no digits: 327680 bytes, chunks of 3 and 2 -- not two full chunks, so it is not run here.)"""
    check(oracle_lib, (38400, 25600), gpu_moduli((38400, 25600), 2, "top31"), 5, 4, option_sets=((1, 0, 1), (1, 0, 0)), scratch_mib=1,
          per_ct=scratch_per_ct(10240, 5120))


def test_7_chunked_base2_in_s_prime(oracle_lib):
    """63 -> 105, BaseBGad 2, tunnel_ep = 0, L = 3, batch 9, scratch_mib = 1.  Per ciphertext: 2 x 432 (input) + 2 x 3 x 576 (x0, x1 in S') +
    3 x 93 x 576 (digits) = 165024 bytes -> chunks of 6 and 3 -- 9 ciphertexts at three 31-bit limbs cannot fill a third chunk, so this
    case asserts two chunks of different sizes instead of two full ones and a remainder."""
    pair = (63, 105)
    per = scratch_per_ct(36, 48)
    qs = gpu_moduli(pair, 3, "top31")
    assert per(type("R", (), {"word_bytes": 4, "L": 3}), 3, 93, (0, 0, 1)) == 165024 and 9 * 165024 > 1 << 20
    rp, sp = pair
    gr, gs = A.Ring(rp, qs), A.Ring(sp, qs)
    D = gs.gadget_digits(capi.ALCH_GAD_BASE2)
    assert D == 93 and gs.word_bytes == 4
    rng = np.random.default_rng(63105)
    lin, ks, cts = rand_elems(rng, 3, gs.n, qs), rand_elems(rng, 2 * 3 * D, gs.n, qs), rand_elems(rng, 2 * 9, gr.n, qs)
    s_pre = [int(rng.integers(1, q)) for q in qs]
    want = [oracle_tunnel(oracle_lib, rp, sp, qs, list(lin), list(ks), cts[2 * ct], cts[2 * ct + 1], s_pre, gadget="base2") for ct in range(9)]
    gs.set_option("tunnel_ep", 0)
    tun = A.Tunnel(gr, gs, gs.upload(lin), gs.upload(ks), gadget=capi.ALCH_GAD_BASE2)
    gin, gout = gr.upload(cts), gs.alloc(18)
    got = []
    for mib in (4096, 1):
        gs.set_option("scratch_mib", mib)
        gout.fill_uniform(99)
        tun.apply(gin, gout, 9, s_pre=s_pre)
        got.append(gout.download())
        assert_reduced(got[-1], qs)
        for ct in range(9):
            assert np.array_equal(got[-1][2 * ct], want[ct][0]) and np.array_equal(got[-1][2 * ct + 1], want[ct][1]), (ct, mib)
        assert np.array_equal(gin.download(), cts)
    assert np.array_equal(got[0], got[1])


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", REFUSED, ids=pid)
def test_8_a_two_power_ring_against_a_general_one_is_refused(pair):
    """alch_tunnel_create refuses on the host (nothing is launched).  alch_tunnel_info only does the index arithmetic for such a pair."""
    qs = primes_below(192, 2, 1 << 31)
    gr, gs = A.Ring(pair[0], qs), A.Ring(pair[1], qs)
    d_rel = 1 if pair[0] < pair[1] else 2
    assert A.Tunnel.info(gr, gs) == (64, d_rel)
    with pytest.raises(A.AlchemyError):
        A.Tunnel(gr, gs, gs.alloc(d_rel), gs.alloc(2 * d_rel * 2))
    with pytest.raises(A.AlchemyError):
        A.Tunnel(gr, gs, gs.alloc(d_rel), gs.alloc(2 * d_rel * 62), gadget=capi.ALCH_GAD_BASE2)


def test_8_rings_that_differ_in_one_modulus_are_refused():
    qs = primes_below(300, 3, 1 << 31)
    gr, gs = A.Ring(25, qs[:2]), A.Ring(15, [qs[0], qs[2]])
    assert A.Tunnel.info(gr, gs) == (5, 5)
    with pytest.raises(A.AlchemyError):
        A.Tunnel(gr, gs, gs.alloc(5), gs.alloc(2 * 5 * 2))
    gs62 = A.Ring(15, [qs[0], primes_below(75, 1, 1 << 62)[0]])        # the same limb count, another word size
    with pytest.raises(A.AlchemyError):
        A.Tunnel(gr, gs62, gs62.alloc(5), gs62.alloc(2 * 5 * 2))
