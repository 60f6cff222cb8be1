"""CPU: ring tunnels between two-power cyclotomic rings -- the ground the device path for two-power rings (do_tunnel_pow2 in
alchemy_amd/csrc/alchemy_hip.hip) stands on.  The exact model builds valid instances on two-power towers and decrypts them to f(pt);
the C restatement's composition (helpers.oracle_tunnel) reproduces the model word for word; and the CLOSED-FORM index maps the device
uses instead of tables -- the stride-d_rel de-interleave for `coeffs`, position j 2^sh for embedPow, slot k >> sh for embedCRT --
equal the model's index tables and the direct evaluation of both sides."""
import random

import numpy as np
import pytest

from helpers import load_golden, oracle_tunnel, primes_1_mod, to_aos
from oracle import model_gen as G

TOWERS = [(4, 8, 32, 64), (64, 32, 64, 32), (8, 32, 32, 128), (128, 32, 128, 32)]


def _instance(r, s, rp, sp, gadget, seed):
    rng = random.Random(seed)
    p = 4
    T = G.tunnel_indices(r, s, rp, sp)
    qs = primes_1_mod(max(rp, sp), 3, 1 << 29)
    sk_in, sk_out = G.g_gen_sk(T.rp, rng), G.g_gen_sk(T.sp, rng)
    ys = [[rng.randrange(p) for _ in range(T.s.n)] for _ in range(T.r.n // T.e.n)]
    pt = [rng.randrange(p) for _ in range(T.r.n)]
    ct = G.g_to_msd(G.g_mod_switch_up(G.g_encrypt(sk_in, pt, T.r, T.rp, p, qs[1:], rng), qs[:1]))
    lin_q, hints = G.g_tunnel_hint(ys, T, p, sk_in, sk_out, qs, rng, gadget=gadget)
    tun = G.g_tunnel(lin_q, hints, ct, T, gadget=gadget)
    want = G.eval_lin_dec(ys, G.linv_def(pt, T.r, p), T.e, T.r, T.s, p)
    return T, qs, sk_out, lin_q, hints, ct, tun, want


@pytest.mark.parametrize("gadget", ["triv", "base2"])
@pytest.mark.parametrize("r,s,rp,sp", TOWERS)
def test_two_power_tunnel_decrypts_and_the_c_restatement_equals_the_model(oracle_lib, r, s, rp, sp, gadget):
    T, qs, sk_out, lin_q, hints, ct, tun, want = _instance(r, s, rp, sp, gadget, rp * 7 + sp)
    assert T.ep.m == min(rp, sp) and len(lin_q) == max(1, rp // sp)
    assert G.g_decrypt(sk_out, G.g_mod_switch_down(tun, 1)) == want                      # the model instance decrypts to f(pt)
    Or, Os = oracle_lib.GenRing(rp, qs), oracle_lib.GenRing(sp, qs)
    lin = [Os.crt(to_aos(y)) for y in lin_q]
    ks = []
    for hint_i in hints:
        for b, a in hint_i:
            ks += [Os.crt(to_aos(b)), Os.crt(to_aos(a))]
    c0, c1 = Or.crt(to_aos(ct.c[0])), Or.crt(to_aos(ct.c[1]))
    w0, w1 = oracle_tunnel(oracle_lib, rp, sp, qs, lin, ks, c0, c1, pow_out=True, gadget=gadget)
    lm = lambda a: np.asarray(a).T.tolist()
    assert lm(w0) == tun.c[0] and lm(w1) == tun.c[1]                                      # oracle_tunnel equals the model


def test_fixture_is_what_its_generator_describes(oracle_lib):
    """tests/golden/tunnel_twopower_small.json: the C restatement's composition reproduces every record, and the recorded output
    decrypts to the recorded f(pt)."""
    lm = lambda a: np.asarray(a).T.tolist()
    recs = load_golden("tunnel_twopower_small.json")
    assert len(recs) == 4
    for rec in recs:
        qs = rec["qs"]
        assert len(qs) == 3
        Or, Os = oracle_lib.GenRing(rec["rp"], qs), oracle_lib.GenRing(rec["sp"], qs)
        lin = [Os.crt(to_aos(y)) for y in rec["lin"]]
        ks = []
        for hint_i in rec["hints"]:
            for b, a in hint_i:
                ks += [Os.crt(to_aos(b)), Os.crt(to_aos(a))]
        c0, c1 = Or.crt(to_aos(rec["ct_in"][0])), Or.crt(to_aos(rec["ct_in"][1]))
        w0, w1 = oracle_tunnel(oracle_lib, rec["rp"], rec["sp"], qs, lin, ks, c0, c1, pow_out=True, gadget=rec["gadget"])
        assert lm(w0) == rec["ct_out"][0] and lm(w1) == rec["ct_out"][1], (rec["rp"], rec["sp"], rec["gadget"])
        T = G.tunnel_indices(rec["r"], rec["s"], rec["rp"], rec["sp"])
        out = G.GCT(G.MSD, 0, rec["ct_out_l"], rec["ct_out"], rec["p"], qs, T.sp, T.s)
        assert G.g_decrypt(rec["sk_out"], G.g_mod_switch_down(out, 1)) == rec["f_of_pt"]


@pytest.mark.parametrize("rp,sp", [(32, 64), (64, 32), (64, 512), (512, 64), (32, 128), (128, 32), (1 << 12, 1 << 13), (1 << 14, 1 << 11)])
def test_closed_form_index_maps_equal_the_model_tables(rp, sp):
    """What k_tun2_gather computes instead of reading a table: with E' the smaller ring, d = d_rel = max(1, n_r / n_s),
    E'-coefficient i of a Pow vector over R' is entry i + d k, and embedPow E' -> S' puts coefficient j at position j 2^sh."""
    ep = min(rp, sp)
    ie, ir, isx = G.Index(ep), G.Index(rp), G.Index(sp)
    d, sh = ir.n // ie.n, (isx.n // ie.n).bit_length() - 1
    assert d == max(1, rp // sp) and isx.n == ie.n << sh
    rows = G.coeffs_indices(ie, ir)
    assert len(rows) == d
    for i, row in enumerate(rows):
        assert list(row) == [i + d * k for k in range(ie.n)]
    assert list(G.embed_indices(ie, isx)) == [j << sh for j in range(ie.n)]
    # two-power index: g = 1 and l = identity, so the tunnel has no lInv / l step
    x = list(range(1, ir.n + 1))
    assert G.linv_def(x, ir, 1 << 20) == x


@pytest.mark.parametrize("e_m,s_m", [(32, 64), (32, 128), (64, 512), (16, 32), (128, 128)])
def test_crt_of_an_embedded_element_reads_slot_k_shifted(e_m, s_m):
    """crt_S'(embedPow x)[k] = crt_E'(x)[k >> sh] by direct evaluation of both sides (the identity of
    test_crt_of_an_embedded_element_is_the_small_crt_replicated, in the closed form k_tun2_mac uses): the slot rule of a two-power
    index is bit-reversed, so the slots of S' above one slot of E' are consecutive."""
    ie, isx = G.Index(e_m), G.Index(s_m)
    sh = (isx.n // ie.n).bit_length() - 1
    q = primes_1_mod(s_m, 1, 1 << 20)[0]
    rng = random.Random(e_m * 1000 + s_m)
    x = [rng.randrange(q) for _ in range(ie.n)]
    big = G.crt_def(G.embed_pow(x, ie, isx), isx, q)
    small = G.crt_def(x, ie, q)
    assert all(big[k] == small[k >> sh] for k in range(isx.n))


@pytest.mark.parametrize("m", [32, 64, 256])
def test_general_oracle_slot_order_is_the_two_power_slot_order(oracle_lib, m):
    """GenRing(m).crt equals the two-power Ring(m / 2).crt: the slot order the general-index oracle checks the device against is the
    slot rule of include/alchemy_hip.h for a two-power index."""
    qs = primes_1_mod(m, 2, 1 << 29)
    rng = np.random.default_rng(m)
    x = np.stack([rng.integers(0, q, size=m // 2, dtype=np.int64) for q in qs], axis=1)
    assert np.array_equal(oracle_lib.GenRing(m, qs).crt(x.copy()), oracle_lib.Ring(m // 2, qs).crt(x.copy()))
