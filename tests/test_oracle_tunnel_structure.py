"""CPU: the checker of the tunnel tests (tests/helpers.py::oracle_tunnel, a composition of the C restatement's primitives) against the
by-definition model (oracle/model_gen.py::g_tunnel) on the small index pairs of tests/test_gpu_tunnel_structure.py -- e' = 1, e' = s',
e' = r', dimensions of 2 and 6, the prime 11 -- where it had only ever been compared on (40, 60)-like pairs.  Random linear function,
hints, ciphertext and encoding scalars; two moduli = 1 mod lcm(r', s'), one below and one above 2^31; both gadgets, CRT- and Pow-basis
output; bit for bit."""
import math
import random

import numpy as np
import pytest

from helpers import from_aos, oracle_tunnel, primes_1_mod, to_aos
from oracle import model_gen as G
from oracle.model import MSD

import test_gpu_tunnel_structure as TS

PAIRS = list(TS.SMALL)                          # every small pair: phi(r'), phi(s') <= 110


def test_the_pairs_cover_the_shapes():
    assert max(G.totient(m) for p in PAIRS for m in p) == 110
    gcds = {p: math.gcd(*p) for p in PAIRS}
    assert any(e == 1 for e in gcds.values()) and any(e == p[1] for p, e in gcds.items()) and any(e == p[0] for p, e in gcds.items())
    assert any((p[0] * p[1]) % 11 == 0 for p in PAIRS)
    assert {G.totient(e) % 4 for e in gcds.values()} == {0, 1, 2}


@pytest.mark.parametrize("gadget", ["triv", "base2"])
@pytest.mark.parametrize("pair", PAIRS, ids=TS.pid)
def test_the_composition_equals_the_model(oracle_lib, pair, gadget):
    rp, sp = pair
    lcm = rp * sp // math.gcd(rp, sp)
    qs = [primes_1_mod(lcm, 1, 1 << 29)[0], primes_1_mod(lcm, 1, 1 << 31)[0]]
    assert qs[0] < 1 << 31 < qs[1]
    T = G.TunnelInfo(None, None, None, G.Index(math.gcd(rp, sp)), G.Index(rp), G.Index(sp))
    d_rel = T.rp.n // T.ep.n
    D = len(qs) if gadget == "triv" else sum((q - 1).bit_length() for q in qs)
    rng = random.Random(1000 * rp + sp)
    elem = lambda n: [[rng.randrange(q) for _ in range(n)] for q in qs]              # limb-major, Pow basis
    lin_pow = [elem(T.sp.n) for _ in range(d_rel)]
    hints = [[[elem(T.sp.n), elem(T.sp.n)] for _ in range(D)] for _ in range(d_rel)]
    ct = [elem(T.rp.n), elem(T.rp.n)]
    s_pre = [rng.randrange(1, q) for q in qs]
    scaled = [[[v * s % q for v in limb] for limb, s, q in zip(c, s_pre, qs)] for c in ct]
    want = G.g_tunnel(lin_pow, hints, G.GCT(MSD, 0, 1, scaled, 4, qs, T.rp, None), T, gadget=gadget)
    Or, Os = oracle_lib.GenRing(rp, qs), oracle_lib.GenRing(sp, qs)
    lin_crt = [Os.crt(to_aos(y)) for y in lin_pow]
    ks_crt = [Os.crt(to_aos(x)) for hint_i in hints for b, a in hint_i for x in (b, a)]
    c0, c1 = Or.crt(to_aos(ct[0])), Or.crt(to_aos(ct[1]))
    p0, p1 = oracle_tunnel(oracle_lib, rp, sp, qs, lin_crt, ks_crt, c0, c1, s_pre, pow_out=True, gadget=gadget)
    assert from_aos(p0) == want.c[0] and from_aos(p1) == want.c[1]
    w0, w1 = oracle_tunnel(oracle_lib, rp, sp, qs, lin_crt, ks_crt, c0, c1, s_pre, gadget=gadget)
    assert np.array_equal(w0, Os.crt(to_aos(want.c[0]))) and np.array_equal(w1, Os.crt(to_aos(want.c[1])))
    assert int(w0.min()) >= 0 and all(int(w0[:, j].max()) < q and int(w1[:, j].max()) < q for j, q in enumerate(qs))
