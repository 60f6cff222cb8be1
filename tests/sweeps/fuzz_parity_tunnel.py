#!/usr/bin/env python3
"""Randomised parity sweep of alch_ct_tunnel: random index pairs (r', s') over the primes 2, 3, 5, 7, 11, 13 with lcm <= 60000 and
phi <= 3000 that satisfy Lol's tunnel conditions (alch_tunnel_info decides; d_rel = 1 and e' = s' pairs included), 1..4 moduli = 1 mod
lcm(r', s') -- one case in three from the ends of the group-size classes of the lazy inner product and the level edges of dense_row
(helpers.threshold_moduli), one in four on 8-byte words (helpers.resident_edge_rings: the largest primes below 2^62, the first above
2^31, a 62-bit one next to a 17-bit one) -- TrivGad or BaseBGad 2 hints, random linear functions, hints, ciphertexts (one 32-bit TrivGad
case in four: the worst case of the inner product, helpers.tunnel_worst_operands), encoding scalars, batch 1..9, the tunnel_ep /
tunnel_fused / tunnel_mac options, scratch_mib 1 or 4096, the Pow-basis-in and -out flags, and (one case in four) an input on fewer
limbs than the tunnel's ring, against the C restatement's composition (tests/helpers.py::oracle_tunnel -- the checker of the tunnel
tests).  usage: tests/sweeps/fuzz_parity_tunnel.py [seconds] [seed]"""
import math, os, random, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import alchemy_amd as A
from alchemy_amd import capi
from oracle import cref
from helpers import assert_reduced, oracle_tunnel, primes_1_mod, resident_edge_rings, threshold_moduli, tunnel_worst_operands


def phi(m):
    r, p, t = m, 2, m
    while p * p <= t:
        if t % p == 0:
            r -= r // p
            while t % p == 0: t //= p
        p += 1
    return r - r // t if t > 1 else r


def rand_index(rng):
    m = (2 ** rng.choice([0, 0, 2, 3]) * 3 ** rng.choice([0, 1, 2]) * 5 ** rng.choice([0, 1]) * 7 ** rng.choice([0, 1]) *
         11 ** rng.choice([0, 0, 1]) * 13 ** rng.choice([0, 0, 1]))
    return m


def main():
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else int(time.time())
    rng, nprng = random.Random(seed), np.random.default_rng(seed)
    cref.build()
    t0, cases, refused, tally = time.time(), 0, 0, {}
    print(f"seed {seed}", flush=True)
    while time.time() - t0 < budget:
        rp, sp = rand_index(rng), rand_index(rng)
        if rng.random() < 0.2:                                       # d_rel = 1 / e' = s': one index divides the other
            sp = rp * rng.choice([2, 3, 4, 5, 7, 9, 11])
            if rng.random() < 0.5: rp, sp = sp, rp
        if rp == sp or min(rp, sp) < 3 or rp % 4 == 2 or sp % 4 == 2: continue
        lcm = rp * sp // math.gcd(rp, sp)
        if lcm > 60000 or max(phi(rp), phi(sp)) > 3000 or min(phi(rp), phi(sp)) < 4: continue
        if (rp & (rp - 1)) == 0 and (sp & (sp - 1)) == 0: continue
        if rng.random() < 0.25:
            qs, edges = resident_edge_rings(lcm)[rng.choice(["TOP62", "LOW64", "MIX64"])], True
        else:
            edges = rng.random() < 0.33
            qs = threshold_moduli(rng, lcm, rng.randint(1, 4)) if edges else primes_1_mod(lcm, rng.randint(1, 4), lo=rng.choice([1 << 28, 1 << 29, 1 << 30]))
        wide = max(qs) >= 1 << 31                                    # 8-byte words (a drawn prime above 2^30 may be above 2^31 too)
        L = len(qs)
        try:
            gr, gs = A.Ring(rp, qs), A.Ring(sp, qs)
            ep, d_rel = A.Tunnel.info(gr, gs)
        except capi.AlchemyError:
            refused += 1
            continue
        assert gr.word_bytes == gs.word_bytes == (8 if wide else 4)
        gadget = rng.choice(["triv", "triv", "base2"])
        D = gs.gadget_digits(capi.ALCH_GAD_BASE2) if gadget == "base2" else L
        if d_rel * D > 400 and gs.n > 500: continue                  # keep the oracle's work per case small
        batch = rng.randint(1, 9)
        if d_rel * D * batch * gs.n > 4_000_000: batch = rng.randint(1, 3)
        dup = rng.randint(1, L - 1) if L > 1 and rng.random() < 0.25 and len({q >= 1 << 31 for q in qs}) == 1 else 0
        pow_in = dup == 0 and rng.random() < 0.3
        pow_out = rng.random() < 0.3
        qin = qs[dup:]
        rnd = lambda c, n, ql: np.stack([np.stack([nprng.integers(0, q, size=n, dtype=np.int64) for q in ql], axis=1) for _ in range(c)])
        lin, ks, cts = rnd(d_rel, gs.n, qs), rnd(2 * d_rel * D, gs.n, qs), rnd(2 * batch, gr.n, qin)
        s_pre = None if rng.random() < 0.5 else [rng.randrange(1, q) for q in qs]
        worst = gadget == "triv" and not wide and dup == 0 and not pow_in and rng.random() < 0.25
        if worst:
            s_pre = rng.choice([None, [q - 1 for q in qs]])
            lin, ks, cts = tunnel_worst_operands(cref, rp, sp, qs, batch, s_pre is not None, True)(nprng, d_rel, D, gr.n, gs.n)
        opts = {"tunnel_ep": rng.choice([0, 1]), "tunnel_mac": rng.choice([0, 1]), "scratch_mib": rng.choice([1, 4096]),
                "tunnel_fused": rng.choice([0, 2, 4]) if gadget == "triv" else 0}
        for k, v in opts.items(): gs.set_option(k, v)
        tun = A.Tunnel(gr, gs, gs.upload(lin), gs.upload(ks), gadget=capi.ALCH_GAD_BASE2 if gadget == "base2" else capi.ALCH_GAD_TRIV)
        out = gs.alloc(2 * batch)
        gin_ring = A.Ring(rp, qin) if dup else gr
        gin = gin_ring.upload(cts)
        tun.apply(gin, out, batch, s_pre=s_pre, flags=(capi.ALCH_POW_OUT if pow_out else 0) | (capi.ALCH_POW_IN if pow_in else 0))
        got = out.download()
        assert_reduced(got, qs)
        # the oracle's input: CRT basis on all L limbs (modSwitch up: x -> (0, q_a x))
        Oin = cref.GenRing(rp, qin)
        crt_in = [Oin.crt(np.ascontiguousarray(c)) for c in cts] if pow_in else list(cts)
        if dup:
            mult = math.prod(qs[:dup])
            crt_in = [np.ascontiguousarray(np.concatenate([np.zeros((gr.n, dup), dtype=np.int64), Oin.scale(np.ascontiguousarray(c), [mult % q for q in qin])], axis=1))
                      for c in crt_in]
        case = dict(rp=rp, sp=sp, qs=qs, gadget=gadget, batch=batch, pow_in=pow_in, pow_out=pow_out, dup=dup, opts=opts, seed=seed)
        for ct in range(batch):
            w0, w1 = oracle_tunnel(cref, rp, sp, qs, list(lin), list(ks), crt_in[2 * ct], crt_in[2 * ct + 1], s_pre, pow_out=pow_out, gadget=gadget)
            if not (np.array_equal(got[2 * ct], w0) and np.array_equal(got[2 * ct + 1], w1)):
                print("MISMATCH", dict(case, ct=ct)); return 1
        if not np.array_equal(gin.download(), cts):
            print("INPUT CHANGED", case); return 1
        cases += 1
        shape = "e' = s'" if ep == sp else "d_rel 1" if d_rel == 1 else "d_rel %d" % d_rel
        key = (gadget, "%d-byte" % gs.word_bytes, shape, "edge moduli" if edges else "drawn moduli", "worst case" if worst else "uniform",
               "11" if (rp * sp) % 11 == 0 else "-", "dup" if dup else "pow_in" if pow_in else "crt_in")
        tally[key] = tally.get(key, 0) + 1
        if cases % 20 == 0: print(f"{cases} cases, {time.time() - t0:.0f} s", flush=True)
    for k in sorted(tally): print(k, tally[k])
    print(f"OK: {cases} random tunnels bit-exact against the oracle ({refused} index pairs refused by alch_tunnel_info; seed {seed})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
