#!/usr/bin/env python3
"""Randomised parity sweep of alch_ct_tunnel between TWO-POWER rings of the radix-16 engine: random pairs of distinct (and, now and
then, equal) indices 32 .. 2^13, 1..8 moduli = 1 mod the larger index near 2^28, 2^30, 2^59 or just below 2^62 (32- and 64-bit words) or from the
ends of the group-size classes of the lazy inner product (helpers.threshold_moduli), TrivGad or
BaseBGad 2 hints, ciphertexts 0..2 limbs below the hint's ring, random linear functions, hints, ciphertexts, encoding scalars (uniform words, or the
extreme residues of helpers.extreme_words with s_pre = -1, or the worst case helpers.tunnel_worst_operands on 32-bit TrivGad cases), all four
ALCH_POW_IN / ALCH_POW_OUT combinations, batches of 1..9 and a small scratch now and then (several chunks), against the C restatement's
composition (tests/helpers.py::oracle_tunnel).  usage: tests/sweeps/fuzz_parity_tunnel_twopower.py [seconds] [seed] [max cases]"""
import os, random, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import alchemy_amd as A
from alchemy_amd import capi
from oracle import cref
from helpers import extreme_words, oracle_tunnel, primes_1_mod, primes_below, threshold_moduli, tunnel_worst_operands


def main():
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else int(time.time())
    max_cases = int(sys.argv[3]) if len(sys.argv) > 3 else 1 << 30
    rng, nprng = random.Random(seed), np.random.default_rng(seed)
    cref.build()
    t0, cases, tally = time.time(), 0, {}
    print(f"seed {seed}", flush=True)
    while time.time() - t0 < budget and cases < max_cases:
        rp, sp = 1 << rng.randint(5, 13), 1 << rng.randint(5, 13)
        if rp == sp and rng.random() < 0.9: continue
        lo = rng.choice([0, 0, 1 << 28, 1 << 30, 1 << 30, 1 << 59, 1 << 62])                  # 0: the class ends
        L = rng.randint(1, 8)
        if lo == 0: qs = threshold_moduli(rng, max(rp, sp), L)
        else: qs = primes_below(max(rp, sp), L, 1 << 62) if lo == 1 << 62 else primes_1_mod(max(rp, sp), L, lo=lo)   # 2^62: the last primes BELOW it
        if lo < 1 << 31 and max(qs) >= 1 << 31: continue
        dup = rng.choice([0, 0, 1, 2])
        if dup >= L: dup = 0
        gadget = rng.choice(["triv", "triv", "base2"])
        worst = gadget == "triv" and lo < 1 << 31 and rng.random() < 0.3
        if worst: dup = 0
        gr, gs = A.Ring(rp, qs), A.Ring(sp, qs)
        gin_ring = A.Ring(rp, qs[dup:]) if dup else gr
        ep, d_rel = A.Tunnel.info(gr, gs)
        D = gs.gadget_digits(capi.ALCH_GAD_BASE2) if gadget == "base2" else L
        if d_rel * D * L * gs.n > 3_000_000: continue               # keep the oracle's work per case small
        batch = rng.randint(1, 9) if d_rel * D * gs.n < 300_000 else rng.randint(1, 2)
        extreme = rng.random() < 0.3
        if extreme: rnd = lambda c, n, ms: extreme_words(nprng, c, n, ms)
        else: rnd = lambda c, n, ms: np.stack([np.stack([nprng.integers(0, q, size=n, dtype=np.int64) for q in ms], axis=1) for _ in range(c)])
        lin, ks, cts = rnd(d_rel, gs.n, qs), rnd(2 * d_rel * D, gs.n, qs), rnd(2 * batch, gr.n, qs[dup:])
        s_pre = None if rng.random() < 0.5 else [q - 1 for q in qs] if extreme or worst else [rng.randrange(1, q) for q in qs]
        if worst: lin, ks, cts = tunnel_worst_operands(cref, rp, sp, qs, batch, s_pre is not None, True)(nprng, d_rel, D, gr.n, gs.n)
        flags = rng.choice([0, 0, capi.ALCH_POW_IN, capi.ALCH_POW_OUT, capi.ALCH_POW_IN | capi.ALCH_POW_OUT])
        small_scratch = rng.random() < 0.25
        if small_scratch: gs.set_option("scratch_mib", 1)
        # the oracle takes CRT-basis ciphertexts on the hint's ring: modSwitch up (x -> (0, q_a x)) done here with exact integers
        mult = 1
        for q in qs[:dup]: mult *= q
        up = []
        for c in cts:
            scaled = np.stack([(c[:, j].astype(object) * mult % qs[dup + j]).astype(np.int64) for j in range(L - dup)], axis=1)
            up.append(np.ascontiguousarray(np.concatenate([np.zeros((gr.n, dup), dtype=np.int64), scaled], axis=1)))
        Oin, Os = cref.GenRing(rp, qs[dup:]), cref.GenRing(sp, qs)
        src = np.stack([Oin.crtinv(np.ascontiguousarray(c)) for c in cts]) if flags & capi.ALCH_POW_IN else cts
        tun = A.Tunnel(gr, gs, gs.upload(lin), gs.upload(ks), gadget=capi.ALCH_GAD_BASE2 if gadget == "base2" else capi.ALCH_GAD_TRIV)
        gin, out = gin_ring.upload(src), gs.alloc(2 * batch)
        tun.apply(gin, out, batch, s_pre=s_pre, flags=flags)
        got = out.download()
        case = dict(rp=rp, sp=sp, qs=qs, dup=dup, gadget=gadget, batch=batch, flags=flags, small_scratch=small_scratch, extreme=extreme, seed=seed)
        for ct in range(batch):
            w0, w1 = oracle_tunnel(cref, rp, sp, qs, list(lin), list(ks), up[2 * ct], up[2 * ct + 1], s_pre,
                                   pow_out=bool(flags & capi.ALCH_POW_OUT), gadget=gadget)
            if not (np.array_equal(got[2 * ct], w0) and np.array_equal(got[2 * ct + 1], w1)):
                print("MISMATCH", dict(case, ct=ct)); return 1
        if not np.array_equal(gin.download(), src):
            print("INPUT MODIFIED", case); return 1
        cases += 1
        key = (gadget, "up" if sp > rp else "down" if rp > sp else "same", "62-bit" if lo == 1 << 62 else "%d-bit" % (64 if lo > 1 << 31 else 32), "dup %d" % dup,
               "edge moduli" if lo == 0 else "drawn moduli", "worst case" if worst else "extreme" if extreme else "uniform")
        tally[key] = tally.get(key, 0) + 1
        if cases % 20 == 0: print(f"{cases} cases, {time.time() - t0:.0f} s", flush=True)
    for k in sorted(tally): print(k, tally[k])
    print(f"OK: {cases} random two-power tunnels bit-exact against the oracle (seed {seed})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
