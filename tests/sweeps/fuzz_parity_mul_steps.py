#!/usr/bin/env python3
"""Randomised sweep of mul_ one SHE operation at a time against the fused entry points: random ring (two-power 32 .. 2^16, or
m = 2^a 3^b 5^c 7^d 13^e with phi(m) <= 3000), 30-bit moduli, or 59-bit or just below 2^62 on two-power rings, or (two-power rings) an edge pair of helpers.word32_edge_rings -- around 2^30, either side of the balanced / unbalanced boundary -- behind the largest primes below its qmax, 2..5 limbs, TrivGad or BaseBGad 2, random
launch options (split_fused, gen_fused, rs_lin, scratch_mib), batch 1..9, with and without s_pre.  Per case, on uniform words or on the
extreme residues of helpers.extreme_words (s_pre = -1 then):
  key_switch_quad(mul(a, b, s))                              == alch_ct_mul_relin(a, b, s)          (s also split between the calls)
  mod_switch(key_switch_quad(mod_switch_deg(mul, ., 2)))     == alch_ct_mul_full                    (TrivGad: up; BaseBGad 2: down)
  the same chain with ALCH_POW_IN / ALCH_POW_OUT on every step == the CRT-basis chain
  mod_switch_deg(degree 1)                                   == alch_ct_mod_switch
every comparison word for word.
usage: tests/sweeps/fuzz_parity_mul_steps.py [seconds] [seed]"""
import os, random, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import alchemy_amd as A
from alchemy_amd import capi
from alchemy_amd import mulsteps as MS
from helpers import extreme_words, primes_1_mod, primes_below, word32_edge_rings

TRIV, BASE2, PIN, POUT = capi.ALCH_GAD_TRIV, capi.ALCH_GAD_BASE2, capi.ALCH_POW_IN, capi.ALCH_POW_OUT


def phi(m):
    r, p, t = m, 2, m
    while p * p <= t:
        if t % p == 0:
            r -= r // p
            while t % p == 0: t //= p
        p += 1
    return r - r // t if t > 1 else r


def uniform(ring, count, seed):
    b = ring.alloc(count); b.fill_uniform(seed); return b


def operands(ring, count, seed, extreme):
    if not extreme: return uniform(ring, count, seed)
    return ring.upload(extreme_words(np.random.default_rng(seed), count, ring.n, ring.qs))


def same(x, y, count):
    return x.checksum(0, count) == y.checksum(0, count) and (x.ring.n > 4096 or np.array_equal(x.download(0, count), y.download(0, count)))


def main():
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else int(time.time())
    rng = random.Random(seed)
    t0, cases, tally = time.time(), 0, {}
    print(f"seed {seed}", flush=True)
    while time.time() - t0 < budget:
        pow2 = rng.random() < 0.5
        if pow2:
            m = 1 << rng.choice([5, 6, 8, 10, 11, 12, 13, 14, 15, 16, 17])
        else:
            m = 2 ** rng.choice([0, 0, 2, 3, 5]) * 3 ** rng.choice([0, 1, 2]) * 5 ** rng.choice([0, 1, 2]) * 7 ** rng.choice([0, 1]) * 13 ** rng.choice([0, 1])
            if m & (m - 1) == 0: continue
        n = phi(m)
        if n < 4 or (not pow2 and n > 3000): continue
        wide = pow2 and m <= 1 << 16 and rng.random() < 0.3
        L = rng.randint(2, 4 if (wide or n >= 1 << 14) else 5)
        gadget = BASE2 if (n <= 4096 and rng.random() < 0.4) else TRIV
        top = wide and rng.random() < 0.5                              # the top of the accepted range instead of its middle
        qs = primes_below(m, L, 1 << 62) if top else primes_1_mod(m, L, lo=(1 << 58) if wide else rng.choice([1 << 28, 1 << 29]))
        edge = None
        if pow2 and not wide and rng.random() < 0.3:                   # the 4-byte dispatch boundaries: q30 or not, balanced or not
            pairs = word32_edge_rings(m)
            edge = rng.choice(sorted(pairs))
            qs = [q for q in primes_below(m, L, max(pairs[edge])) if q not in pairs[edge]][:L - 2] + pairs[edge]
        extreme = rng.random() < 0.3
        batch = rng.randint(1, 3 if n >= 1 << 14 else 9)
        rings = [A.Ring(m, qs[L - k:]) for k in range(1, L + 1)]
        opts = {}
        if rng.random() < 0.5: opts["split_fused"] = rng.choice([0, 1, 2])
        if rng.random() < 0.5: opts["gen_fused"] = rng.choice([0, 1])
        if rng.random() < 0.5: opts["rs_lin"] = rng.choice([0, 1])
        if rng.random() < 0.5: opts["scratch_mib"] = rng.choice([1, 2, 64])
        info = dict(m=m, qs=qs, edge=edge, gadget=gadget, batch=batch, opts=opts, extreme=extreme, seed=seed)
        ring = rings[-1]
        s = None if rng.random() < 0.3 else [q - 1 for q in qs] if extreme else [rng.randrange(1, q) for q in qs]
        a, b = operands(ring, 2 * batch, rng.randrange(1 << 30), extreme), operands(ring, 2 * batch, rng.randrange(1 << 30), extreme)
        sums = (a.checksum(), b.checksum())
        hint = ring.hint_from_buf(operands(ring, 2 * ring.gadget_digits(gadget), rng.randrange(1 << 30), extreme), gadget=gadget)
        want = ring.alloc(2 * batch)
        ring.ct_mul_relin(hint, a, b, want, batch, s_pre=s)
        for r in rings:
            for k, v in opts.items(): r.set_option(k, v)
        quad = MS.ct_mul(a, b, batch, s_pre=s)
        if not same(MS.key_switch_quad(hint, quad, batch), want, 2 * batch):
            print("MISMATCH relin", info); return 1
        if s is not None:
            s1 = [rng.randrange(1, q) for q in qs]
            s2 = [x * pow(y, -1, q) % q for x, y, q in zip(s, s1, qs)]
            if not same(MS.key_switch_quad(hint, MS.ct_mul(a, b, batch, s_pre=s1), batch, s_pre=s2), want, 2 * batch):
                print("MISMATCH relin, split scalar", info); return 1
        # Pow-basis flags on both steps
        ap, bp = ring.alloc(2 * batch), ring.alloc(2 * batch)
        ap.copy_from(a, 2 * batch); bp.copy_from(b, 2 * batch); ap.crtinv(); bp.crtinv()
        qp = MS.ct_mul(ap, bp, batch, s_pre=s, flags=PIN | POUT)
        lp = MS.key_switch_quad(hint, qp, batch, flags=PIN | POUT)
        lp.crt()
        if not same(lp, want, 2 * batch):
            print("MISMATCH relin, Pow flags", info); return 1
        # the whole mul_ over three rings
        if L >= 3:
            if gadget == TRIV:
                l_h = rng.randint(3, L); l_in = rng.randint(max(1, l_h - 2), l_h - 1); l_out = rng.randint(max(1, l_h - 3), l_h - 1)
            else:
                l_in = rng.randint(3, L); l_h = rng.randint(2, l_in - 1); l_out = rng.randint(1, l_h - 1)
            r_in, r_h, r_out = rings[l_in - 1], rings[l_h - 1], rings[l_out - 1]
            info.update(limbs=(l_in, l_h, l_out))
            fa, fb = operands(r_in, 2 * batch, rng.randrange(1 << 30), extreme), operands(r_in, 2 * batch, rng.randrange(1 << 30), extreme)
            fh = r_h.hint_from_buf(operands(r_h, 2 * r_h.gadget_digits(gadget), rng.randrange(1 << 30), extreme), gadget=gadget)
            fs = None if s is None else s[L - l_in:]
            pow_out = POUT if rng.random() < 0.3 else 0
            fwant, got = r_out.alloc(2 * batch), r_out.alloc(2 * batch)
            capi.ct_mul_full(fh, fa, fb, fwant, batch, s_pre=fs, flags=pow_out)
            sw = MS.mod_switch(MS.ct_mul(fa, fb, batch, s_pre=fs), r_h, batch, degree=2)
            lin = MS.key_switch_quad(fh, sw, batch)
            capi.ct_mod_switch(lin, got, batch, pow_out)
            if not same(got, fwant, 2 * batch):
                print("MISMATCH full", info); return 1
            d1 = MS.mod_switch(lin, r_out, batch, degree=1, flags=pow_out)
            if not same(d1, got, 2 * batch):
                print("MISMATCH degree 1", info); return 1
        if (a.checksum(), b.checksum()) != sums:
            print("INPUT MODIFIED", info); return 1
        cases += 1
        key = ("two-power" if pow2 else "general", "62-bit" if top else "60-bit" if wide else edge if edge else "32-bit", "BaseBGad2" if gadget == BASE2 else "TrivGad",
               "extreme" if extreme else "uniform")
        tally[key] = tally.get(key, 0) + 1
        if cases % 25 == 0: print(f"{cases} cases, {time.time() - t0:.0f} s", flush=True)
    for k in sorted(tally): print(k, tally[k])
    print(f"OK: {cases} random mul_ step chains bit-exact against the fused entry points (seed {seed})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
