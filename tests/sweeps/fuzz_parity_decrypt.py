#!/usr/bin/env python3
"""Randomised parity sweep of decrypt / error rates on resident batches: random ring (two-power 32 .. 2^14 or m = 2^a 3^b 5^c 7^d 13^e
with phi(m) <= 3000), 1..8 moduli = 1 mod m (30-bit, or 59-bit or just below 2^62 on two-power rings, balanced or not), words (uniform, or the extreme residues of
helpers.extreme_words), degree, batch and p.  Per case:
alch_ct_error_term against the C restatement (Horner on the CRT basis, crtInv, lInv) word for word, then alch_buf_lift of that result
against Python integers (residues l * (x mod p) mod p and the digit vectors of max |x|), and alch_ct_decrypt_lift against both.
usage: tests/sweeps/fuzz_parity_decrypt.py [seconds] [seed]"""
import os, random, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import alchemy_amd as A
from alchemy_amd import capi
from alchemy_amd import decrypt as D
from oracle import cref
from helpers import extreme_words, primes_1_mod, primes_below


def phi(m):
    r, p, t = m, 2, m
    while p * p <= t:
        if t % p == 0:
            r -= r // p
            while t % p == 0: t //= p
        p += 1
    return r - r // t if t > 1 else r


def to_digits(x, qs):
    out = []
    for q in qs:
        out.append(x % q); x //= q
    return out


def garner(res, qs):
    """(count, n, L) residues -> (count, n) centred integers (object array)."""
    Q = 1
    for q in qs: Q *= q
    x = np.zeros(res.shape[:2], dtype=object)
    for j, q in enumerate(qs):
        Qj = Q // q
        x = (x + res[:, :, j].astype(object) * (Qj * pow(Qj % q, -1, q))) % Q
    return np.where(x > (Q - 1) // 2, x - Q, x)


def main():
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else int(time.time())
    rng, nprng = random.Random(seed), np.random.default_rng(seed)
    cref.build()
    t0, cases, tally = time.time(), 0, {}
    print(f"seed {seed}", flush=True)
    while time.time() - t0 < budget:
        pow2 = rng.random() < 0.4
        if pow2:
            m = 1 << rng.randint(5, 14)
        else:
            m = 2 ** rng.choice([0, 0, 2, 3, 5]) * 3 ** rng.choice([0, 1, 2]) * 5 ** rng.choice([0, 1, 2]) * 7 ** rng.choice([0, 1]) * 13 ** rng.choice([0, 1])
            if m & (m - 1) == 0: continue
        n = phi(m)
        if n < 4 or n > 8192: continue
        if not pow2 and n > 3000: continue
        L = rng.randint(1, 8)
        wide = pow2 and rng.random() < 0.3
        if wide:
            L = min(L, 4)
            top = rng.random() < 0.5                                    # the last primes below 2^62 instead of the first above 2^58
            qs = primes_below(m, L, 1 << 62) if top else primes_1_mod(m, L, lo=1 << 58)
        elif rng.random() < 0.25 and L >= 2:                            # very different sizes: the unbalanced digit path
            qs = primes_1_mod(m, L - 1, lo=0) + primes_1_mod(m, 1, lo=1 << 29)
        else:
            qs = primes_1_mod(m, L, lo=rng.choice([1 << 28, 1 << 29, (1 << 30) + (1 << 29)]))
        if not wide and max(qs) >= 1 << 31: continue
        rng.shuffle(qs)
        degree, batch = rng.randint(1, 2), rng.randint(1, 9)
        p = rng.choice([2, 4, 7, 8, 32, 1 << 30, rng.randrange(2, 1 << 31)])
        l = rng.choice([1, p - 1, rng.randrange(p)])
        flags = capi.ALCH_POW_IN if rng.random() < 0.4 else 0
        extreme = rng.random() < 0.3                                    # key, ciphertexts and scalar from the extreme residues
        s_pre = None if rng.random() < 0.5 else [q - 1 for q in qs] if extreme else [rng.randrange(1, q) for q in qs]
        if extreme: rnd = lambda c: extreme_words(nprng, c, n, qs)
        else: rnd = lambda c: np.stack([np.stack([nprng.integers(0, q, size=n, dtype=np.int64) for q in qs], axis=1) for _ in range(c)])
        g, zp = A.Ring(m, qs), A.Ring(m, [p], nocrt=True)
        general = not (m >= 32 and m & (m - 1) == 0)
        o = cref.GenRing(m, qs) if general else cref.Ring(n, qs)
        per = degree + 1
        cts, sk = rnd(per * batch), rnd(1)
        want = []
        for b in range(batch):
            acc = cts[per * b + degree]
            for c in range(degree - 1, -1, -1): acc = o.add(o.mul(acc, sk[0]), cts[per * b + c])
            if s_pre is not None: acc = o.scale(acc, s_pre)
            acc = o.crtinv(np.ascontiguousarray(acc))
            want.append(o.linv(acc) if general else acc)
        want = np.stack(want)
        gin = g.upload(np.stack([o.crtinv(np.ascontiguousarray(c)) for c in cts]) if flags else cts)
        gsk = g.upload(sk)
        et = D.error_term(gin, batch, gsk, degree=degree, s_pre=s_pre, flags=flags)
        info = dict(m=m, qs=qs, degree=degree, batch=batch, p=p, l=l, flags=flags, extreme=extreme, seed=seed)
        if not np.array_equal(et.download(0, batch), want):
            print("MISMATCH error_term", info); return 1
        x = garner(want, qs)
        want_res = np.array((x * l) % p, dtype=np.int64)
        want_dig = [to_digits(max(abs(int(v)) for v in row), qs) for row in x]
        for name, call in (("lift", lambda d: D.lift(et, d, l=l, want_max=True, count=batch)),
                           ("decrypt_lift", lambda d: D.decrypt_lift(gin, batch, gsk, degree=degree, s_pre=s_pre, dst=d, l=l, want_max=True, flags=flags))):
            dst = zp.alloc(batch)
            digits = call(dst)
            if digits != want_dig or not np.array_equal(dst.download()[:, :, 0], want_res):
                print("MISMATCH", name, info); return 1
            del dst
        del et, gin, gsk
        cases += 1
        key = ("two-power" if pow2 else "general", ("62-bit" if top else "60-bit") if wide else "32-bit", f"L {L}", "extreme" if extreme else "uniform")
        tally[key] = tally.get(key, 0) + 1
        if cases % 25 == 0: print(f"{cases} cases, {time.time() - t0:.0f} s", flush=True)
    for k in sorted(tally): print(k, tally[k])
    print(f"OK: {cases} random decrypt cases exact against the oracle and Python integers (seed {seed})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
