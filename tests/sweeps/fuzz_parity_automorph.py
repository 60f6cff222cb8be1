"""Randomised parity of the Galois automorphisms: per trial a random index (both engines, the split sizes among them), unit j,
moduli class (31-bit / mixed / just below 2^62, or one of the resident edge rings), gadget, batch and placement (plain buffers, or
views in the interior of gapped parents whose every other word is asserted afterwards).
  * alch_buf_automorph against the permutation restated from the header's slot rule (tests/automorph_model.py);
  * alch_ct_automorph against the composition that defines it: alch_buf_automorph, then alch_ct_tunnel from the ring to itself with
    lin_crt = crt(1) and the same hint -- word for word, with a random "scratch_mib" on one trial in three.
The log goes to profiles/fuzz_parity_automorph.log.
Run on the GPU machine:  python tests/sweeps/fuzz_parity_automorph.py [--trials N] [--seed S]"""
import argparse
import math
import os
import random
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: F401,E402  (one HIP runtime per process: before the library)
import alchemy_amd as A  # noqa: E402
import automorph_model as M  # noqa: E402
from alchemy_amd import capi  # noqa: E402
from helpers import Gapped, draw_resident_edge_ring, primes_1_mod, primes_below  # noqa: E402

SMALL = [4, 8, 16, 32, 64, 256, 1 << 11, 3, 7, 9, 11, 13, 21, 27, 45, 60, 63, 91, 121, 169, 420]
LARGE = [1 << 14, 1 << 16, 1 << 17, 11648, 20475]                                    # one trial in eight, batch <= 2


def moduli(rnd, m, L):
    kind = rnd.choice(["w32", "mixed", "w62"])
    if m == 1 << 17:
        kind = "w32"                                                                 # n = 2^16 exists with 4-byte words only
    if kind == "w32":
        return kind, primes_1_mod(m, L, 1 << rnd.choice([20, 29]))
    if kind == "w62":
        return kind, primes_below(m, L, 1 << 62)
    return kind, (primes_1_mod(m, max(1, L - 1), 1 << 17) + primes_below(m, 1, 1 << rnd.choice([40, 62])))[:L] if L > 1 else primes_1_mod(m, 1, 1 << 40)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=160)
    ap.add_argument("--seed", type=int, default=2026)
    a = ap.parse_args()
    rnd = random.Random(a.seed)
    nprng = np.random.default_rng(a.seed)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    bad, gapped_cases = 0, 0
    tables = {}
    with open(os.path.join(ROOT, "profiles", "fuzz_parity_automorph.log"), "w") as log:
        for trial in range(a.trials):
            large = rnd.random() < 0.125
            m, L = rnd.choice(LARGE if large else SMALL), rnd.randint(1, 3)
            if rnd.random() < 0.25 and m != 1 << 17:
                kind, qs = draw_resident_edge_ring(rnd, m)
                if m == 1 << 16 and max(qs) >= 1 << 31:
                    qs = qs[:2]
            else:
                kind, qs = moduli(rnd, m, L)
            L = len(qs)
            ring = A.Ring(m, qs)
            n = ring.n
            j = rnd.choice([u for u in (rnd.randrange(1, max(2, m)) for _ in range(64)) if math.gcd(u, m) == 1] or [1])
            if (m, j) not in tables:
                tables[(m, j)] = np.array(M.table(m, j), dtype=np.int64)
            tab = tables[(m, j)]
            batch = rnd.randint(1, 2 if large else 9)
            gadget = rnd.choice([capi.ALCH_GAD_TRIV, capi.ALCH_GAD_BASE2, capi.ALCH_GAD_BASEPOW2(rnd.randint(2, 16))])
            if large and gadget == capi.ALCH_GAD_BASE2:
                gadget = capi.ALCH_GAD_BASEPOW2(8)                                   # keeps a large ring's hint to a few hundred MiB
            on = rnd.random() < 0.5
            gapped_cases += on
            gp = Gapped(on, nprng, margin=2, tail=2)
            host = np.ascontiguousarray(np.stack([nprng.integers(0, q, size=(2 * batch, n), dtype=np.int64) for q in qs], axis=2))
            cts = gp.operand(ring, host)
            # the buffer call
            perm = gp.result(ring, 2 * batch)
            A.buf_automorph(perm, cts, j)
            got = perm.download()
            ok = np.array_equal(got, host[:, tab, :])
            # the ciphertext call against its definition
            D = ring.gadget_digits(gadget)
            ks = ring.alloc(2 * D)
            ks.fill_uniform(rnd.getrandbits(32))
            mib = None
            if rnd.random() < 0.33:
                mib = rnd.choice([1, 2, 8])
                ring.set_option("scratch_mib", mib)
            s_pre = rnd.choice([None, [q - 1 for q in qs], [rnd.randrange(1, q) for q in qs]])
            lin = ring.upload(np.ones((1, n, L), dtype=np.int64))
            tun = A.Tunnel(ring, ring, lin, ks, gadget=gadget)
            want = ring.alloc(2 * batch)
            tun.apply(perm, want, batch, s_pre=s_pre)
            auto = A.Automorph(ring, j + rnd.choice([0, m]), ks, gadget)
            ks.fill_uniform(1)                                                       # copied at create time
            out = gp.result(ring, 2 * batch)
            A.ct_automorph(auto, cts, batch, s_pre=s_pre, out=out)
            ok = ok and np.array_equal(out.download(), want.download()) and np.array_equal(cts.download(), host)
            try:
                gp.check()
            except AssertionError:
                ok = False
            bad += not ok
            line = (f"trial {trial}: m={m} n={n} L={L} {kind} word={ring.word_bytes} j={j} gadget={gadget:#x} D={D} batch={batch} "
                    f"gapped={int(on)} scratch_mib={mib} s_pre={'none' if s_pre is None else 'set'} -> {'ok' if ok else 'MISMATCH'}")
            print(line, file=log, flush=True)
            if not ok:
                print(line, flush=True)
            auto.free()
            tun.free()
            del cts, perm, out, want, ks, lin, gp
            ring.close()
        tail = f"{a.trials} trials, {bad} mismatches, {gapped_cases} with gapped parents"
        print(tail, file=log)
    print(tail)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
