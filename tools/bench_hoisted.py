#!/usr/bin/env python3
"""Hoisted automorphisms on resident batches, measured (include/alchemy_hip.h, "Hoisted automorphisms").

HIP-event time on the ring's stream (Ring.timer_start / timer_stop), per figure a warm-up block and then the median of 5 blocks of
back-to-back calls (block length calibrated to about 0.1 s), min and max alongside; ONE PROCESS PER CASE (the driver starts a fresh
child for each, so no case inherits another's scratch, clocks or cached tables).  64 resident ciphertexts on four 31-bit limbs:
n = 2^15 (radix-16 engine) and H5' = 20475 (general engine, phi = 8640).
  cases   R in {2, 8, 32} units x {TrivGad, BaseBGad 2}
  arms    alch_ct_automorph_hoisted (R output batches); its sum form (ALCH_AUTO_SUM, one output batch); R back-to-back
          alch_ct_automorph calls on the same build -- the comparator, existing code
  bar     a gain (or a loss) is claimed only where the median ratio differs from 1 by more than twice the larger relative [min, max]
          spread of the two arms' blocks (DESIGN section 11's bar); otherwise the line says "within the spread"
  --ab    instead: alch_ct_automorph alone, `--label NAME`; run alternately with ALCH_LIB_PATH naming the parent commit's library to
          see that the existing path did not move.  It touches no new symbol.
Lines are appended to profiles/automorph_hoisted.jsonl (`--fresh` truncates it first)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

QS_2P = [2147352577, 2146959361, 2146041857, 2145976321]            # the four largest primes below 2^31 that are 1 mod 2^16
BLOCKS = 5
RINGS = {"n = 2^15": 1 << 16, "H5' = 20475": 20475}
GADGETS = {"TrivGad": 0, "BaseBGad 2": 1}
OUT = os.path.join(ROOT, "profiles", "automorph_hoisted.jsonl")


def primes_1_mod(m, count, hi):
    """The `count` largest primes below hi that are 1 mod m (trial division: 31-bit candidates)."""
    out, q = [], ((hi - 2) // m) * m + 1
    while len(out) < count:
        if q % 2 and all(q % d for d in range(3, int(q ** 0.5) + 1, 2)):
            out.append(q)
        q -= m
    return out


def units(m, count):
    """`count` distinct units of Z_m^* other than 1, spread over the group."""
    import math
    us = [j for j in range(2, m) if math.gcd(j, m) == 1]
    step = max(1, len(us) // count)
    return [us[(7 + i * step) % len(us)] for i in range(count)]


def measure(ring, fn):
    """(median, min, max, calls per block) milliseconds per call of fn."""
    fn()
    ring.sync()
    ring.timer_start()
    for _ in range(3):
        fn()
    per = max(ring.timer_stop() / 3, 1e-3)
    reps = int(max(3, min(2000, 100.0 / per)))
    for _ in range(reps):                                            # the warm-up block
        fn()
    ring.sync()
    ms = []
    for _ in range(BLOCKS):
        ring.timer_start()
        for _ in range(reps):
            fn()
        ms.append(ring.timer_stop() / reps)
    return statistics.median(ms), min(ms), max(ms), reps


def fig(t):
    return {"ms": round(t[0], 5), "ms_min_max": [round(t[1], 5), round(t[2], 5)], "calls_per_block": t[3], "blocks": BLOCKS}


def spread(t):
    return (t[2] - t[1]) / t[0]


def verdict(comparator, arm):
    ratio, bar = comparator[0] / arm[0], 2 * max(spread(comparator), spread(arm))
    word = "gain" if ratio - 1 > bar else "loss: call alch_ct_automorph there" if 1 - ratio > bar else "within the spread"
    return {"comparator_over_arm": round(ratio, 4), "bar": round(bar, 4), "verdict": word}


def one_case(a):
    import torch  # noqa: F401  (one HIP runtime per process: before the library)
    import alchemy_amd as A
    from alchemy_amd import capi
    m = RINGS[a.ring]
    qs = QS_2P if m == 1 << 16 else primes_1_mod(m, 4, 1 << 31)
    gadget, B, R = GADGETS[a.gadget], a.batch, a.units
    ring = A.Ring(m, qs)
    D = ring.gadget_digits(gadget)
    js = units(m, R)
    cts = ring.alloc(2 * B)
    cts.fill_uniform(3)
    base = {"build": a.label, "library": os.path.relpath(capi.lib_path(), ROOT), "ring": a.ring, "index": m, "n": ring.n, "limbs": ring.L,
            "word_bytes": ring.word_bytes, "ciphertexts": B, "gadget": a.gadget, "digits": D, "units": R}
    ks = ring.alloc(2 * D * R)
    ks.fill_uniform(2)
    autos = []
    for r, j in enumerate(js):
        autos.append(A.Automorph(ring, j, ks.view(2 * D * r, 2 * D), gadget))
    res = ring.alloc(2 * B)

    def back_to_back():
        for auto in autos:
            A.ct_automorph(auto, cts, B, out=res)

    if a.ab:
        tc = measure(ring, back_to_back)
        return {**base, "what": f"(ab) {R} back-to-back alch_ct_automorph calls alone", "ct_automorph_x_units": fig(tc)}
    aset = A.AutomorphSet(ring, js, ks, gadget)
    out_all, out_sum = ring.alloc(2 * B * R), ring.alloc(2 * B)
    th = measure(ring, lambda: A.ct_automorph_hoisted(aset, cts, B, out=out_all))
    tc = measure(ring, back_to_back)
    ts = measure(ring, lambda: A.ct_automorph_hoisted(aset, cts, B, out=out_sum, sum=True))
    return {**base, "what": "hoisted and its sum form vs R back-to-back alch_ct_automorph calls", "hoisted": fig(th), "hoisted_sum": fig(ts),
            "ct_automorph_x_units": fig(tc), "hoisted_vs_comparator": verdict(tc, th), "sum_vs_comparator": verdict(tc, ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--label", default="this build")
    ap.add_argument("--fresh", action="store_true")
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--ring", choices=sorted(RINGS))
    ap.add_argument("--gadget", choices=sorted(GADGETS))
    ap.add_argument("--units", type=int)
    a = ap.parse_args()
    if a.ring and a.gadget and a.units:                               # a child: one case, one line on stdout
        print(json.dumps(one_case(a)), flush=True)
        return
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w" if a.fresh else "a") as out:
        cases = [(r, g, u) for r in RINGS for g in GADGETS for u in ((8,) if a.ab else (2, 8, 32))]
        for ring, gadget, n_units in cases:
            cmd = [sys.executable, os.path.abspath(__file__), "--batch", str(a.batch), "--label", a.label, "--ring", ring, "--gadget", gadget,
                   "--units", str(n_units)] + (["--ab"] if a.ab else [])
            child = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if child.returncode != 0:
                sys.stderr.write(child.stdout[-2000:] + child.stderr[-2000:])
                raise SystemExit(f"case {ring} / {gadget} / {n_units} units ended with status {child.returncode}")
            line = child.stdout.strip().split("\n")[-1]
            json.loads(line)
            print(line, flush=True)
            print(line, file=out, flush=True)


if __name__ == "__main__":
    main()
