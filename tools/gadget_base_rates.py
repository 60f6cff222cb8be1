#!/usr/bin/env python3
"""Rates of the BaseBGad 2^w gadget beside its digit count: alch_ct_mul_relin at n = 2^15 on four 31-bit limbs and the five hops of
the reference's Tunnel example (alchemy_amd.tunnelhops, its moduli), at w = 1, 2, 4, 8 in ONE process.

The rule of DESIGN section 11: same box, same day, alternating runs -- every round visits every width once, `--rounds` rounds, and the
figure of a width is the median over the rounds with the spread (max - min) / median next to it.  w = 1 is ALCH_GAD_BASE2 itself.
The tool predicts nothing: it prints D(w) and the measured rate, one JSON line per workload.

The reference arm, BaseBGad 2 on another commit: `--tree DIR --widths 1` imports `alchemy_amd` from a built checkout of that commit
(width 1 uses only what the package had before the gadget code existed).  Run the two commands alternately, several times each; a
process is one sample of its arm, and `--compare A.log B.log` then prints, per workload, each arm's median over its processes, its
spread (max - min) / median, the relative difference of the medians and the bar of twice the larger spread.

    python tools/gadget_base_rates.py [--rounds 5] [--batch 64] [--hop-batch 16] [--widths 1,2,4,8] [--tree DIR]
    python tools/gadget_base_rates.py --compare this_tree.log other_tree.log"""
import argparse
import json
import os
import statistics
import sys

MUL_QS = [2147352577, 2146959361, 2146041857, 2145976321]


def code(w):
    return capi.ALCH_GAD_BASE2 if w == 1 else capi.ALCH_GAD_BASEPOW2(w)


class MulRelin:
    def __init__(self, w, batch):
        self.B, self.ring = batch, A.Ring(1 << 16, MUL_QS)
        self.D = self.ring.gadget_digits(code(w))
        src = self.ring.alloc(2 * self.D)
        src.fill_uniform(1)
        self.hint = self.ring.hint_from_buf(src, gadget=code(w))
        self.a, self.b, self.out = (self.ring.alloc(2 * batch) for _ in range(3))
        self.a.fill_uniform(2); self.b.fill_uniform(3)

    def measure(self, reps):
        run = lambda: self.ring.ct_mul_relin(self.hint, self.a, self.b, self.out, self.B)
        run(); self.ring.sync()
        self.ring.timer_start()
        for _ in range(reps):
            run()
        return reps * self.B / (self.ring.timer_stop() * 1e-3)


def summarise(name, unit, widths, digits, samples):
    row = {"workload": name, "unit": unit}
    for w in widths:
        med = statistics.median(samples[w])
        row["w%d" % w] = {"D": digits[w], "rate": round(med, 1), "spread": round((max(samples[w]) - min(samples[w])) / med, 4)}
    print(json.dumps(row), flush=True)


def compare(path_a, path_b):
    """Two logs, each the concatenated output of several processes of one arm at one width."""
    def arm(path):
        runs = {}
        for line in open(path):
            if line.startswith('{"workload"'):
                row = json.loads(line)
                key = [k for k in row if k.startswith("w") and k != "workload"][0]
                runs.setdefault(row["workload"].split(" (")[0], []).append(row[key]["rate"])
        return runs
    a, b = arm(path_a), arm(path_b)
    for name in a:
        ma, mb = statistics.median(a[name]), statistics.median(b[name])
        sa, sb = (max(a[name]) - min(a[name])) / ma, (max(b[name]) - min(b[name])) / mb
        print(json.dumps({"workload": name, "a": {"median": round(ma, 1), "spread": round(sa, 4), "runs": len(a[name])},
                          "b": {"median": round(mb, 1), "spread": round(sb, 4), "runs": len(b[name])},
                          "a_over_b_minus_1": round(ma / mb - 1, 4), "bar": round(2 * max(sa, sb), 4)}))


def main():
    global A, capi, tunnelhops
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--compare", nargs=2, metavar=("A_LOG", "B_LOG"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--hop-batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--widths", default="1,2,4,8")
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare)
    widths = [int(x) for x in args.widths.split(",")]
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch  # noqa: F401  (before the HIP library: one HIP runtime per process)
    import alchemy_amd as A
    from alchemy_amd import capi, tunnelhops

    muls = {w: MulRelin(w, args.batch) for w in widths}
    samples = {w: [] for w in widths}
    for _ in range(args.rounds):
        for w in widths:
            samples[w].append(muls[w].measure(args.reps))
    summarise("ct_mul_relin n=2^15 L=4", "ops/s", widths, {w: muls[w].D for w in widths}, samples)
    del muls

    for k in range(5):
        hops = {w: tunnelhops.Hop(k, args.hop_batch) if w == 1 else tunnelhops.Hop(k, args.hop_batch, gadget=code(w)) for w in widths}
        samples = {w: [] for w in widths}
        for _ in range(args.rounds):
            for w in widths:
                samples[w].append(hops[w].measure(args.reps)[0])
        h0 = hops[widths[0]]
        summarise("Tunnel.hs hop %d (limbs %d/%d/%d at w=%d)" % (k + 1, h0.lin, h0.lh, h0.lout, widths[0]), "hops/s",
                  widths, {w: hops[w].D for w in widths}, samples)
        del hops


if __name__ == "__main__":
    main()
