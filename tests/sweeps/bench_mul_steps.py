"""Cost of running mul_ one SHE operation at a time: HIP-event time of the four-step chain (alch_ct_mul, alch_ct_mod_switch_deg,
alch_ct_key_switch_quad, alch_ct_mod_switch) against alch_ct_mul_full on the same resident batch, and of alch_ct_mul alone against a
device-to-device copy of the bytes it must move (4 elements read, 3 written per ciphertext).
Shapes: n = 2^15 with 4 -> 5 -> 3 limbs, and H5' = F20475 (phi 8640) with 3 -> 4 -> 2 of four HomomRLWR moduli; TrivGad.
Each figure is the median of 5 blocks of --reps calls after a warm-up block (scratch allocation, clocks).  The chain is expected to
be slower than the fused call -- it is composed and it materialises the quadratic ciphertext; the ratio is recorded, not gated.
One JSON line per shape.  Run on the GPU box:  python tests/sweeps/bench_mul_steps.py [--batch N] [--reps R]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import torch  # noqa: F401,E402  (one HIP runtime per process: before the library)
import alchemy_amd as A  # noqa: E402
from alchemy_amd import capi  # noqa: E402
from alchemy_amd import mulsteps as MS  # noqa: E402

RLWR = [1543651201, 689270401, 718099201, 720720001, 1556755201, 1567238401]
CFG3 = [2147352577, 2146959361, 2146041857, 2145976321]                    # config 3: 31-bit primes = 1 mod 2^16


def timed(ring, fn, reps, blocks=5):
    for _ in range(reps):                                                    # warm-up block
        fn()
    out = []
    for _ in range(blocks):
        ring.timer_start()
        for _ in range(reps):
            fn()
        out.append(ring.timer_stop() / reps)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    B = a.batch
    from oracle.model import is_prime
    q5 = next(q for q in range(CFG3[-1] - (1 << 16), 1 << 30, -(1 << 16)) if is_prime(q))      # a fifth modulus below the four
    CFG5 = [q5] + CFG3
    for name, m, qs, (l_in, l_h, l_out) in (("n = 2^15, 4 -> 5 -> 3 limbs", 1 << 16, CFG5, (4, 5, 3)),
                                            ("H5' (phi 8640), 3 -> 4 -> 2 limbs", 20475, list(reversed(RLWR[:4])), (3, 4, 2))):
        L = len(qs)
        r_in, r_h, r_out = A.Ring(m, qs[L - l_in:]), A.Ring(m, qs[L - l_h:]), A.Ring(m, qs[L - l_out:])
        for r in (r_in, r_out):
            r.share_stream(r_h)                                             # one stream: the events of one ring time all four steps
        x, y = r_in.alloc(2 * B), r_in.alloc(2 * B)
        x.fill_uniform(1)
        y.fill_uniform(2)
        hb = r_h.alloc(2 * l_h)
        hb.fill_uniform(3)
        hint = r_h.hint_from_buf(hb)
        out_f, out_c = r_out.alloc(2 * B), r_out.alloc(2 * B)
        quad, up, lin = r_in.alloc(3 * B), r_h.alloc(3 * B), r_h.alloc(2 * B)

        def fused():
            capi.ct_mul_full(hint, x, y, out_f, B)

        def chain():
            MS.ct_mul(x, y, B, out=quad)
            MS.mod_switch(quad, r_h, B, degree=2, out=up)
            MS.key_switch_quad(hint, up, B, out=lin)
            capi.ct_mod_switch(lin, out_c, B)

        src, dst = r_in.alloc(4 * B), r_in.alloc(4 * B)

        def copy():                                                         # 4 elements read + 4 written; scaled to 4 + 3 below
            dst.copy_from(src, 4 * B)

        t_f, t_c = timed(r_h, fused, a.reps), timed(r_h, chain, a.reps)
        same = out_f.checksum() == out_c.checksum()
        t_m = timed(r_h, lambda: MS.ct_mul(x, y, B, out=quad), a.reps)
        t_cp = timed(r_h, copy, a.reps) * 7.0 / 8.0
        eb = r_in.n * l_in * r_in.word_bytes
        print(json.dumps({"shape": name, "batch": B, "gadget": "TrivGad", "bit_equal": same,
                          "mul_full_ms": round(t_f, 3), "step_chain_ms": round(t_c, 3), "chain_over_fused": round(t_c / t_f, 2),
                          "ct_mul_ms": round(t_m, 3), "copy_same_bytes_ms": round(t_cp, 3), "ct_mul_over_copy": round(t_m / t_cp, 2),
                          "ct_mul_GBps": round(7 * B * eb / (t_m * 1e-3) / 1e9, 1)}), flush=True)
        del x, y, hb, out_f, out_c, quad, up, lin, src, dst


if __name__ == "__main__":
    main()
