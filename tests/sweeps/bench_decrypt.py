"""Rate of alch_ct_decrypt_lift -- c(s) on the decoding basis, centred lift, residues mod p and the digit vectors of max |lift| --
on a resident batch of linear ciphertexts, next to the per-ciphertext path it replaces.
Rings: n = 2^15 with the four config-3 moduli, and H5' = F20475 (phi 8640) with four HomomRLWR moduli; 8192 ciphertexts (--batch).
Reported per ring, one JSON line: ciphertexts/s (HIP-event time of the whole call), the fraction of the byte roofline at the device
word -- compulsory bytes: read both components, the key once, write one Z_p word per coefficient -- for the call with both outputs,
residues alone and digits alone, and the rate of the per-ciphertext path on the same box: one alch_ct_error_term per ciphertext,
L * n words downloaded, the lift on the host (numpy-vectorised Garner here, so a bound from above on the C++ mirror's scalar loop).
Run on the GPU box:  python tests/sweeps/bench_decrypt.py [--batch N] [--reps R]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import torch  # noqa: F401,E402  (one HIP runtime per process: before the library)
import alchemy_amd as A  # noqa: E402
from alchemy_amd import decrypt as D  # noqa: E402

RLWR = [1543651201, 689270401, 718099201, 720720001, 1556755201, 1567238401]
CFG3 = [2147352577, 2146959361, 2146041857, 2145976321]
HBM_PEAK_GBS = 8000.0


def host_lift(res, qs, p):
    """(n, L) residues -> residues mod p and max |x| / Q: mixed-radix digits, sign from the top digit down (vectorised)."""
    L = len(qs)
    d = []
    for j in range(L):
        t = res[:, j].astype(object)
        for i in range(j):
            t = (t - d[i]) * pow(qs[i], -1, qs[j]) % qs[j]
        d.append(t)
    x = d[L - 1]
    for j in range(L - 2, -1, -1):
        x = x * qs[j] + d[j]
    Q = 1
    for q in qs:
        Q *= q
    x = np.where(x > (Q - 1) // 2, x - Q, x)
    return x % p, max(abs(int(v)) for v in x) / Q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-cts", type=int, default=8)
    a = ap.parse_args()
    p = 32
    for name, m, qs in (("n = 2^15, 4 limbs", 1 << 16, CFG3), ("H5' (phi 8640), 4 limbs", 20475, list(reversed(RLWR[:4])))):
        r, zp = A.Ring(m, qs), A.Ring(m, [p], nocrt=True)
        B, L, n, w = a.batch, len(qs), r.n, r.word_bytes
        cts, sk, dst = r.alloc(2 * B), r.alloc(1), zp.alloc(B)
        cts.fill_uniform(1)
        sk.fill_uniform(2)
        s_pre = [p % q for q in qs]
        algo = B * 2 * L * n * w + L * n * w + B * n * 4
        out = {"ring": name, "batch": B, "word_bytes": w, "compulsory_bytes": algo}
        for label, d, want_max in (("both", dst, True), ("residues", dst, False), ("digits", None, True)):
            D.decrypt_lift(cts, B, sk, s_pre=s_pre, dst=d, l=3, want_max=want_max)       # warm-up: scratch allocation
            best = 1e30
            for _ in range(a.reps):
                r.timer_start()
                D.decrypt_lift(cts, B, sk, s_pre=s_pre, dst=d, l=3, want_max=want_max)
                best = min(best, r.timer_stop())
            out[label] = {"ms": round(best, 3), "ciphertexts_per_s": round(B / best * 1e3, 1),
                          "frac_of_byte_roofline": round(algo / (best * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
        # the per-ciphertext path: c(s) of one ciphertext on the device, L * n words to the host, the lift there
        one = r.alloc(1)
        t0 = time.perf_counter()
        for b in range(a.host_cts):
            D.error_term(cts.view(2 * b, 2), 1, sk, s_pre=s_pre, out=one)
            host_lift(one.download()[0], qs, p)
        out["per_ciphertext_host_path_ciphertexts_per_s"] = round(a.host_cts / (time.perf_counter() - t0), 1)
        print(json.dumps(out), flush=True)
        del cts, sk, dst, one


if __name__ == "__main__":
    main()
