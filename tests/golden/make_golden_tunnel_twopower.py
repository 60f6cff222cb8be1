#!/usr/bin/env python3
"""Regenerates tests/golden/tunnel_twopower_small.json from the exact model (oracle/model_gen.py): run from the repo root,
    python tests/golden/make_golden_tunnel_twopower.py
Valid tunnel instances between TWO-POWER ciphertext rings that the radix-16 engine serves (r', s' >= 32), one per tower
(r, s, r', s') and gadget: (4, 8, 32, 64) goes up (R' = E' inside S', d_rel = 1), (64, 32, 64, 32) goes down (S' = E', d_rel = 2).
Record layout of tunnel_small.json (make_golden_general.py, `tunnel_vectors`) plus the key "gadget" ("triv" / "base2"): linear
function, tunnel hint, MSD input ciphertext over R'_q, SymmSHE.tunnel's output over S'_q and f(pt); three limbs of 21 bits (so that the
BaseBGad 2 hints, 63 rows per coefficient, keep the file small), all values Python
ints, ring elements limb-major [L][n] on the Pow basis."""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

from oracle import model_gen as G      # noqa: E402
from helpers import primes_1_mod       # noqa: E402

TOWERS = ((4, 8, 32, 64, 4), (64, 32, 64, 32, 4))


def tunnel_vectors():
    import math
    rng = random.Random(20261017)
    out = []
    for r, s, rp, sp, p in TOWERS:
        for gadget in ("triv", "base2"):
            T = G.tunnel_indices(r, s, rp, sp)
            qs = primes_1_mod(rp * sp // math.gcd(rp, sp), 3, 1 << 20)     # 21-bit moduli: BaseBGad 2 rows stay few and short
            sk_in, sk_out = G.g_gen_sk(T.rp, rng), G.g_gen_sk(T.sp, rng)
            ys = [[rng.randrange(p) for _ in range(T.s.n)] for _ in range(T.r.n // T.e.n)]
            pt = [rng.randrange(p) for _ in range(T.r.n)]
            ct = G.g_to_msd(G.g_mod_switch_up(G.g_encrypt(sk_in, pt, T.r, T.rp, p, qs[1:], rng), qs[:1]))
            lin_q, hints = G.g_tunnel_hint(ys, T, p, sk_in, sk_out, qs, rng, gadget=gadget)
            tun = G.g_tunnel(lin_q, hints, ct, T, gadget=gadget)
            down = G.g_mod_switch_down(tun, 1)
            want = G.eval_lin_dec(ys, G.linv_def(pt, T.r, p), T.e, T.r, T.s, p)
            assert G.g_decrypt(sk_out, down) == want
            out.append({"r": r, "s": s, "rp": rp, "sp": sp, "ep": T.ep.m, "p": p, "gadget": gadget, "qs": qs, "ys": ys, "pt": pt,
                        "f_of_pt": want, "sk_in": sk_in, "sk_out": sk_out, "lin": lin_q, "hints": hints, "ct_in": ct.c,
                        "ct_out": tun.c, "ct_out_l": tun.l})
    return out


if __name__ == "__main__":
    name = "tunnel_twopower_small.json"
    with open(os.path.join(HERE, name), "w") as f:
        json.dump(tunnel_vectors(), f, separators=(",", ":"))
    print(name, os.path.getsize(os.path.join(HERE, name)), "bytes")
