"""One ring tunnel between two-power cyclotomic rings on a resident batch: `modSwitch_ .: tunnel_ hint .: modSwitch_`
(PT2CT.hs:224-229) with both rings on the radix-16 engine (m >= 32).  The two-power counterpart of tunnelhops.Hop.

The hint lives on `l_hint` limbs of ring_s = S'; the input batch on the last `l_in <= l_hint` limbs of R' (the leading modSwitch up is
part of alch_ct_tunnel), the result on the last `l_out <= l_hint` limbs of S'.  Moduli are the first primes q = 1 (mod 2^18) above
2^29 -- the size of examples/Tunnel.hs:34-39's -- so one list serves every index up to 2^17 + 1 step of margin; pass `qs` for others.
Residues, linear function and hints are synthetic (seeds below).  Used by tools/bench_tunnel.py and tests/test_gpu_tunnel_twopower.py."""
from . import capi
from .capi import Ring, Tunnel

SEED_LIN, SEED_KS, SEED_X = 1, 2, 3


def _is_prime(n):
    if n < 2:
        return False
    for p in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if n % p == 0:
            return n == p
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):      # deterministic below 3.3e24
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def primes_1_mod(m, count, lo):
    """The first `count` primes q > lo with q = 1 (mod m)."""
    out, q = [], (lo // m) * m + 1
    while len(out) < count:
        if q > lo and _is_prime(q):
            out.append(q)
        q += m
    return out


def tunnel_sized_moduli(L):
    return primes_1_mod(1 << 18, L, 1 << 29)


class TwoPowerHop:
    """One hop R' (index rp) -> S' (index sp), both powers of two >= 32, with resident hint and a seeded input batch."""

    def __init__(self, rp, sp, batch, l_hint=6, l_in=None, l_out=None, gadget=capi.ALCH_GAD_BASE2, qs=None, ring_opts=()):
        self.rp, self.sp, self.B, self.gadget = rp, sp, batch, gadget
        self.lh = l_hint
        self.lin = l_hint if l_in is None else l_in
        self.lout = l_hint if l_out is None else l_out
        self.qs = list(qs) if qs is not None else tunnel_sized_moduli(l_hint)
        assert len(self.qs) == l_hint and 1 <= self.lin <= l_hint and 1 <= self.lout <= l_hint
        self._rings = {}
        self.ring_opts = tuple(ring_opts)
        self.rin, self.rr = self.ring(rp, self.lin), self.ring(rp, l_hint)
        self.rs, self.ro = self.ring(sp, l_hint), self.ring(sp, self.lout)
        self.e_prime, self.d_rel = Tunnel.info(self.rr, self.rs)
        self.D = self.rs.gadget_digits(gadget)
        self.lin_buf, self.ks = self.rs.alloc(self.d_rel), self.rs.alloc(2 * self.d_rel * self.D)
        self.lin_buf.fill_uniform(SEED_LIN); self.ks.fill_uniform(SEED_KS)
        self.tun = Tunnel(self.rr, self.rs, self.lin_buf, self.ks, gadget=gadget)
        self.x = self.rin.alloc(2 * batch)
        self.x.fill_uniform(SEED_X)
        self.mid = self.rs.alloc(2 * batch)
        self.out = self.ro.alloc(2 * batch) if self.lout != l_hint else None

    def ring(self, m, L):
        if (m, L) not in self._rings:
            r = Ring(m, self.qs[self.lh - L:])                   # the last L limbs of the hint's ring
            for name, v in self.ring_opts:
                r.set_option(name, v)
            self._rings[(m, L)] = r
        return self._rings[(m, L)]

    def run(self, first=0, count=None):
        """modSwitch . tunnel hint . modSwitch on ciphertexts [first, first + count) of the batch (default: all of it); returns the
        result buffer (CRT basis over S', l_out limbs)."""
        count = self.B - first if count is None else count
        src, mid = self.x, self.mid
        if first or count != self.B:
            src, mid = self.x.view(2 * first, 2 * count), self.mid.view(2 * first, 2 * count)
        self.tun.apply(src, mid, count)                          # the leading modSwitch up is folded into the tunnel
        if self.out is not None:
            out = self.out if mid is self.mid else self.out.view(2 * first, 2 * count)
            capi.ct_mod_switch(mid, out, count)
            return self.out
        return self.mid

    def measure(self, reps=1):
        """ciphertexts per second over `reps` back-to-back runs, HIP events on ring_s's stream (one warm-up run first)."""
        self.run(); self.rs.sync()
        self.rs.timer_start()
        for _ in range(reps):
            res = self.run()
        return reps * self.B / (self.rs.timer_stop() * 1e-3), res

    def algorithmic_bytes(self):
        """Compulsory bytes of one hop at the reference's 8-byte word: one linear ciphertext in (l_in limbs over R'), one out
        (l_out limbs over S')."""
        return 2 * 8 * (self.lin * self.rin.n + self.lout * self.ro.n)
