"""GPU: stream ordering of the entry points that touch several rings, several internal streams or pooled buffers -- on LOADED streams
and on CALLER-OWNED streams (alch_ring_set_stream, the null stream included).

Every other GPU test makes its call on idle streams, where the host is slower than the kernels and queue order equals issue order:
a missing wait, a kernel on the wrong stream or a scratch buffer reused too early still gives the right words there.  Here a ballast
of transform round trips (tests/stream_load.py) is queued in front of the call under test, and every case asserts that the loaded
stream is still busy when the call has returned: only then did the call's kernels really wait in a queue, and only then does the case
count.  Expected values come from the C restatement and the index model in oracle/, every comparison is bit for bit, every
downloaded batch is checked for reduced words.  "Garbage" is always a reduced uniform fill: a wrong order yields wrong words, never
an out-of-range access.

Hazards, for an entry point whose source, work and output rings may differ:
  RAW        the source holds garbage; ballast on the SOURCE ring's stream, then copy_from(real) on that stream, then the call
  WAR        ballast on the WORK ring's stream, the call, then the source is overwritten with garbage on its own ring's stream
  hand-back  ballast on the WORK ring's stream, the call, then the output is downloaded through its own ring at once
Stream modes: "ring" (every ring on the stream the library gave it), "caller" (every ring on a torch.cuda.Stream of its own),
"null" (the work ring bound to the null stream with set_stream(0), ballast through a ballast ring bound the same way).

Calls that synchronise the host before they return (alch_ct_mul_full with a BaseBGad 2 hint, alch_pt_rescale, alch_buf_lift and
alch_ct_decrypt_lift with max_digits) leave nothing queued, so for them -- and only for them: mul_full_base2, pt_rescale, lift_max,
decrypt_lift_max -- the busy assert stands right BEFORE the call, after the producer has been queued behind the ballast; they run a
fourth hazard, WAW: garbage is written to the output behind ballast on the output ring's stream, then the call.  The results are
pinned, not the synchronisation.

Limits of what a run can show.  Two streams that the runtime has put on one hardware queue run in issue order whatever the events
say; between such a pair a missing wait cannot show, which pairs those are changes with the number of live streams, and it is not
the same set from run to run.  One set of rings is therefore alive at a time (Case.dev), and every entry point runs in two or three
stream modes.  The join of alch_ct_mul_relin's lanes is checked by a download right after the call, but lane 0 is the ring's own
stream and always holds at least as much work as any other lane, so a missing join shows only when another lane happens to finish
last: that test can fail on a broken join, it is not certain to.
"""
import math

import numpy as np
import pytest

import alchemy_amd as A
from alchemy_amd import capi, mulsteps
from helpers import (assert_reduced, oracle_full_mul, oracle_full_mul_general, oracle_tunnel, primes_1_mod)
from stream_load import Ballast, busy

pytestmark = pytest.mark.gpu

RLWR_QS = [1543651201, 689270401, 718099201, 720720001, 1556755201, 1567238401]
HAZARDS = ["raw", "war", "handback"]


def rand_elems(rng, count, n, qs):
    return np.stack([np.stack([rng.integers(0, q, size=n, dtype=np.int64) for q in qs], axis=1) for _ in range(count)])


def per_limb(fn, x):
    """A model function on one limb's coefficient list, applied to every limb of an (n, L) element."""
    return np.ascontiguousarray(np.stack([np.array(fn(x[:, j].tolist()), dtype=np.int64) for j in range(x.shape[1])], axis=1))


# ---- the ballast: one ring for the whole module, re-bound to the stream under test ---------------------------------------------
_BALLAST = []


def ballast_on(stream_of):
    if not _BALLAST:
        _BALLAST.append(Ballast(stream_of))
    else:
        _BALLAST[0].bind(stream_of)
    return _BALLAST[0]


# ---- one set of rings of a case in one stream mode ---------------------------------------------------------------------------------
class Dev:
    """work: the ring whose stream carries the call; src_ring / out_ring: the rings the operands and the result live on (any of the
    three may coincide); call(bufs, out) makes the call under test; keep: handles that must outlive it (hints, tunnels)."""

    def __init__(self, mode, work, src_ring, out_ring, call, keep=(), others=()):
        import torch
        self.mode, self.work, self.src_ring, self.out_ring, self.call, self.keep = mode, work, src_ring, out_ring, call, keep
        self.rings = []
        for r in (work, src_ring, out_ring) + tuple(others):
            if all(r is not x for x in self.rings):
                self.rings.append(r)
        self.sync()                                   # set-up work (hint and tunnel uploads) ran on the rings' first streams
        self.streams = []
        if mode == "caller":
            for r in self.rings:
                s = torch.cuda.Stream()
                assert s.cuda_stream != 0 and all(s.cuda_stream != t.cuda_stream for t in self.streams)
                r.set_stream(s.cuda_stream)
                assert r.device_stream()[1] == s.cuda_stream
                self.streams.append(s)
        elif mode == "null":
            work.set_stream(0)
            assert work.device_stream()[1] == 0
        else:
            assert mode == "ring"
            ptrs = [r.device_stream()[1] for r in self.rings]
            assert 0 not in ptrs and len(set(ptrs)) == len(ptrs)

    def close(self):
        for k in self.keep:
            k.free()
        self.keep = ()
        for r in self.rings:
            r.close()

    def sync(self):
        for r in self.rings:
            r.sync()


class Case:
    """Host operands `srcs` (arrays of elements of the source ring), the oracle's result `want` (elements of the output ring) and
    make(mode) -> Dev.  Built once per module; the rings are made per run of one mode's hazards."""

    def __init__(self, srcs, want, make, want_ret=None):
        self.srcs, self.want, self.make, self.want_ret = [np.ascontiguousarray(s) for s in srcs], np.ascontiguousarray(want), make, want_ret
        self.want.setflags(write=False)

    def dev(self, mode):
        """One set of rings is alive at a time: the runtime spreads all live streams over a few hardware queues, and the more rings a
        process holds, the more often two streams of a case share a queue and run in issue order whatever the events say -- a missing
        wait between them then cannot show (measured: with every set kept alive, half the cases passed with ext_order switched off)."""
        if not _LIVE or _LIVE[0][0] != (id(self), mode):
            fresh = self.make(mode)                   # before the old set goes: new streams, not the old ones' places over again
            if _LIVE:
                _LIVE.pop()[1].close()
            _LIVE.append(((id(self), mode), fresh))
        return _LIVE[0][1]


_LIVE = []


def check(got, case, dev):
    assert_reduced(got, dev.out_ring.qs)
    bad = [e for e in range(len(case.want)) if not np.array_equal(got[e], case.want[e])]
    assert not bad, f"elements {bad} of {len(case.want)} differ from the oracle"


def run_hazard(case, mode, hazard):
    dev = case.dev(mode)
    dev.sync()
    reals = [dev.src_ring.upload(x) for x in case.srcs]
    out = dev.out_ring.alloc(len(case.want))
    out.fill_uniform(4242)                            # never a stale right answer in a recycled buffer
    if hazard == "raw":
        bufs = [dev.src_ring.alloc(len(x)) for x in case.srcs]
        for i, b in enumerate(bufs):
            b.fill_uniform(77 + i)
        dev.sync()
        loaded = dev.src_ring
        ballast_on(loaded).push()
        for b, r in zip(bufs, reals):
            b.copy_from(r, r.n_elems)
        dev.call(bufs, out)
        assert busy(loaded), "the ballast drained before the call returned: the case proved nothing"
    else:
        dev.sync()
        loaded = dev.work
        ballast_on(loaded).push()
        dev.call(reals, out)
        assert busy(loaded), "the ballast drained before the call returned: the case proved nothing"
        if hazard == "war":
            for i, b in enumerate(reals):
                b.fill_uniform(991 + i)               # on the source ring's stream
    check(out.download(), case, dev)                  # synchronises the output ring's stream only
    dev.sync()


def run_synced_hazard(case, mode, hazard):
    """The hazards of a call that synchronises the host before it returns: the loaded stream is asserted busy right before the call."""
    dev = case.dev(mode)
    dev.sync()
    reals = [dev.src_ring.upload(x) for x in case.srcs]
    out = dev.out_ring.alloc(len(case.want))
    out.fill_uniform(4242)
    drained = "the ballast drained before the call was made: the case proved nothing"
    if hazard == "raw":
        bufs = [dev.src_ring.alloc(len(x)) for x in case.srcs]
        for i, b in enumerate(bufs):
            b.fill_uniform(77 + i)
        dev.sync()
        ballast_on(dev.src_ring).push()
        for b, r in zip(bufs, reals):
            b.copy_from(r, r.n_elems)
        assert busy(dev.src_ring), drained
        ret = dev.call(bufs, out)
    elif hazard == "waw":
        assert dev.out_ring is not dev.work
        dev.sync()
        ballast_on(dev.out_ring).push()
        out.fill_uniform(4343)                        # behind the ballast: must land before the call's result, not on top of it
        assert busy(dev.out_ring), drained
        ret = dev.call(reals, out)
    else:
        dev.sync()
        ballast_on(dev.work).push()
        assert busy(dev.work), drained
        ret = dev.call(reals, out)
        if hazard == "war":
            for i, b in enumerate(reals):
                b.fill_uniform(991 + i)
    check(out.download(), case, dev)
    assert case.want_ret is None or ret == case.want_ret
    dev.sync()


# ---- cases ----------------------------------------------------------------------------------------------------------------------------
_CASES = {}


def case(name, oracle_lib):
    if name not in _CASES:
        _CASES[name] = (BUILDERS.get(name) or SYNCED[name])(oracle_lib)
    return _CASES[name]


def ext_case(kind):
    """embed / twace / coeffs between the rings of index 12 and 60 (n = 4 and 16), two limbs, four elements: the destination ring works."""
    def build(oracle_lib):
        from oracle import model_gen as G
        ms, mb, count = 12, 60, 4
        qs = primes_1_mod(60, 2, 1 << 29)
        s, b = G.Index(ms), G.Index(mb)
        rng = np.random.default_rng(len(kind) * 7 + ord(kind[-1]))
        op, basis = kind.split("_") if "_" in kind else (kind, None)
        src = rand_elems(rng, count, (s if op == "embed" else b).n, qs)
        if op == "embed":
            fn = {"pow": lambda v: G.embed_pow(v, s, b), "crt": lambda v: G.embed_crt_def(v, s, b)}.get(basis)
            if basis == "dec":
                want = np.stack([np.stack([np.array(G.embed_dec_def(x[:, j].tolist(), s, b, q), dtype=np.int64) for j, q in enumerate(qs)], axis=1)
                                 for x in src])
            else:
                want = np.stack([per_limb(fn, x) for x in src])
        elif op == "twace":
            if basis == "crt":
                want = np.stack([np.stack([np.array(G.twace_crt_def(x[:, j].tolist(), s, b, q), dtype=np.int64) for j, q in enumerate(qs)], axis=1)
                                 for x in src])
            else:
                want = np.stack([per_limb(lambda v: G.twace_pow_dec(v, s, b), x) for x in src])
        else:
            want = np.concatenate([np.stack([np.array(c, dtype=np.int64) for c in zip(*[G.coeffs(x[:, j].tolist(), s, b) for j in range(len(qs))])])
                                   .transpose(0, 2, 1) for x in src])
        code = {"pow": capi.ALCH_BASIS_POW, "dec": capi.ALCH_BASIS_DEC, "crt": capi.ALCH_BASIS_CRT}.get(basis)

        def make(mode):
            rs, rb = A.Ring(ms, qs), A.Ring(mb, qs)
            if op == "embed":
                return Dev(mode, rb, rs, rb, lambda bufs, out: out.embed_from(bufs[0], count, code))
            if op == "twace":
                return Dev(mode, rs, rb, rs, lambda bufs, out: out.twace_from(bufs[0], count, code))
            return Dev(mode, rs, rb, rs, lambda bufs, out: out.coeffs_from(bufs[0], count))
        return Case([src], np.ascontiguousarray(want), make)
    return build


def mod_switch_case(m, degree, up):
    """alch_ct_mod_switch (degree 1) / alch_ct_mod_switch_deg (degree 2) between three and two limbs, batch 3: the bigger ring works."""
    def build(oracle_lib):
        gen = m & (m - 1) != 0
        qs = primes_1_mod(m, 3, 1 << 29) if gen else primes_1_mod(m, 3, 1 << 30)
        mk = (lambda q: oracle_lib.GenRing(m, q)) if gen else (lambda q: oracle_lib.Ring(m // 2, q))
        ob, osm = mk(qs), mk(qs[1:])
        per, batch = degree + 1, 3
        rng = np.random.default_rng(m + 10 * degree + up)
        if up:
            src = rand_elems(rng, per * batch, osm.n if gen else m // 2, qs[1:])
            scaled = [osm.scale(x, [qs[0] % q for q in qs[1:]]) for x in src]
            want = np.stack([np.concatenate([np.zeros((x.shape[0], 1), dtype=np.int64), x], axis=1) for x in scaled])
        else:
            src = rand_elems(rng, per * batch, ob.n if gen else m // 2, qs)
            want = []
            for e, x in enumerate(src):
                cur = ob.crtinv(x)
                dec = gen and e % per == 0                        # c0 is rescaled on the decoding basis, c1 and c2 on the powerful basis
                cur = osm.l(ob.rescale_drop0(ob.linv(cur))) if dec else ob.rescale_drop0(cur)
                want.append(osm.crt(cur))
            want = np.stack(want)

        def make(mode):
            big, small = A.Ring(m, qs), A.Ring(m, qs[1:])
            if degree == 1:
                call = lambda bufs, out: capi.ct_mod_switch(bufs[0], out, batch)
            else:
                call = lambda bufs, out: mulsteps.mod_switch(bufs[0], out.ring, batch, degree=2, out=out)
            return Dev(mode, big, small if up else big, big if up else small, call)
        return Case([src], want, make)
    return build


def mul_full_case(general):
    """alch_ct_mul_full, TrivGad hint, three distinct rings, 4 -> 5 -> 3 limbs: the hint's ring works.
    Two-power: n = 2^11, option chunk = 8 and batch 11, so the fused path forks onto its second stream and joins (two chunks).
    General index 20475 (n = 8640): the unfused path, option rs_lin = 0 (rescale_down_limbs) and scratch_mib = 1; batch 3."""
    def build(oracle_lib):
        if general:
            m, batch = 20475, 3
            qs_h = list(reversed(RLWR_QS[:5]))
            n = oracle_lib.GenRing(m, qs_h).n
        else:
            m, batch = 1 << 12, 11
            qs_h = primes_1_mod(m, 5, 1 << 30)
            n = m // 2
        rng = np.random.default_rng(m + 5)
        hint = rand_elems(rng, 10, n, qs_h)
        a, b = rand_elems(rng, 2 * batch, n, qs_h[1:]), rand_elems(rng, 2 * batch, n, qs_h[1:])
        s_pre = [int(rng.integers(1, q)) for q in qs_h[1:]]
        want = []
        for ct in range(batch):
            if general:
                w = oracle_full_mul_general(oracle_lib, m, qs_h, 4, 3, list(hint), a[2 * ct], a[2 * ct + 1], b[2 * ct], b[2 * ct + 1], s_pre)
            else:
                w = oracle_full_mul(oracle_lib, n, qs_h, 4, 3, list(hint), a[2 * ct], a[2 * ct + 1], b[2 * ct], b[2 * ct + 1], s_pre)
            want += [w[0], w[1]]

        def make(mode):
            rh, rin, rout = A.Ring(m, qs_h), A.Ring(m, qs_h[1:]), A.Ring(m, qs_h[2:])
            if general:
                rh.set_option("rs_lin", 0)
                rh.set_option("scratch_mib", 1)
                # do_mul_full_unfused: a chunk's scratch is (2 + stage + 4) elements of the hint's ring per ciphertext, stage >= 0
                eb = 5 * n * rh.word_bytes
                assert batch > (1 << 20) // (6 * eb), "one chunk would hold the whole batch"
            else:
                rh.set_option("chunk", 8)
                assert batch > 8
            gh = rh.hint_load(hint)
            return Dev(mode, rh, rin, rout, lambda bufs, out: capi.ct_mul_full(gh, bufs[0], bufs[1], out, batch, s_pre=s_pre), keep=(gh,))
        return Case([a, b], np.stack(want), make)
    return build


def up_switched(osm, cts, q_front, qs_tail):
    """modSwitch up by one limb of CRT-basis elements: (0, q_front x)."""
    return [np.ascontiguousarray(np.concatenate([np.zeros((x.shape[0], 1), dtype=np.int64), osm.scale(x, [q_front % q for q in qs_tail])], axis=1))
            for x in cts]


_TUNNEL_WANT = {}


def tunnel_case(rp, sp, L, batch, gadget="triv", flags=0, ep=1, dup=1, chunked=True):
    """alch_ct_tunnel: the target ring works; the input lives on the last L - dup limbs of R' (a third ring; with the private E'
    ring of a general-index pair that makes four)."""
    def build(oracle_lib):
        gen = rp & (rp - 1) != 0
        qs = RLWR_QS[:L] if rp > 1000 and gen else primes_1_mod(rp * sp // math.gcd(rp, sp), L, 1 << 29)
        Or, Os, Oin = oracle_lib.GenRing(rp, qs), oracle_lib.GenRing(sp, qs), oracle_lib.GenRing(rp, qs[dup:])
        n_r, n_s = Or.n, Os.n
        d_rel = n_r // oracle_lib.GenRing(math.gcd(rp, sp), qs).n
        D = L if gadget == "triv" else sum((q - 1).bit_length() for q in qs)
        rng = np.random.default_rng(rp + sp + L)
        lin, ks = rand_elems(rng, d_rel, n_s, qs), rand_elems(rng, 2 * d_rel * D, n_s, qs)
        cts = rand_elems(rng, 2 * batch, n_r, qs[dup:])
        s_pre = [int(rng.integers(1, q)) for q in qs]
        up = up_switched(Oin, cts, qs[0], qs[dup:]) if dup else list(cts)
        assert dup in (0, 1)
        key = (rp, sp, L, batch, gadget, dup)          # the same draw whatever the flags and options: one oracle run serves them all
        if key not in _TUNNEL_WANT:
            _TUNNEL_WANT[key] = [w for ct in range(batch)
                                 for w in oracle_tunnel(oracle_lib, rp, sp, qs, list(lin), list(ks), up[2 * ct], up[2 * ct + 1], s_pre, gadget=gadget)]
        want = _TUNNEL_WANT[key]
        if flags & capi.ALCH_POW_OUT:
            want = [Os.crtinv(np.ascontiguousarray(w)) for w in want]
        src = np.stack([Oin.crtinv(np.ascontiguousarray(c)) for c in cts]) if flags & capi.ALCH_POW_IN else cts

        def make(mode):
            gr, gs, gin = A.Ring(rp, qs), A.Ring(sp, qs), A.Ring(rp, qs[dup:]) if dup else None
            gs.set_option("tunnel_ep", ep)
            gs.set_option("scratch_mib", 1)
            assert A.Tunnel.info(gr, gs)[1] == d_rel
            if chunked:
                # the LARGEST chunk do_tunnel / do_tunnel_pow2 can choose with 1 MiB (per_ct of their comments, least scratch variant)
                wb, Lx = gs.word_bytes, L - dup
                ebr = Lx * n_r * wb
                if gen:
                    n_x = n_r // d_rel if ep else n_s                                  # E' (private ring) or S'
                    per_ct = 2 * ebr + 2 * d_rel * Lx * n_x * wb                       # the fused form keeps no digits in memory
                elif gadget == "base2":
                    assert rp > sp                                                     # down: transforms at n_s
                    per_ct = d_rel * D * L * n_s * wb                                  # the digits alone
                else:
                    assert rp > sp and not flags & capi.ALCH_POW_IN
                    per_ct = 2 * ebr + d_rel * Lx * n_s * wb + d_rel * Lx * L * n_s * wb
                assert batch > (1 << 20) // per_ct, "one chunk would hold the whole batch"
            tun = A.Tunnel(gr, gs, gs.upload(lin), gs.upload(ks), gadget=capi.ALCH_GAD_BASE2 if gadget == "base2" else capi.ALCH_GAD_TRIV)
            call = lambda bufs, out: tun.apply(bufs[0], out, batch, s_pre=s_pre, flags=flags)
            return Dev(mode, gs, gin if dup else gr, gs, call, keep=(tun,), others=(gr,))
        return Case([src], np.stack(want), make)
    return build


def centred_lift(x, qs):
    """(n, L) residues -> n Python integers in (-Q/2, Q/2]: the integer the residues stand for (CRT recombination, then centred)."""
    Q = math.prod(qs)
    out = []
    for row in x.tolist():
        v = sum(r * (Q // q) * pow(Q // q, -1, q) for r, q in zip(row, qs)) % Q
        out.append(v - Q if v > (Q - 1) // 2 else v)
    return out


def lift_case(decrypt, want_max=False):
    """alch_buf_lift / alch_ct_decrypt_lift on the two-power ring of index 64, two limbs, into a Z_p ring of its own, p = 8, scalar
    l = 3: the source ring works.  want_max: max_digits requested too (the call then synchronises the host)."""
    def build(oracle_lib):
        from alchemy_amd import decrypt as D
        m, p, l, batch = 64, 8, 3, 4
        qs = primes_1_mod(m, 2, 1 << 29)
        o = oracle_lib.Ring(m // 2, qs)
        rng = np.random.default_rng(64 + decrypt)
        if decrypt:
            cts, sk = rand_elems(rng, 2 * batch, m // 2, qs), rand_elems(rng, 1, m // 2, qs)
            elems = [o.crtinv(o.add(cts[2 * e], o.mul(cts[2 * e + 1], sk[0]))) for e in range(batch)]     # c(s); Dec = Pow on a two-power index
            srcs = [cts, sk]
        else:
            elems = list(rand_elems(rng, batch, m // 2, qs))
            srcs = [np.stack(elems)]
        lifts = [centred_lift(x, qs) for x in elems]
        want = np.stack([np.array([(l * v) % p for v in x], dtype=np.int64).reshape(-1, 1) for x in lifts])
        digits = None
        if want_max:                                  # mixed-radix digits of the largest |lift| of every element, limb 0 least significant
            digits = []
            for x in lifts:
                v, row = max(abs(c) for c in x), []
                for q in qs:
                    row.append(v % q)
                    v //= q
                digits.append(row)

        def make(mode):
            r, zp = A.Ring(m, qs), A.Ring(m, [p], nocrt=True)
            if decrypt:
                call = lambda bufs, out: D.decrypt_lift(bufs[0], batch, bufs[1], dst=out, l=l, want_max=want_max)
            else:
                call = lambda bufs, out: D.lift(bufs[0], out, l=l, want_max=want_max)
            return Dev(mode, r, r, zp, call)
        return Case(srcs, want, make, want_ret=digits)
    return build


def pt_mul_case(oracle_lib):
    """alch_pt_mul: operands and result on a Z_p ring (index 32, p = 32), the lifting ring works."""
    from alchemy_amd import plaintext
    from oracle import model_gen as G
    m, p, batch = 32, 32, 3
    idx = G.Index(m)
    rng = np.random.default_rng(32)
    a, b = rng.integers(0, p, size=(batch, idx.n, 1), dtype=np.int64), rng.integers(0, p, size=(batch, idx.n, 1), dtype=np.int64)
    want = np.array([G.ring_mul_def(x[:, 0].tolist(), y[:, 0].tolist(), idx, p) for x, y in zip(a, b)], dtype=np.int64).reshape(batch, idx.n, 1)
    qs = primes_1_mod(m, 2, 1 << 30)

    def make(mode):
        lift, zp = A.Ring(m, qs), A.Ring(m, [p], nocrt=True)
        return Dev(mode, lift, zp, zp, lambda bufs, out: plaintext.pt_mul(lift, out, bufs[0], bufs[1], batch))
    return Case([a, b], want, make)


def pt_eval_lin_case(oracle_lib):
    """alch_pt_eval_lin, 32 -> 24 over p = 4: source ring, destination ring, the ring the function's values came from and the lifting
    ring of the target index, which works."""
    from alchemy_amd import plaintext
    from oracle import model_gen as G
    r, s, p, batch = 32, 24, 4, 3
    E, R, S = G.Index(math.gcd(r, s)), G.Index(r), G.Index(s)
    rng = np.random.default_rng(24)
    ys = rng.integers(0, p, size=(R.n // E.n, S.n, 1), dtype=np.int64)
    xs = rng.integers(0, p, size=(batch, R.n, 1), dtype=np.int64)
    want = np.array([G.eval_lin_dec([y[:, 0].tolist() for y in ys], G.linv_def(x[:, 0].tolist(), R, p), E, R, S, p) for x in xs],
                    dtype=np.int64).reshape(batch, S.n, 1)
    qs = primes_1_mod(s, 2, 1 << 30)

    def make(mode):
        lift, zr, zs, zy = A.Ring(s, qs), A.Ring(r, [p], nocrt=True), A.Ring(s, [p], nocrt=True), A.Ring(s, [p], nocrt=True)
        f = plaintext.pt_linear(lift, zy.upload(ys), r)
        return Dev(mode, lift, zr, zs, lambda bufs, out: f.apply(bufs[0], out, batch), keep=(f,), others=(zy,))
    return Case([xs], want, make)


def pt_rescale_case(oracle_lib):
    """alch_pt_rescale (div2_) from Z_32 to Z_16 on index 32, every coefficient even: the destination ring works and the call reads its
    divisibility flag back, so it synchronises the host."""
    from alchemy_amd import plaintext
    m, p, p2, batch = 32, 32, 16, 3
    rng = np.random.default_rng(16)
    half = rng.integers(0, p2, size=(batch, m // 2, 1), dtype=np.int64)

    def make(mode):
        zs, zd = A.Ring(m, [p], nocrt=True), A.Ring(m, [p2], nocrt=True)
        return Dev(mode, zd, zs, zd, lambda bufs, out: plaintext.pt_rescale(bufs[0], out, batch))
    return Case([2 * half], half, make, want_ret=True)


def mul_full_base2_case(oracle_lib):
    """alch_ct_mul_full with a BaseBGad 2 hint, three rings of index 128 on 2 -> 3 -> 1 limbs, batch 2: host-synchronised today."""
    n, batch, qs_h = 64, 2, [268440577, 8392193, 1073750017]
    D = sum((q - 1).bit_length() for q in qs_h)
    rng = np.random.default_rng(128)
    hint = rand_elems(rng, 2 * D, n, qs_h)
    a, b = rand_elems(rng, 2 * batch, n, qs_h[1:]), rand_elems(rng, 2 * batch, n, qs_h[1:])
    s_pre = [int(rng.integers(1, q)) for q in qs_h[1:]]
    want = [w for ct in range(batch) for w in oracle_full_mul(oracle_lib, n, qs_h, 2, 1, list(hint), a[2 * ct], a[2 * ct + 1], b[2 * ct],
                                                              b[2 * ct + 1], s_pre, gadget="base2")]

    def make(mode):
        rh, rin, rout = A.Ring(2 * n, qs_h), A.Ring(2 * n, qs_h[1:]), A.Ring(2 * n, qs_h[2:])
        assert rh.gadget_digits(capi.ALCH_GAD_BASE2) == D
        gh = rh.hint_load(hint, gadget=capi.ALCH_GAD_BASE2)
        return Dev(mode, rh, rin, rout, lambda bufs, out: capi.ct_mul_full(gh, bufs[0], bufs[1], out, batch, s_pre=s_pre), keep=(gh,))
    return Case([a, b], np.stack(want), make)


def gauss_case(oracle_lib):
    """alch_buf_gauss_dec with a coset on a Z_p ring (index 45: both odd-prime passes and the ring's double scratch; p = 7; two
    limbs; four elements) against the sampler's model: the destination ring works, the coset ring is the source."""
    import gauss_model as GM
    from alchemy_amd import encrypt as E
    m, p, count, seed, elem0 = 45, 7, 4, 0xA1C45, 1000
    qs = primes_1_mod(m, 2, 1 << 29)
    svar = 3.0 / math.sqrt(GM.totient(m)) * float(p) * float(p)
    coset = np.random.default_rng(45).integers(0, p, size=(count, GM.totient(m), 1), dtype=np.int64)
    z = GM.gauss_dec(m, svar, seed, elem0, count, p, coset[:, :, 0])
    assert np.array_equal(np.mod(z, p), coset[:, :, 0]) and int(np.abs(z).max()) > p // 2

    def make(mode):
        ring, zp = A.Ring(m, qs), A.Ring(m, [p], nocrt=True)
        return Dev(mode, ring, zp, ring, lambda bufs, out: E.gauss_dec(out, svar, seed, 0, count, bufs[0], 0, elem0))
    return Case([coset], GM.words(z, qs), make)


BUILDERS = {
    "gauss_dec_coset": gauss_case,
    "lift": lift_case(False), "decrypt_lift": lift_case(True), "pt_mul": pt_mul_case, "pt_eval_lin": pt_eval_lin_case,
    "embed_pow": ext_case("embed_pow"), "embed_dec": ext_case("embed_dec"), "embed_crt": ext_case("embed_crt"),
    "twace_pow": ext_case("twace_pow"), "twace_dec": ext_case("twace_dec"), "twace_crt": ext_case("twace_crt"), "coeffs": ext_case("coeffs"),
    "ms_pow2_down": mod_switch_case(1 << 12, 1, False), "ms_pow2_up": mod_switch_case(1 << 12, 1, True),
    "ms_pow2_deg2_down": mod_switch_case(1 << 12, 2, False), "ms_pow2_deg2_up": mod_switch_case(1 << 12, 2, True),
    "ms_gen_down": mod_switch_case(455, 1, False), "ms_gen_up": mod_switch_case(455, 1, True),
    "ms_gen_deg2_down": mod_switch_case(455, 2, False), "ms_gen_deg2_up": mod_switch_case(455, 2, True),
    "mul_full_fused": mul_full_case(False), "mul_full_unfused": mul_full_case(True),
    # the reference's first hop H0' -> H1' on three limbs, input on two; the chunk counts are asserted in make()
    "tunnel_gen_ep": tunnel_case(11648, 29120, 3, 8), "tunnel_gen_noep": tunnel_case(11648, 29120, 3, 8, ep=0),
    "tunnel_gen_pow_in_out": tunnel_case(11648, 29120, 3, 8, flags=capi.ALCH_POW_IN | capi.ALCH_POW_OUT),
    "tunnel_small_base2": tunnel_case(40, 60, 3, 3, gadget="base2", chunked=False),
    "tunnel_small_base2_pow": tunnel_case(40, 60, 3, 3, gadget="base2", flags=capi.ALCH_POW_IN | capi.ALCH_POW_OUT, chunked=False),
    "tunnel_pow2": tunnel_case(1 << 13, 1 << 12, 3, 6), "tunnel_pow2_small": tunnel_case(32, 64, 3, 3, chunked=False),
    "tunnel_pow2_base2": tunnel_case(64, 32, 3, 3, gadget="base2", flags=capi.ALCH_POW_OUT, chunked=False),
    # BaseBGad 2 over several chunks (one ciphertext's digits alone exceed 1 MiB), Pow basis in and out
    "tunnel_pow2_base2_chunked": tunnel_case(1 << 13, 1 << 12, 3, 2, gadget="base2", flags=capi.ALCH_POW_IN | capi.ALCH_POW_OUT),
}
# calls that synchronise the host before they return: run_synced_hazard
SYNCED = {"mul_full_base2": mul_full_base2_case, "pt_rescale": pt_rescale_case, "lift_max": lift_case(False, True),
          "decrypt_lift_max": lift_case(True, True)}
SYNCED_RUNS = [(n, h) for n in SYNCED for h in HAZARDS + ["waw"] if not (n == "pt_rescale" and h == "waw")]   # its output ring works
# the work ring on the null stream: the two-ring modSwitch, the unfused mul_ and every tunnel
NULL_CASES = ["embed_dec", "ms_pow2_down", "ms_pow2_up", "ms_gen_down", "ms_gen_up", "mul_full_unfused"] + [k for k in BUILDERS if k.startswith("tunnel")]


@pytest.mark.parametrize("hazard", HAZARDS)
@pytest.mark.parametrize("mode", ["ring", "caller"])
@pytest.mark.parametrize("name", list(BUILDERS))
def test_cross_ring_call_on_loaded_streams(oracle_lib, name, mode, hazard):
    run_hazard(case(name, oracle_lib), mode, hazard)


@pytest.mark.parametrize("hazard", HAZARDS)
@pytest.mark.parametrize("name", NULL_CASES)
def test_cross_ring_call_with_the_work_ring_on_the_null_stream(oracle_lib, name, hazard):
    """alch_ring_set_stream(ring, 0) is the header's own example (torch's current stream unless the caller switched): the transforms a
    call queues "on the work ring's stream" on behalf of another ring must land on the null stream too, not on that other ring's own."""
    run_hazard(case(name, oracle_lib), "null", hazard)


@pytest.mark.parametrize("mode", ["ring", "caller"])
@pytest.mark.parametrize("name,hazard", SYNCED_RUNS)
def test_host_synchronised_cross_ring_call_behind_ballast(oracle_lib, name, hazard, mode):
    """The result is pinned, not the synchronisation: were these calls made asynchronous, the same cases would hold them to the order."""
    run_synced_hazard(case(name, oracle_lib), mode, hazard)


# ---- inside one ring: the lanes of alch_ct_mul_relin and of the fused alch_ct_mul_full ----------------------------------------------
RELIN_OPTS = [{"nstreams": 1}, {"nstreams": 2}, {"nstreams": 3}, {"nstreams": 4}, {"one_stream": 1}, {"pipe": 1, "nstreams": 1},
              {"pipe": 1, "nstreams": 2}]
_RELIN = {}


def relin_data(oracle_lib):
    """n = 2^11, four limbs, chunk = 8, batch 37 (five chunks, the last ragged): two operand sets and their oracle results."""
    if not _RELIN:
        qs, n, batch = primes_1_mod(1 << 12, 4, 1 << 30), 1 << 11, 37
        orc = oracle_lib.Ring(n, qs)
        rng = np.random.default_rng(37)
        hint = rand_elems(rng, 8, n, qs)
        sets = []
        for _ in range(2):
            a, b = rand_elems(rng, 2 * batch, n, qs), rand_elems(rng, 2 * batch, n, qs)
            want = []
            for ct in range(batch):
                want += list(orc.ct_mul_relin(list(hint), a[2 * ct], a[2 * ct + 1], b[2 * ct], b[2 * ct + 1]))
            w = np.stack(want)
            w.setflags(write=False)
            sets.append((a, b, w))
        _RELIN.update(qs=qs, n=n, batch=batch, hint=hint, sets=sets)
    return _RELIN


def relin_ring(d, opts, stream=None):
    r = A.Ring(2 * d["n"], d["qs"])
    r.set_option("chunk", 8)
    for k, v in opts.items():
        r.set_option(k, v)
    if stream is not None:
        r.set_stream(stream)
    return r


def differing(got, want):
    return [e for e in range(len(want)) if not np.array_equal(got[e], want[e])]


@pytest.mark.parametrize("opts", RELIN_OPTS, ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_mul_relin_lanes_read_operands_produced_behind_ballast(oracle_lib, opts):
    """RAW into every lane: the operands are copied into place behind ballast on the ring's stream; every lane the call forks must
    wait for them, and the download right after the call must see every lane joined."""
    d = relin_data(oracle_lib)
    r = relin_ring(d, opts)
    a, b, want = d["sets"][0]
    gh, ra, rb = r.hint_load(d["hint"]), r.upload(a), r.upload(b)
    ga, gb, out = r.alloc(len(a)), r.alloc(len(b)), r.alloc(len(want))
    for i, x in enumerate((ga, gb, out)):
        x.fill_uniform(5 + i)
    r.sync()
    ballast_on(r).push()
    ga.copy_from(ra, len(a)); gb.copy_from(rb, len(b))
    r.ct_mul_relin(gh, ga, gb, out, d["batch"])
    assert busy(r), "the ballast drained before the call returned: the case proved nothing"
    got = out.download()
    assert_reduced(got, d["qs"])
    assert not differing(got, want)


@pytest.mark.parametrize("opts", RELIN_OPTS, ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_mul_relin_two_calls_back_to_back_share_the_digit_scratch(oracle_lib, opts):
    """Two calls with different operands into different outputs, ballast before the first: the second call's tensor kernels must
    not overwrite the digit scratch the first call's key switches still read; the download right after the second call is the join."""
    d = relin_data(oracle_lib)
    r = relin_ring(d, opts)
    (a1, b1, w1), (a2, b2, w2) = d["sets"]
    gh = r.hint_load(d["hint"])
    g = [r.upload(x) for x in (a1, b1, a2, b2)]
    o1, o2 = r.alloc(len(w1)), r.alloc(len(w2))
    o1.fill_uniform(1); o2.fill_uniform(2)
    r.sync()
    ballast_on(r).push()
    r.ct_mul_relin(gh, g[0], g[1], o1, d["batch"])
    r.ct_mul_relin(gh, g[2], g[3], o2, d["batch"])
    assert busy(r), "the ballast drained before the calls returned: the case proved nothing"
    got2 = o2.download()
    got1 = o1.download()
    assert_reduced(got1, d["qs"]); assert_reduced(got2, d["qs"])
    assert not differing(got2, w2) and not differing(got1, w1)


_JOIN = {}


def join_data(oracle_lib):
    """256 more ciphertext pairs on the ring of relin_data and their oracle results (one oracle run for the module)."""
    if not _JOIN:
        d = relin_data(oracle_lib)
        orc = oracle_lib.Ring(d["n"], d["qs"])
        rng = np.random.default_rng(256)
        a, b = rand_elems(rng, 512, d["n"], d["qs"]), rand_elems(rng, 512, d["n"], d["qs"])
        want = np.stack([w for ct in range(256) for w in orc.ct_mul_relin(list(d["hint"]), a[2 * ct], a[2 * ct + 1], b[2 * ct], b[2 * ct + 1])])
        want.setflags(write=False)
        _JOIN.update(a=a, b=b, want=want)
    return _JOIN


@pytest.mark.parametrize("opts", [o for o in RELIN_OPTS if o.get("nstreams", 0) >= 2], ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_mul_relin_joins_every_lane_before_the_ring_stream_goes_on(oracle_lib, opts):
    """One full chunk of 64 ciphertexts per lane (batch = 64 lanes), each filling the GPU, and the output downloaded right after the call
    on the ring's stream, which must have joined every lane.  Not a certain detector: lane 0 is the ring's own stream and never holds
    less work than another lane, so without the join the download is wrong only when another lane happens to finish last."""
    d, j = relin_data(oracle_lib), join_data(oracle_lib)
    r = relin_ring(d, opts)
    r.set_option("chunk", 64)
    batch = 64 * opts["nstreams"]
    a, b, want = (j[k][:2 * batch] for k in ("a", "b", "want"))
    gh, ga, gb, out = r.hint_load(d["hint"]), r.upload(a), r.upload(b), r.alloc(2 * batch)
    out.fill_uniform(9)
    r.sync()
    ballast_on(r).push()
    r.ct_mul_relin(gh, ga, gb, out, batch)
    assert busy(r), "the ballast drained before the call returned: the case proved nothing"
    got = out.download()
    assert_reduced(got, d["qs"])
    assert not differing(got, want)


def test_mul_full_fused_two_calls_back_to_back(oracle_lib):
    """The same for the fused alch_ct_mul_full (fork and join over the hint ring's second stream): operands behind ballast on THEIR
    ring's stream, two calls back to back, the second output downloaded at once."""
    c = case("mul_full_fused", oracle_lib)
    dev = c.dev("ring")
    dev.sync()
    a, b = c.srcs
    ra, rb = dev.src_ring.upload(a), dev.src_ring.upload(b)
    ga, gb = dev.src_ring.alloc(len(a)), dev.src_ring.alloc(len(b))
    ga.fill_uniform(3); gb.fill_uniform(4)
    o1, o2 = dev.out_ring.alloc(len(c.want)), dev.out_ring.alloc(len(c.want))
    o1.fill_uniform(1); o2.fill_uniform(2)
    dev.sync()
    ballast_on(dev.work).push()
    dev.call([ra, rb], o1)
    dev.call([ra, rb], o2)
    assert busy(dev.work), "the ballast drained before the calls returned: the case proved nothing"
    check(o2.download(), c, dev)
    check(o1.download(), c, dev)
    dev.sync()
    ballast_on(dev.src_ring).push()
    ga.copy_from(ra, len(a)); gb.copy_from(rb, len(b))
    o1.fill_uniform(6)
    dev.call([ga, gb], o1)
    assert busy(dev.src_ring), "the ballast drained before the call returned: the case proved nothing"
    check(o1.download(), c, dev)


# ---- pooled buffers across rings -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ms_pow2_up", "embed_crt", "tunnel_pow2"])
def test_pooled_buffer_is_not_recycled_under_a_queued_consumer(oracle_lib, name):
    """x belongs to ring A; a call on ring B's loaded stream consumes it; x.free(); A.alloc of the same size returns the same device
    memory and garbage is written to it on A's stream at once: the consumer still read x."""
    c = case(name, oracle_lib)
    dev = c.dev("ring")
    assert dev.src_ring is not dev.work
    dev.sync()
    x = dev.src_ring.upload(c.srcs[0])
    out = dev.out_ring.alloc(len(c.want))
    out.fill_uniform(8)
    dev.sync()
    ptr = x.device_ptr()
    ballast_on(dev.work).push()
    dev.call([x], out)
    assert busy(dev.work), "the ballast drained before the call returned: the case proved nothing"
    x.free()
    y = dev.src_ring.alloc(len(c.srcs[0]))
    assert y.device_ptr() == ptr, "the pool handed out other memory: the case proved nothing"
    y.fill_uniform(13)
    check(out.download(), c, dev)
    dev.sync()


# ---- caller-owned streams ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", [{}, {"nstreams": 4}], ids=["default", "nstreams4"])
def test_mul_relin_on_the_null_stream(oracle_lib, opts):
    d = relin_data(oracle_lib)
    r = relin_ring(d, opts, stream=0)
    assert r.device_stream()[1] == 0
    a, b, want = d["sets"][1]
    gh, ra, rb = r.hint_load(d["hint"]), r.upload(a), r.upload(b)
    ga, gb, out = r.alloc(len(a)), r.alloc(len(b)), r.alloc(len(want))
    for i, x in enumerate((ga, gb, out)):
        x.fill_uniform(15 + i)
    r.sync()
    ballast_on(0).push()
    ga.copy_from(ra, len(a)); gb.copy_from(rb, len(b))
    r.ct_mul_relin(gh, ga, gb, out, d["batch"])
    assert busy(0), "the ballast drained before the call returned: the case proved nothing"
    got = out.download()
    assert_reduced(got, d["qs"])
    assert not differing(got, want)


def test_torch_reads_and_writes_in_stream_order_on_a_caller_owned_stream(oracle_lib):
    """A ring bound to a non-default torch stream s.  Under torch.cuda.stream(s): a clone of the as_torch view queued right after a
    library call behind ballast, without any synchronisation, equals a later download; and a torch write into the view followed by a
    library call is read by that call."""
    import torch
    d = relin_data(oracle_lib)
    s = torch.cuda.Stream()
    r = relin_ring(d, {}, stream=s.cuda_stream)
    o = oracle_lib.Ring(d["n"], d["qs"])
    x = d["sets"][0][0][:3]
    buf = r.upload(x)
    r.sync()
    with torch.cuda.stream(s):
        ballast_on(s).push()
        buf.crt()
        snap = buf.as_torch().clone()
        assert busy(s), "the ballast drained before the clone was queued: the case proved nothing"
    later = buf.download()
    assert np.array_equal(later, np.stack([o.crt(e) for e in x]))
    words = np.ascontiguousarray(later.transpose(0, 2, 1)).reshape(-1)               # limb-major device words
    assert np.array_equal(snap.cpu().numpy().astype(np.int64) & 0xFFFFFFFF, words)
    # the other direction: torch writes element 1's CRT words over element 0, the library transforms back
    per = d["n"] * len(d["qs"])
    with torch.cuda.stream(s):
        ballast_on(s).push()
        view = buf.as_torch()
        view[:per].copy_(view[per:2 * per])
        buf.crtinv(0, 1)
        assert busy(s), "the ballast drained before the call returned: the case proved nothing"
    got = buf.download(0, 1)
    assert_reduced(got, d["qs"])
    assert np.array_equal(got[0], x[1])


def test_stream_changes_lose_no_work_and_leave_the_callers_stream_alive(oracle_lib):
    """set_stream after work was queued on the ring's own stream loses none of it; a second ring takes the caller's stream over with
    share_stream; after both rings are destroyed the torch stream still runs a kernel and synchronises (the library has not destroyed
    a stream it does not own)."""
    import torch
    d = relin_data(oracle_lib)
    o = oracle_lib.Ring(d["n"], d["qs"])
    x = d["sets"][1][0][:4]
    r = relin_ring(d, {})
    buf = r.upload(x)
    r.sync()
    ballast_on(r).push()
    buf.crt()
    assert busy(r), "the ballast drained before the call returned: the case proved nothing"
    s = torch.cuda.Stream()
    r.set_stream(s.cuda_stream)                                  # behind the queued transform
    buf.crtinv(0, 2)                                             # on s
    got = buf.download()
    assert np.array_equal(got[:2], x[:2]) and np.array_equal(got[2:], np.stack([o.crt(e) for e in x[2:]]))
    r2 = relin_ring(d, {})
    r2.share_stream(r)
    assert r2.device_stream()[1] == s.cuda_stream
    b2 = r2.upload(x[:1])
    ballast_on(s).push()
    b2.crt()
    assert busy(s), "the ballast drained before the call returned: the case proved nothing"
    assert np.array_equal(b2.download()[0], o.crt(x[0]))
    b2.free(); buf.free()
    r.close(); r2.close()
    with torch.cuda.stream(s):
        t = torch.arange(1024, device="cuda") * 2
    s.synchronize()
    assert int(t.sum().item()) == 1023 * 1024
