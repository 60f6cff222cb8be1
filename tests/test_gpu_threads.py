"""GPU: the entry points are thread-safe (include/alchemy_hip.h: a call holds the lock of its ring's device until it returns).

A -threaded Haskell RTS forces tensors from any thread, and `GT` keeps one ring per (index, modulus list) for the whole process, so
calls on ONE ring arrive from several OS threads at once; a ring's scratch, pinned staging and buffer pool are plain members.  ctypes
releases the GIL during a call, so Python threads do overlap inside the library here.  Every thread checks its own results; without
the per-device lock the pinned staging of concurrent small transfers is the first thing to tear.

The host-buffer family (alch_crt, alch_mul, alch_l, alch_decompose_*, alch_hint_load, alch_embed_pow ...) is what that host calls
most: every one of them stages through the ring's ONE scratch element, which a larger request replaces, and the calls between two rings
share one cache of extension tables per ring.  The later tests drive those from eight threads that start together on a barrier; what
every call must return comes from the by-definition model (oracle/model_gen.py, oracle/model.py), computed on the main thread
before any worker runs.  A worker that is still alive 60 s after the start is a failure (a deadlock), not a hang of the suite."""
import threading
import time

import numpy as np
import pytest

import alchemy_amd as A
from alchemy_amd import capi
from helpers import primes_1_mod, primes_below, to_aos
from oracle import model as M
from oracle import model_gen as G
from oracle.model import is_prime

pytestmark = pytest.mark.gpu
QS = [1543651201, 689270401, 718099201]


def rand_elems(rng, count, n, qs):
    return np.stack([np.stack([rng.integers(0, q, size=n, dtype=np.int64) for q in qs], axis=1) for _ in range(count)])


def _hammer(ring, seed, rounds, errors):
    try:
        rng = np.random.default_rng(seed)
        for _ in range(rounds):
            x = rand_elems(rng, 1, ring.n, ring.qs)
            b = ring.upload(x)                                   # pinned staging of a small transfer
            c = ring.alloc(1)
            c.tensor_op(b, capi.ALCH_T_CRT)                      # pooled one-element buffers
            d = ring.alloc(1)
            d.tensor_op(c, capi.ALCH_T_CRTINV)
            if not np.array_equal(d.download(), x):
                errors.append(f"thread {seed}: crtInv(crt(x)) != x")
                return
            b.free(); c.free(); d.free()
    except Exception as e:                                       # noqa: BLE001 -- reported by the main thread
        errors.append(f"thread {seed}: {e!r}")


def test_one_ring_from_eight_threads():
    ring = A.Ring(11648, QS)
    errors = []
    threads = [threading.Thread(target=_hammer, args=(ring, 100 + t, 40, errors)) for t in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def test_two_rings_on_one_stream_from_four_threads():
    """Two rings that share a stream (what `GT` sets up) driven from four threads, with calls between the rings mixed in."""
    small, big = A.Ring(128 * 7, QS), A.Ring(11648, QS)
    small.share_stream(big)
    rng = np.random.default_rng(7)
    x = rand_elems(rng, 1, small.n, QS)
    want = small.embed_pow(big, x[0])
    errors = []

    def embedder(seed):
        try:
            for _ in range(30):
                bx = small.upload(x)
                out = big.alloc(1)
                out.embed_from(bx, 1, capi.ALCH_BASIS_POW)
                if not np.array_equal(out.download()[0], want):
                    errors.append(f"embedder {seed}: embedPow differs")
                    return
                bx.free(); out.free()
        except Exception as e:                                   # noqa: BLE001
            errors.append(f"embedder {seed}: {e!r}")

    threads = [threading.Thread(target=_hammer, args=(big, 200, 30, errors)), threading.Thread(target=_hammer, args=(small, 201, 30, errors)),
               threading.Thread(target=embedder, args=(1,)), threading.Thread(target=embedder, args=(2,))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


# ---------------------------------------------------------------------------------------------------------------------------------------
# the host-buffer family and the calls between two rings, eight threads at a time
# ---------------------------------------------------------------------------------------------------------------------------------------
N_THREADS = 8
JOIN_S = 60.0


def run_workers(workers):
    """Starts every worker(errors) on one barrier in a daemon thread of its own and waits at most JOIN_S seconds for all of them: a
    worker that is still alive then (a deadlock) fails the test instead of hanging the suite, and every mismatch a worker found, or the
    exception that ended it, is in the list that must be empty."""
    barrier, errors = threading.Barrier(len(workers)), []

    def body(k, work):
        try:
            barrier.wait(timeout=JOIN_S)
            work(errors)
        except Exception as e:                                   # noqa: BLE001 -- reported by the main thread
            errors.append(f"worker {k}: {e!r}")

    threads = [threading.Thread(target=body, args=(k, w), daemon=True) for k, w in enumerate(workers)]
    for t in threads:
        t.start()
    deadline = time.monotonic() + JOIN_S
    for t in threads:
        t.join(timeout=max(0.0, deadline - time.monotonic()))
    alive = [k for k, t in enumerate(threads) if t.is_alive()]
    assert not alive, f"workers {alive} are still running after {JOIN_S:.0f} s (deadlock?); errors so far: {errors}"
    assert not errors, errors


def limbs(a):
    """(n, L) host layout -> L lists of Python integers."""
    return np.asarray(a).T.tolist()


def per_limb(fn, x, qs):
    """fn(limb, q) on every limb of a host-layout element, back in host layout."""
    return to_aos([fn(v, q) for v, q in zip(limbs(x), qs)])


def reduced_digits(digits, qs):
    """The model's integer digits as the library returns them: every digit reduced into every limb, shape (D, n, L)."""
    return np.stack([to_aos([[d % q for d in dig] for q in qs]) for dig in digits])


def rand_elem(rng, n, qs):
    return np.ascontiguousarray(np.stack([rng.integers(0, q, size=n, dtype=np.int64) for q in qs], axis=1))


def host_menu(idx, qs, rng):
    """One input set of the host-buffer menu: [(name, call(ring) -> array, expected array)], every expected value by definition."""
    x, y = rand_elem(rng, idx.n, qs), rand_elem(rng, idx.n, qs)
    s = [int(rng.integers(1, q)) for q in qs]
    xl = limbs(x)
    cx = per_limb(lambda v, q: G.crt_def(v, idx, q), x, qs)
    cy = per_limb(lambda v, q: G.crt_def(v, idx, q), y, qs)
    g_pow = per_limb(lambda v, q: G.mulg_pow_def(v, idx, q), x, qs)
    g_dec = per_limb(lambda v, q: G.mulg_dec_def(v, idx, q), x, qs)
    g_crt = to_aos([[g * c % q for g, c in zip(G.g_crt(idx, q), v)] for v, q in zip(limbs(cx), qs)])
    w4 = capi.ALCH_GAD_BASEPOW2(4)
    return [
        ("crt", lambda r: r.crt(x), cx),
        ("crtinv", lambda r: r.crtinv(y), per_limb(lambda v, q: G.crtinv_def(v, idx, q), y, qs)),
        ("mul", lambda r: r.mul(cx, cy),
         to_aos([G.crt_def(G.ring_mul_def(a, b, idx, q), idx, q) for a, b, q in zip(xl, limbs(y), qs)])),
        ("add", lambda r: r.add(x, y), to_aos([[(a + b) % q for a, b in zip(u, v)] for u, v, q in zip(xl, limbs(y), qs)])),
        ("sub", lambda r: r.sub(x, y), to_aos([[(a - b) % q for a, b in zip(u, v)] for u, v, q in zip(xl, limbs(y), qs)])),
        ("scale", lambda r: r.scale(x, s), to_aos([[a * sj % q for a in v] for v, sj, q in zip(xl, s, qs)])),
        ("mulg_pow", lambda r: r.mulg_pow(x), g_pow),
        ("divg_pow", lambda r: r.divg_pow(g_pow), x),
        ("mulg_dec", lambda r: r.mulg_dec(x), g_dec),
        ("divg_dec", lambda r: r.divg_dec(g_dec), x),
        ("mulg_crt", lambda r: r.mulg_crt(cx), g_crt),
        ("divg_crt", lambda r: r.divg_crt(g_crt), cx),
        ("l", lambda r: r.l(x), per_limb(lambda v, q: G.l_def(v, idx, q), x, qs)),
        ("linv", lambda r: r.linv(x), per_limb(lambda v, q: G.linv_def(v, idx, q), x, qs)),
        ("decompose_triv", lambda r: np.stack(r.decompose_triv(x)), reduced_digits(M.decompose_triv(xl, qs), qs)),
        ("decompose_base2", lambda r: np.stack(r.decompose_baseb(x, capi.ALCH_GAD_BASE2)), reduced_digits(M.decompose_baseb(xl, qs, 2), qs)),
        ("decompose_base16", lambda r: np.stack(r.decompose_baseb(x, w4)), reduced_digits(M.decompose_baseb(xl, qs, 16), qs)),
    ]


HOST_RINGS = {"m45": lambda: (45, primes_1_mod(45, 2, 1 << 29), 4),
              "m64": lambda: (64, primes_1_mod(64, 2, 1 << 29), 4),
              "m45_word8": lambda: (45, primes_below(45, 2, 1 << 62), 8)}
HOST_ROUNDS = 12                                                 # 18 menu entries a round: 216 calls per thread


@pytest.mark.parametrize("name", sorted(HOST_RINGS))
def test_host_buffer_calls_on_one_ring_from_eight_threads(name):
    """Every host-buffer entry point on ONE ring from eight threads, each on inputs of its own, each starting the menu at another entry:
    at any moment the threads ask for scratch of 1, 2, 1 + L, 1 + D and 2D elements, so the scratch is replaced under calls that still
    use the old one unless each call holds the device lock from scratch_get to its download.  A hint loaded in a thread is checked by
    use: one mul_relin with it equals, word for word, the one with a hint the main thread loaded from the same host array
    (tests/test_gpu_golden.py pins that path to the oracle)."""
    m, qs, word = HOST_RINGS[name]()
    idx = G.Index(m)
    ring = A.Ring(m, qs)
    assert (ring.n, ring.word_bytes) == (idx.n, word)
    assert len({1, 2, 1 + ring.L, 1 + ring.gadget_digits(capi.ALCH_GAD_BASE2), 1 + ring.gadget_digits(capi.ALCH_GAD_BASEPOW2(4)),
                2 * ring.gadget_digits()}) == 6       # six scratch sizes on the menu
    rng = np.random.default_rng(4500 + m + word)
    cts = rand_elems(rng, 4, ring.n, qs)
    ga, gb = ring.upload(cts[:2]), ring.upload(cts[2:])          # the one fixed ciphertext pair, read by every thread's mul_relin

    def relin(hint_host):
        hint, out = ring.hint_load(hint_host), ring.alloc(2)
        ring.ct_mul_relin(hint, ga, gb, out, 1)
        got = out.download()
        out.free(); hint.free()
        return got

    menus, hints = [], []
    for t in range(N_THREADS):
        menus.append([host_menu(idx, qs, rng) for _ in range(2)])
        hint_host = rand_elems(rng, 2 * ring.L, ring.n, qs)
        hints.append((hint_host, relin(hint_host)))

    def worker(t):
        def work(errors):
            sets, (hint_host, want_relin) = menus[t], hints[t]
            entries = len(sets[0]) + 1                           # + hint_load
            calls = 0
            for rnd in range(HOST_ROUNDS):
                menu = sets[rnd % 2]
                for k in range(entries):
                    e = (t + k) % entries
                    if e == len(menu):
                        what, got, want = "hint_load", relin(hint_host), want_relin
                    else:
                        what, call, want = menu[e]
                        got = call(ring)
                    calls += 1
                    if got is None or not np.array_equal(np.asarray(got), want):
                        errors.append(f"thread {t} round {rnd}: {what} differs from the model")
                        return
            assert calls >= 200
        return work

    run_workers([worker(t) for t in range(N_THREADS)])
    ga.free(); gb.free()


def prime_1_mod(m, start):
    """The modulus rule of tests/test_tensor_ext.py."""
    q = start - start % m + 1
    while not is_prime(q):
        q += m
    return q


EXT_ROUNDS = 30


@pytest.mark.parametrize("m,mb", [(12, 60), (32, 96)])
def test_first_use_of_extension_tables_from_threads(m, mb):
    """Two fresh rings and no call between them before the barrier: every thread's first call needs the pair's extension tables, which
    ext_tables builds on first use and caches in the big ring.  Six threads take one host form each, two run the resident forms on
    buffers of their own; every result against the model."""
    s, b = G.Index(m), G.Index(mb)
    qs = [prime_1_mod(mb, 1 << 29), prime_1_mod(mb, 1 << 30)]
    rs, rb = A.Ring(m, qs), A.Ring(mb, qs)
    rng = np.random.default_rng(m * 97 + mb)
    rows = len(G.coeffs_indices(s, b))

    def coeffs_want(y):
        per = [G.coeffs(v, s, b) for v in limbs(y)]                                  # [limb][row][k]
        return np.stack([to_aos([per[j][i] for j in range(len(qs))]) for i in range(rows)])

    def host_case(kind):
        x, y = rand_elem(rng, s.n, qs), rand_elem(rng, b.n, qs)
        return {"embed_pow": (lambda: rs.embed_pow(rb, x), per_limb(lambda v, q: G.embed_pow(v, s, b), x, qs)),
                "embed_dec": (lambda: rs.embed_dec(rb, x), per_limb(lambda v, q: G.embed_dec_def(v, s, b, q), x, qs)),
                "embed_crt": (lambda: rs.embed_crt(rb, x), per_limb(lambda v, q: G.embed_crt_def(v, s, b), x, qs)),
                "twace_pow_dec": (lambda: rs.twace_pow_dec(rb, y), per_limb(lambda v, q: G.twace_pow_dec(v, s, b), y, qs)),
                "twace_crt": (lambda: rs.twace_crt(rb, y), per_limb(lambda v, q: G.twace_crt_def(v, s, b, q), y, qs)),
                "coeffs": (lambda: rs.coeffs(rb, y), coeffs_want(y))}[kind]

    def resident_case(first):
        """embed_from then twace_from (first = 'embed'), or coeffs_from then twace_from on the CRT basis, on this thread's buffers."""
        x, y = rand_elem(rng, s.n, qs), rand_elem(rng, b.n, qs)
        bx, by = rs.upload(x[None]), rb.upload(y[None])                              # uploads are no extension calls
        big, small, cbuf = rb.alloc(1), rs.alloc(1), rs.alloc(rows)
        if first == "embed":
            steps = [("embed_from", lambda: (big.embed_from(bx, 1, capi.ALCH_BASIS_POW), big.download()[0])[1],
                      per_limb(lambda v, q: G.embed_pow(v, s, b), x, qs)),
                     ("twace_from", lambda: (small.twace_from(by, 1, capi.ALCH_BASIS_POW), small.download()[0])[1],
                      per_limb(lambda v, q: G.twace_pow_dec(v, s, b), y, qs))]
        else:
            steps = [("coeffs_from", lambda: (cbuf.coeffs_from(by, 1), cbuf.download())[1], coeffs_want(y)),
                     ("twace_from crt", lambda: (small.twace_from(by, 1, capi.ALCH_BASIS_CRT), small.download()[0])[1],
                      per_limb(lambda v, q: G.twace_crt_def(v, s, b, q), y, qs))]
        return steps

    plans = [[(k,) + host_case(k)] for k in ("embed_pow", "embed_dec", "embed_crt", "twace_pow_dec", "twace_crt", "coeffs")]
    plans += [resident_case("embed"), resident_case("coeffs")]
    assert len(plans) == N_THREADS

    def worker(t):
        def work(errors):
            for rnd in range(EXT_ROUNDS):
                for what, call, want in plans[t]:
                    if not np.array_equal(np.asarray(call()), want):
                        errors.append(f"thread {t} round {rnd}: {what} differs from the model")
                        return
        return work

    run_workers([worker(t) for t in range(N_THREADS)])


def test_host_calls_race_the_resident_dec_embed_that_borrows_their_scratch():
    """alch_buf_embed on the decoding basis converts a copy of its source in the SMALL ring's scratch element -- the one alch_crt,
    alch_l and alch_decompose_triv on that ring stage through.  Four threads of each, on one shared stream."""
    m, mb, count = 12, 60, 3
    s, b = G.Index(m), G.Index(mb)
    qs = [prime_1_mod(mb, 1 << 29), prime_1_mod(mb, 1 << 30)]
    small, big = A.Ring(m, qs), A.Ring(mb, qs)
    small.share_stream(big)
    rng = np.random.default_rng(1260)

    def host_plan():
        x = rand_elem(rng, s.n, qs)
        return [("crt", lambda: small.crt(x), per_limb(lambda v, q: G.crt_def(v, s, q), x, qs)),
                ("l", lambda: small.l(x), per_limb(lambda v, q: G.l_def(v, s, q), x, qs)),
                ("decompose_triv", lambda: np.stack(small.decompose_triv(x)), reduced_digits(M.decompose_triv(limbs(x), qs), qs))]

    def embed_plan():
        xs = rand_elems(rng, count, s.n, qs)
        src, dst = small.upload(xs), big.alloc(count)
        want = np.stack([per_limb(lambda v, q: G.embed_dec_def(v, s, b, q), x, qs) for x in xs])
        return [("embed_from dec", lambda: (dst.embed_from(src, count, capi.ALCH_BASIS_DEC), dst.download())[1], want)]

    plans = [host_plan() for _ in range(4)] + [embed_plan() for _ in range(4)]

    def worker(t):
        def work(errors):
            for rnd in range(EXT_ROUNDS):
                for what, call, want in plans[t]:
                    if not np.array_equal(np.asarray(call()), want):
                        errors.append(f"thread {t} round {rnd}: {what} differs from the model")
                        return
        return work

    run_workers([worker(t) for t in range(N_THREADS)])
