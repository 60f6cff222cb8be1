"""GPU: which operand ranges of one call may share memory (include/alchemy_hip.h, "Overlapping ranges"; DESIGN.md, "Overlap rules").

Every entry point that takes two or more ranges of one ring either refuses a byte overlap between the range it writes and a range it
reads (ALCH_E_INVALID, the function's name in alch_last_error, nothing launched) or accepts the one overlap that is safe: the written
range STARTING where the operand starts, where each lane reads the words it writes before it writes them.  The operands of a case are
views (alch_buf_view) of one parent buffer of a handful of elements (helpers.carve), so "touching" means adjacent views of one
allocation -- the legitimate case -- and "overlapping by one element" the smallest refused one.

Rings, at the smallest shapes that reach each dispatch branch; every case asserts the word size:
  P32x2  index 32 (n = 16), the two largest primes below 2^31         4-byte words, 16-byte packs, radix-16 engine
  P32w8  index 32, the largest prime below 2^62                       8-byte words
  G9     index 9 (n = 6), two primes below 2^31                       general engine, n % 4 != 0: the one-word (VW = 1 / _scalar) forms
  P32x3 / P32x1 / Z4   three limbs (a digit range with a middle), one 31-bit limb (a lift into the same ring), Z_4 without CRT (alch_pt_*)
Operands: uniform words, never all zero.  Every comparison is bit for bit or a status; there is no tolerance.

   1. test_elementwise                 alch_buf_mul / _add / _sub (either operand and both), alch_buf_scale, dst / src of alch_buf_mul_public
                                       and alch_ct_add_public: coincide (same handle, and a second view), touch on either side,
                                       overlap by one element on either side
   2. test_public_element              pub[pub_index] of alch_buf_mul_public, alch_ct_add_public, alch_buf_add_public in the first, a
                                       middle (an odd element: a c1 component) and the last element of the written range, just before and
                                       just after it, and inside src
   3. test_decompose_source            element src_index of alch_buf_decompose_triv against the L digits, L = 3, 2, 1
   4. test_mul_relin                   alch_ct_mul_relin, batch 2: out a view of a, out shifted into b, out touching a / b, a == b,
                                       one refusal with ALCH_POW_IN | ALCH_POW_OUT (the check runs before the workspace staging)
   5. test_hint_from_buf_copies, test_tunnel_create_copies     alch_hint_from_buf and alch_tunnel_create (64 -> 32) copy their sources
   6. test_between_index_methods_on_one_ring, test_tunnel_to_itself, test_mul_full_on_one_suffix_ring
                                       the cross-ring entry points where one ring can serve as both: alch_buf_embed / _twace / _coeffs with
                                       equal indices, alch_ct_tunnel from a ring to itself, alch_ct_mul_full with operands and result on
                                       one suffix ring (both gadgets)
   7. test_ct_mul, test_key_switch_quad, test_ct_add     3 * batch against 2 * batch, both ways round; alch_ct_add of a linear and
                                       a quadratic operand (out may start where the quadratic one starts only)
   8. test_error_term, test_decrypt_lift         degree 1 and 2; the secret-key element counts as an operand
   9. test_buf_lift, test_pt_rescale, test_pt_eval_lin, test_tensor_op_and_copy, test_add_bcast_and_pt_mul
                                       the touch and one-element rows the entry points that already checked lacked

References: Python integers from the uploaded words (1, 2, 7 and the copies); the C restatement for the TrivGad digits and for
alch_ct_mul_relin (oracle_lib, as tests/test_gpu_parity.py and tests/test_gpu_general_index.py); for the composed entry points of 6, 8
and 9, whose arithmetic other files pin against the model, the same call into a separate buffer -- what an overlap could change is
which words a lane sees, and the separate buffer is the run where it sees the uploaded ones."""
import functools

import numpy as np
import pytest

from helpers import assert_parent_unchanged, assert_reduced, carve, primes_below

pytestmark = pytest.mark.gpu

RING_DEFS = {"P32x2": (32, 2, 1 << 31, 4), "P32w8": (32, 1, 1 << 62, 8), "G9": (9, 2, 1 << 31, 4),
             "P32x3": (32, 3, 1 << 31, 4), "P32x1": (32, 1, 1 << 31, 4), "P64x2": (64, 2, 1 << 31, 4)}
MAIN = ["P32x2", "P32w8", "G9"]
P_PLAIN = 4


@functools.lru_cache(maxsize=None)
def ring_of(name):
    """(ring, moduli): created once per module; asserts the index's dimension and the word size."""
    import alchemy_amd as A
    m, L, hi, word = RING_DEFS[name]
    qs = primes_below(m, L, hi)
    ring = A.Ring(m, qs)
    assert ring.word_bytes == word and ring.L == L, name
    assert ring.n == {32: 16, 9: 6, 64: 32}[m]
    if name == "G9":
        assert ring.n % 4 != 0                                               # 4-byte words: ALCH_LAUNCH_VW picks VW = 1, k_pointwise_scalar
    return ring, qs


@functools.lru_cache(maxsize=None)
def plain_ring():
    import alchemy_amd as A
    return A.Ring(32, [P_PLAIN], nocrt=True)


def words(seed, count, n, qs):
    """(count, n, L) uniform residues; no element is zero everywhere."""
    rng = np.random.default_rng(seed)
    x = np.ascontiguousarray(np.stack([rng.integers(0, q, size=(count, n), dtype=np.int64) for q in qs], axis=2))
    assert all(e.any() for e in x)
    return x


def ints(a):
    return np.asarray(a).astype(object)


def i64(a):
    return np.ascontiguousarray(np.asarray(a).astype(np.int64))


def qvec(qs):
    return np.array([int(q) for q in qs], dtype=object)


def accepted(ring, host, spans, call, written, want, what):
    """The call runs on views of one parent; the written span equals `want`, every other word of the parent is as uploaded."""
    parent, views = carve(ring, host, *spans)
    call(*views, parent)
    got = assert_parent_unchanged(parent, host, [written])
    assert np.array_equal(got[written[0]:written[0] + written[1]], want), what
    return got


def refused(ring, host, spans, call, name, what):
    """ALCH_E_INVALID, alch_last_error names the function, every word of the parent is as uploaded."""
    from alchemy_amd import capi
    parent, views = carve(ring, host, *spans)
    with pytest.raises(capi.AlchemyError) as err:
        call(*views, parent)
    assert err.value.code == capi.ALCH_E_INVALID, (what, str(err.value))
    assert name + ":" in str(err.value), (what, str(err.value))
    assert_parent_unchanged(parent, host)


# ---- 1. element-wise calls: the written range against one operand range ----------------------------------------------------------------
def half(qs):
    return [(q + 1) // 2 for q in qs]


# name -> (function named in the refusal, run(dst, x, y, qs), reference(X, Y, q) on Python integers); x is the operand whose range
# moves against dst, y a second operand elsewhere in the parent (for the public-element calls its element 0 is the public element)
EW_OPS = {
    "mul_a": ("alch_buf_mul", lambda d, x, y, qs: d.mul(x, y, 2), lambda X, Y, q: X * Y % q),
    "mul_b": ("alch_buf_mul", lambda d, x, y, qs: d.mul(y, x, 2), lambda X, Y, q: X * Y % q),
    "mul_ab": ("alch_buf_mul", lambda d, x, y, qs: d.mul(x, x, 2), lambda X, Y, q: X * X % q),
    "add_a": ("alch_buf_add", lambda d, x, y, qs: d.add(x, y, 2), lambda X, Y, q: (X + Y) % q),
    "add_b": ("alch_buf_add", lambda d, x, y, qs: d.add(y, x, 2), lambda X, Y, q: (X + Y) % q),
    "sub_a": ("alch_buf_sub", lambda d, x, y, qs: d.sub(x, y, 2), lambda X, Y, q: (X - Y) % q),
    "sub_b": ("alch_buf_sub", lambda d, x, y, qs: d.sub(y, x, 2), lambda X, Y, q: (Y - X) % q),
    "scale": ("alch_buf_scale", lambda d, x, y, qs: d.scale(x, 2, half(qs)), lambda X, Y, q: X * qvec(half(q)) % q),
    "mul_public": ("alch_buf_mul_public", lambda d, x, y, qs: d.mul_public(x, y, 0, 2), lambda X, Y, q: X * Y[0] % q),
    "ct_add_public": ("alch_ct_add_public", lambda d, x, y, qs: d.ct_add_public(x, 1, half(qs), y, 0),
                      lambda X, Y, q: np.stack([(X[0] * qvec(half(q)) + Y[0]) % q, X[1] * qvec(half(q)) % q])),
}
X_SPAN, Y_SPAN = (2, 2), (6, 2)
# dst against x = elements [2, 4): the same range, the two adjacent ones, the two that share one element
EW_ROWS = [("coincide", (2, 2), True), ("touch-after", (4, 2), True), ("touch-before", (0, 2), True),
           ("overlap-last", (3, 2), False), ("overlap-first", (1, 2), False)]


@pytest.mark.parametrize("op", list(EW_OPS))
@pytest.mark.parametrize("name", MAIN)
def test_elementwise(name, op):
    """dst against one operand of an element-wise call, count = 2, in a parent of 8 elements.  Coinciding (through the operand's own
    handle and through a second view of the same range) and touching on either side: accepted, equal to Python integers and to the
    call into a separate buffer, the rest of the parent untouched.  Sharing one element on either side: refused, parent untouched."""
    ring, qs = ring_of(name)
    fn, run, ref = EW_OPS[op]
    host = words(1000 + len(op) + ring.n, 8, ring.n, qs)
    q = qvec(qs)
    want = i64(ref(ints(host[2:4]), ints(host[6:8]), q))
    assert_reduced(want, qs)
    # the call into a separate buffer
    parent, (x, y) = carve(ring, host, X_SPAN, Y_SPAN)
    out = ring.alloc(2)
    run(out, x, y, qs)
    assert np.array_equal(out.download(), want), (op, "separate buffer")
    assert_parent_unchanged(parent, host)
    # through the operand's own handle
    parent, (x, y) = carve(ring, host, X_SPAN, Y_SPAN)
    run(x, x, y, qs)
    got = assert_parent_unchanged(parent, host, [X_SPAN])
    assert np.array_equal(got[2:4], want), (op, "same handle")
    for row, dspan, ok in EW_ROWS:
        call = lambda x, y, d, parent: run(d, x, y, qs)
        if ok:
            accepted(ring, host, [X_SPAN, Y_SPAN, dspan], call, dspan, want, (op, row))
        else:
            refused(ring, host, [X_SPAN, Y_SPAN, dspan], call, fn, (op, row))


# ---- 2. the public element ----------------------------------------------------------------------------------------------------------------
def _mul_public(ring, qs, host, p):
    return (lambda d, s, parent: d.mul_public(s, parent, p, 3)), (3, 3), (8, 3), \
        i64(ints(host[8:11]) * ints(host[p]) % qvec(qs))


def _ct_add_public(ring, qs, host, p):
    s, q = qvec(half(qs)), qvec(qs)
    want = ints(host[8:12]) * s % q
    want[0::2] = (want[0::2] + ints(host[p])) % q
    return (lambda d, src, parent: d.ct_add_public(src, 2, half(qs), parent, p)), (3, 4), (8, 4), i64(want)


def _add_public(ring, qs, host, p):
    want = ints(host[3:7])
    want[0::2] = (want[0::2] + ints(host[p])) % qvec(qs)
    return (lambda d, src, parent: d.add_public(parent, p, 2)), (3, 4), (8, 4), i64(want)


PUBLIC = {"alch_buf_mul_public": (_mul_public, (3, 4, 5), (2, 6, 9)), "alch_ct_add_public": (_ct_add_public, (3, 4, 6), (2, 7, 9)),
          "alch_buf_add_public": (_add_public, (3, 4, 6), (2, 7))}


@pytest.mark.parametrize("fn", list(PUBLIC))
@pytest.mark.parametrize("name", MAIN)
def test_public_element(name, fn):
    """The one element every lane reads, given as (parent, index): inside the written range -- its first element, a middle one (for
    the ciphertext calls the odd element 4, a c1 component, which alch_buf_add_public does not even write: the header refuses the
    whole 2 * batch range) and its last -- refused; in the element just before and just after it, and inside src: accepted, exact."""
    ring, qs = ring_of(name)
    build, inside, outside = PUBLIC[fn]
    host = words(2000 + len(fn) + ring.n, 12, ring.n, qs)
    for p in inside + outside:
        call, dspan, sspan, want = build(ring, qs, host, p)
        if p in inside:
            refused(ring, host, [dspan, sspan], call, fn, (fn, p))
        else:
            assert_reduced(want, qs)
            accepted(ring, host, [dspan, sspan], call, dspan, want, (fn, p))


# ---- 3. alch_buf_decompose_triv --------------------------------------------------------------------------------------------------------------
def oracle_ring(oracle_lib, name):
    m, _, _, _ = RING_DEFS[name]
    qs = ring_of(name)[1]
    return oracle_lib.GenRing(m, qs) if name == "G9" else oracle_lib.Ring(m // 2, qs)


@pytest.mark.parametrize("name", ["P32x3", "P32w8", "G9"])
def test_decompose_source(oracle_lib, name):
    """Digits into elements [2, 2 + L) of the parent, the source element given by index into the same parent: inside the digits (first,
    middle where L = 3, last) refused; element 1 and element 2 + L accepted, equal to the C restatement's digits."""
    ring, qs = ring_of(name)
    L, o = ring.L, oracle_ring(oracle_lib, name)
    host = words(3000 + ring.n + L, L + 4, ring.n, qs)
    for src in range(1, 2 + L + 1):
        call = lambda parent: parent.decompose_triv_into(src, parent, 2)
        if 2 <= src < 2 + L:
            refused(ring, host, [], call, "alch_buf_decompose_triv", src)
        else:
            want = np.stack(o.decompose_triv(host[src]))
            assert_reduced(want, qs)
            accepted(ring, host, [], call, (2, L), want, src)


# ---- 4. alch_ct_mul_relin ------------------------------------------------------------------------------------------------------------------
def relin_want(o, hint, a, b, batch):
    out = []
    for ct in range(batch):
        out += list(o.ct_mul_relin(list(hint), a[2 * ct], a[2 * ct + 1], b[2 * ct], b[2 * ct + 1]))
    return np.stack(out)


@pytest.mark.parametrize("name", ["P32x2", "G9"])
def test_mul_relin(oracle_lib, name):
    """Batch 2: a, b and out are views of 4 elements in a parent of 12.  out touching b (after it) and touching a (before it), and
    a == b: accepted, equal to the C restatement.  out a view of a, out shifted by one element into b (from either side), and the same
    with ALCH_POW_IN | ALCH_POW_OUT, which stages the operands through the workspace: refused before anything runs."""
    from alchemy_amd import capi
    ring, qs = ring_of(name)
    o = oracle_ring(oracle_lib, name)
    hint_host = words(4000 + ring.n, 2 * ring.L, ring.n, qs)
    hint = ring.hint_load(hint_host)
    host = words(4100 + ring.n, 12, ring.n, qs)
    run = lambda flags=0: (lambda a, b, out, parent: ring.ct_mul_relin(hint, a, b, out, 2, flags=flags))
    for a, b, out in (((0, 4), (4, 4), (8, 4)), ((4, 4), (8, 4), (0, 4)), ((4, 4), (4, 4), (8, 4)), ((4, 4), (4, 4), (0, 4))):
        want = relin_want(o, hint_host, host[a[0]:a[0] + 4], host[b[0]:b[0] + 4], 2)
        accepted(ring, host, [a, b, out], run(), out, want, (a, b, out))
    both = capi.ALCH_POW_IN | capi.ALCH_POW_OUT
    for a, b, out, flags in (((0, 4), (4, 4), (0, 4), 0), ((0, 4), (4, 4), (5, 4), 0), ((0, 4), (5, 4), (2, 4), 0),
                             ((4, 4), (4, 4), (1, 4), 0), ((0, 4), (4, 4), (7, 4), both), ((0, 4), (4, 4), (0, 4), both)):
        refused(ring, host, [a, b, out], run(flags), "alch_ct_mul_relin", (a, b, out, flags))


# ---- 5. the entry points that copy their sources ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["P32x2", "G9"])
def test_hint_from_buf_copies(name):
    """alch_hint_from_buf, then fill_uniform over the source: alch_ct_mul_relin gives the words it gave with the source untouched."""
    ring, qs = ring_of(name)
    src = ring.upload(words(5000 + ring.n, 2 * ring.L, ring.n, qs))
    a, b = ring.upload(words(5001, 4, ring.n, qs)), ring.upload(words(5002, 4, ring.n, qs))
    hint = ring.hint_from_buf(src)
    first, second = ring.alloc(4), ring.alloc(4)
    ring.ct_mul_relin(hint, a, b, first, 2)
    before = src.download()
    src.fill_uniform(77)
    assert not np.array_equal(src.download(), before)
    ring.ct_mul_relin(hint, a, b, second, 2)
    assert np.array_equal(first.download(), second.download())


def test_tunnel_create_copies():
    """alch_tunnel_create on 64 -> 32: lin_crt and ks_crt overwritten after creation, the tunnel gives the same words."""
    from alchemy_amd import capi
    rr, qs = ring_of("P64x2")
    import alchemy_amd as A
    rs = A.Ring(32, qs)
    assert rs.word_bytes == 4
    _, d_rel = capi.Tunnel.info(rr, rs)
    assert d_rel == 2
    lin, ks = rs.upload(words(5100, d_rel, rs.n, qs)), rs.upload(words(5101, 2 * d_rel * rs.L, rs.n, qs))
    tun = capi.Tunnel(rr, rs, lin, ks)
    cts = rr.upload(words(5102, 4, rr.n, qs))
    first, second = rs.alloc(4), rs.alloc(4)
    tun.apply(cts, first, 2)
    before = lin.download(), ks.download()
    lin.fill_uniform(78)
    ks.fill_uniform(79)
    assert not np.array_equal(lin.download(), before[0]) and not np.array_equal(ks.download(), before[1])
    tun.apply(cts, second, 2)
    assert np.array_equal(first.download(), second.download())
    assert first.download().any()


# ---- 6. cross-ring entry points with one ring on both sides -----------------------------------------------------------------------------------
def separate_run(ring, host, spans, call, out_elems):
    """The call with its output in a buffer of its own: the reference of the composed entry points."""
    parent, views = carve(ring, host, *spans)
    out = ring.alloc(out_elems)
    call(*views, out)
    assert_parent_unchanged(parent, host)
    return out.download()


def overlap_rows(ring, host, in_span, out_count, call, fn, coincide_ok=False, extra=()):
    """The rows of an entry point that reads in_span and writes out_count elements: out coinciding with the start of in (refused unless
    coincide_ok), out ending where in begins and beginning where in ends (accepted, equal to the separate run), out sharing in's first
    and in's last element only (refused).  call(in_view, *extra_views, out_view); the parent holds out_count free elements on both
    sides of in."""
    first, count = in_span
    assert first >= out_count and first + count + out_count <= len(host)
    spans = [in_span] + list(extra)
    want = separate_run(ring, host, spans, call, out_count)
    assert want.any()
    wrapped = lambda *views: call(*views[:-1])
    for row, ofirst, ok in (("coincide", first, coincide_ok), ("touch-before", first - out_count, True), ("touch-after", first + count, True),
                            ("overlap-first", first - out_count + 1, False), ("overlap-last", first + count - 1, False)):
        ospan = (ofirst, out_count)
        if ok:
            accepted(ring, host, spans + [ospan], wrapped, ospan, want, (fn, row))
        else:
            refused(ring, host, spans + [ospan], wrapped, fn, (fn, row))


@pytest.mark.parametrize("name", ["P32x2", "G9"])
def test_between_index_methods_on_one_ring(name):
    """alch_buf_embed, alch_buf_twace and alch_buf_coeffs with equal indices (every table is the identity, d_rel = 1): dst a view into
    src is refused whole; adjacent views are accepted and hold src's words."""
    from alchemy_amd import capi
    ring, qs = ring_of(name)
    host = words(6000 + ring.n, 8, ring.n, qs)
    for fn, call in (("alch_buf_embed", lambda s, d: d.embed_from(s, 2, capi.ALCH_BASIS_POW)),
                     ("alch_buf_twace", lambda s, d: d.twace_from(s, 2, capi.ALCH_BASIS_POW)),
                     ("alch_buf_coeffs", lambda s, d: d.coeffs_from(s, 2))):
        assert np.array_equal(separate_run(ring, host, [(3, 2)], call, 2), host[3:5]), fn
        overlap_rows(ring, host, (3, 2), 2, call, fn)


def test_tunnel_to_itself():
    """alch_ct_tunnel through a tunnel from the index-32 ring to itself (d_rel = 1: the key switch alone), batch 2."""
    from alchemy_amd import capi
    ring, qs = ring_of("P32x2")
    assert capi.Tunnel.info(ring, ring) == (32, 1)
    tun = capi.Tunnel(ring, ring, ring.upload(words(6100, 1, ring.n, qs)), ring.upload(words(6101, 2 * ring.L, ring.n, qs)))
    host = words(6102, 12, ring.n, qs)
    overlap_rows(ring, host, (4, 4), 4, lambda i, o: tun.apply(i, o, 2), "alch_ct_tunnel")


@pytest.mark.parametrize("gadget", ["triv", "base2"])
def test_mul_full_on_one_suffix_ring(gadget):
    """alch_ct_mul_full with the hint on three limbs and operands and result on ONE ring of the last two, batch 2.  TrivGad: out against
    a and against b, every row.  BaseBGad 2 (its own entry path): out a view of b and out shifted into a, refused."""
    import alchemy_amd as A
    from alchemy_amd import capi
    rh, qh = ring_of("P32x3")
    rs = A.Ring(32, qh[1:])
    assert rs.word_bytes == 4 and rs.L == 2
    g = capi.ALCH_GAD_TRIV if gadget == "triv" else capi.ALCH_GAD_BASE2
    hint = rh.hint_load(words(6200, 2 * rh.gadget_digits(g), rh.n, qh), g)
    host = words(6201, 16, rs.n, qh[1:])
    if gadget == "triv":
        overlap_rows(rs, host, (4, 4), 4, lambda a, b, o: capi.ct_mul_full(hint, a, b, o, 2), "alch_ct_mul_full", extra=[(12, 4)])
        overlap_rows(rs, host, (4, 4), 4, lambda b, a, o: capi.ct_mul_full(hint, a, b, o, 2), "alch_ct_mul_full", extra=[(12, 4)])
    else:
        call = lambda a, b, o, parent: capi.ct_mul_full(hint, a, b, o, 2)
        refused(rs, host, [(0, 4), (4, 4), (4, 4)], call, "alch_ct_mul_full", "out = b")
        refused(rs, host, [(4, 4), (8, 4), (1, 4)], call, "alch_ct_mul_full", "out shifted into a")


# ---- 7. alch_ct_mul, alch_ct_key_switch_quad: 3 * batch against 2 * batch -----------------------------------------------------------------------
def test_ct_mul():
    """out = 3 * batch elements, operands 2 * batch, batch 2, index 32 (g = 1): the tensor product in Python integers.  out touching an
    operand on either side accepted; out's last element on the operand's first, and out's first on the operand's last, refused -- for a
    and for b.  (A 2 * batch in place of the 3 * batch lets the first of the refused rows through.)"""
    from alchemy_amd.mulsteps import ct_mul
    ring, qs = ring_of("P32x2")
    host = words(7000, 20, ring.n, qs)
    q = qvec(qs)

    def want(a, b):
        A, B = ints(host[a:a + 4]), ints(host[b:b + 4])
        out = []
        for ct in range(2):
            a0, a1, b0, b1 = A[2 * ct], A[2 * ct + 1], B[2 * ct], B[2 * ct + 1]
            out += [a0 * b0 % q, (a0 * b1 + a1 * b0) % q, a1 * b1 % q]
        return i64(np.stack(out))

    for swap in (False, True):
        call = (lambda y, x, o, parent: ct_mul(x, y, 2, out=o)) if swap else (lambda x, y, o, parent: ct_mul(x, y, 2, out=o))
        ref = (lambda x, y: want(y, x)) if swap else want
        # x = [6, 10) moves against out, y = [16, 20) stays clear
        for ofirst, ok in ((0, True), (10, True), (1, False), (9, False), (6, False)):
            if ok:
                accepted(ring, host, [(6, 4), (16, 4), (ofirst, 6)], call, (ofirst, 6), ref(6, 16), (swap, ofirst))
            else:
                refused(ring, host, [(6, 4), (16, 4), (ofirst, 6)], call, "alch_ct_mul", (swap, ofirst))


def test_key_switch_quad():
    """in = 3 * batch elements, out = 2 * batch, batch 2: out touching in on either side accepted and equal to the separate run; one
    shared element on either side, and out on in's start, refused."""
    from alchemy_amd.mulsteps import key_switch_quad
    ring, qs = ring_of("P32x2")
    hint = ring.hint_load(words(7100, 2 * ring.L, ring.n, qs))
    host = words(7101, 14, ring.n, qs)
    overlap_rows(ring, host, (4, 6), 4, lambda i, o: key_switch_quad(hint, i, 2, out=o), "alch_ct_key_switch_quad")


def test_ct_add():
    """alch_ct_add of a linear a (2 * batch elements) and a quadratic b (3 * batch), batch 2, no scalars: out (3 * batch) may start
    where b starts but not where a starts (a has not the result's degree); touching either is accepted and equal to the sum in Python
    integers, one shared element refused."""
    from alchemy_amd.ctadd import ct_add_raw
    ring, qs = ring_of("P32x2")
    host = words(7200, 24, ring.n, qs)
    q = qvec(qs)
    A, B = ints(host[6:10]).reshape(2, 2, ring.n, ring.L), ints(host[6:12]).reshape(2, 3, ring.n, ring.L)
    far_a, far_b = ints(host[20:24]).reshape(2, 2, ring.n, ring.L), ints(host[18:24]).reshape(2, 3, ring.n, ring.L)

    def total(a, b):
        out = b.copy()
        out[:, :2] = (out[:, :2] + a) % q
        return i64(out.reshape(6, ring.n, ring.L))

    add_a = lambda a, b, o: ct_add_raw(o, 2, a, 1, None, 0, b, 2, None, 0)
    assert np.array_equal(separate_run(ring, host, [(6, 4), (18, 6)], add_a, 6), total(A, far_b))
    overlap_rows(ring, host, (6, 4), 6, add_a, "alch_ct_add", extra=[(18, 6)])
    add_b = lambda b, a, o: ct_add_raw(o, 2, a, 1, None, 0, b, 2, None, 0)
    assert np.array_equal(separate_run(ring, host, [(6, 6), (20, 4)], add_b, 6), total(far_a, B))
    overlap_rows(ring, host, (6, 6), 6, add_b, "alch_ct_add", coincide_ok=True, extra=[(20, 4)])


# ---- 8. alch_ct_error_term, alch_ct_decrypt_lift ---------------------------------------------------------------------------------------------------
def sk_rows(ring, host, per, call, fn, out_count=2):
    """The key element (index into the parent) against an output range of 2 elements that lies clear of the ciphertexts: just before
    it and just after it accepted (equal to the separate run), its first and its last element refused.  call(in_view, parent, sk_index,
    out_buffer, out_first); ciphertexts = elements [0, 2 * per)."""
    e = 2 * per
    ofirst = e + 1
    assert ofirst + out_count + 1 <= len(host)
    for sk, ok in ((e, True), (ofirst + out_count, True), (ofirst, False), (ofirst + out_count - 1, False)):
        if ok:
            parent, (cts,) = carve(ring, host, (0, e))
            sep = ring.alloc(out_count)
            call(cts, parent, sk, sep, 0)
            want = sep.download()
            accepted(ring, host, [(0, e)], lambda c, parent: call(c, parent, sk, parent, ofirst), (ofirst, out_count), want, (fn, "sk", sk))
        else:
            refused(ring, host, [(0, e)], lambda c, parent: call(c, parent, sk, parent, ofirst), fn, (fn, "sk", sk))


@pytest.mark.parametrize("degree", [1, 2])
def test_error_term(degree):
    """batch 2: the output range (2 elements) against the (degree + 1) * batch ciphertext elements -- touching on either side
    accepted, one shared element on either side and the start of the ciphertexts refused -- and against the key element."""
    from alchemy_amd.decrypt import error_term
    ring, qs = ring_of("P32x2")
    per = degree + 1
    host = words(8000 + degree, 2 * per + 5, ring.n, qs)
    sk_clear = len(host) - 1
    call = lambda c, sk, o: error_term(c, 2, sk, degree=degree, out=o, sk_index=0)
    overlap_rows(ring, host, (2, 2 * per), 2, call, "alch_ct_error_term", extra=[(sk_clear, 1)])
    sk_rows(ring, host, per, lambda c, parent, sk, o, of: error_term(c, 2, parent, degree=degree, out=o, out_first=of, sk_index=sk),
            "alch_ct_error_term")


@pytest.mark.parametrize("degree", [1, 2])
def test_decrypt_lift(degree):
    """The same rows for alch_ct_decrypt_lift on a ring of one 31-bit modulus, which can lift into itself."""
    from alchemy_amd.decrypt import decrypt_lift
    ring, qs = ring_of("P32x1")
    per = degree + 1
    host = words(8100 + degree, 2 * per + 5, ring.n, qs)
    sk_clear = len(host) - 1
    call = lambda c, sk, o: decrypt_lift(c, 2, sk, degree=degree, dst=o)
    overlap_rows(ring, host, (2, 2 * per), 2, call, "alch_ct_decrypt_lift", extra=[(sk_clear, 1)])
    sk_rows(ring, host, per, lambda c, parent, sk, o, of: decrypt_lift(c, 2, parent, degree=degree, dst=o, dst_first=of, sk_index=sk),
            "alch_ct_decrypt_lift")


# ---- 9. the other entry points that already checked ---------------------------------------------------------------------------------------------
def test_buf_lift():
    """alch_buf_lift of a one-limb ring into itself, count 2: in place accepted, adjacent accepted, shifted by one refused."""
    from alchemy_amd.decrypt import lift
    ring, qs = ring_of("P32x1")
    host = words(9000, 8, ring.n, qs)
    overlap_rows(ring, host, (3, 2), 2, lambda s, d: lift(s, d, count=2), "alch_buf_lift", coincide_ok=True)


def plain_words(seed, count):
    r = plain_ring()
    return words(seed, count, r.n, [P_PLAIN])


def test_pt_rescale():
    """alch_pt_rescale from Z_4 to itself (the divisor is 1: dst holds src's words), count 2."""
    from alchemy_amd.plaintext import pt_rescale
    r = plain_ring()
    host = plain_words(9100, 8)
    assert np.array_equal(separate_run(r, host, [(3, 2)], lambda s, d: pt_rescale(s, d, 2), 2), host[3:5])
    overlap_rows(r, host, (3, 2), 2, lambda s, d: pt_rescale(s, d, 2), "alch_pt_rescale", coincide_ok=True)


def test_pt_eval_lin():
    """alch_pt_eval_lin through a linear function from index 32 to itself (d_rel = 1), count 2: any overlap refused, adjacent accepted."""
    from alchemy_amd.plaintext import pt_linear
    lift_ring, _ = ring_of("P32x2")
    r = plain_ring()
    f = pt_linear(lift_ring, r.upload(plain_words(9200, 1)), 32)
    host = plain_words(9201, 8)
    overlap_rows(r, host, (3, 2), 2, lambda s, d: f.apply(s, d, 2), "alch_pt_eval_lin")


@pytest.mark.parametrize("name", ["P32x2", "G9"])
def test_tensor_op_and_copy(oracle_lib, name):
    """alch_buf_tensor_op (crt) and alch_buf_copy between ranges of ONE buffer handle, count 2: the same range is in place / a no-op,
    adjacent ranges accepted (crt equal to the C restatement, copy to the source words), one shared element refused."""
    from alchemy_amd import capi
    ring, qs = ring_of(name)
    o = oracle_ring(oracle_lib, name)
    host = words(9300 + ring.n, 8, ring.n, qs)
    crt = np.stack([o.crt(e) for e in host[3:5]])
    for fn, run, want in (("alch_buf_tensor_op", lambda p, df: p.tensor_op(p, capi.ALCH_T_CRT, count=2, dst_first=df, src_first=3), crt),
                          ("alch_buf_copy", lambda p, df: p.copy_from(p, 2, dst_first=df, src_first=3), host[3:5])):
        for df, ok in ((3, True), (1, True), (5, True), (2, False), (4, False)):
            call = lambda parent: run(parent, df)
            if ok:
                accepted(ring, host, [], call, (df, 2), want, (fn, df))
            else:
                refused(ring, host, [], call, fn, (fn, df))


def test_add_bcast_and_pt_mul():
    """alch_buf_add_bcast (the twin the public-element rule comes from) and alch_pt_mul on Z_4: the rows of 1 and 2."""
    from alchemy_amd.plaintext import add_bcast, pt_mul
    lift_ring, _ = ring_of("P32x2")
    r = plain_ring()
    host = plain_words(9400, 12)
    for p in (3, 4, 5, 2, 6, 9):
        call = lambda d, s, parent: add_bcast(d, s, parent, p, 3)
        if p in (3, 4, 5):
            refused(r, host, [(3, 3), (8, 3)], call, "alch_buf_add_bcast", p)
        else:
            accepted(r, host, [(3, 3), (8, 3)], call, (3, 3), (host[8:11] + host[p]) % P_PLAIN, p)
    add = lambda s, d: add_bcast(d, s, s.ring.upload(plain_words(9401, 1)), 0, 2)
    overlap_rows(r, host, (4, 2), 2, add, "alch_buf_add_bcast", coincide_ok=True)
    for swap in (False, True):
        mul = (lambda y, x, d: pt_mul(lift_ring, d, x, y, 2)) if swap else (lambda x, y, d: pt_mul(lift_ring, d, x, y, 2))
        overlap_rows(r, host, (4, 2), 2, mul, "alch_pt_mul", coincide_ok=True, extra=[(10, 2)])
