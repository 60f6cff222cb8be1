"""GPU: weighted sums of hoisted rotations -- alch_ct_automorph_lincomb (include/alchemy_hip.h, "Weighted sums of hoisted rotations";
kernel_lincomb.hpp).

    out[g batch + b].c_i[k] = sum_r w[w_first + g R + r][k] y_r[b].c_i[k]   (mod q_limb)

The reference is the composition the header names, made of calls that exist without this entry point: alch_ct_automorph_hoisted
(per rotation), alch_buf_mul_public per (row, rotation) and a sum mod q_j (lincomb_cases.reference).  Every comparison is exact,
every ring asserts its word size and every stored word is below its modulus."""
import ctypes as C

import numpy as np
import pytest

import alchemy_amd as A
from alchemy_amd import capi
from helpers import assert_parent_unchanged, assert_reduced, extreme_words, lazy_group
from lincomb_cases import WORD_BYTES, all_units, kernel_constants, moduli, reference, uniform, unit_set

pytestmark = pytest.mark.gpu

TRIV, BASE2, POW2_4 = capi.ALCH_GAD_TRIV, capi.ALCH_GAD_BASE2, capi.ALCH_GAD_BASEPOW2(4)
KEY = bytes(range(32))
ROWS, TILE = kernel_constants()


def test_the_row_counts_below_are_those_of_the_kernel():
    """n_out = ROWS, ROWS + 1 and 2 ROWS + 1 are spelt 4, 5 and 9 in CASES; batch 5 is two tiles and a tail: a retune moves them."""
    assert (ROWS, TILE) == (4, 2)


def make_ring(m, kind):
    qs = moduli(m, kind)
    ring = A.Ring(m, qs)
    assert ring.word_bytes == WORD_BYTES[kind]
    return ring, qs


def run(ring, qs, aset, wts, w_first, n_out, cts, batch, s_pre, want):
    """The call into a buffer with a guard element behind it, against `want` ((n_out, 2 * batch, n, L))."""
    out = ring.alloc(2 * batch * n_out + 1)
    out.fill_uniform(3)
    guard = out.download(2 * batch * n_out, 1)
    assert A.ct_automorph_lincomb(aset, wts, cts, batch, n_out=n_out, w_first=w_first, s_pre=s_pre, out=out) is out
    got = out.download(0, 2 * batch * n_out)
    assert_reduced(got, qs)
    assert np.array_equal(got.reshape(want.shape), want)
    assert np.array_equal(out.download(2 * batch * n_out, 1), guard)       # nothing past 2 * n_out * batch elements
    return out


# ---- 1. against the composition ------------------------------------------------------------------------------------------------------------
CASES = [
    # m', moduli, gadget, unit set, s_pre = -1, keyed, n_out, batch
    (64, "top31", TRIV, "three", False, False, 1, 5),            # n = 32: one workgroup; K = 0, product-at-a-time
    (64, "p28", BASE2, "three", True, False, 2, 5),
    (64, "p28", POW2_4, "one", False, False, 4, 1),              # R = 1, a tile with a dead lane
    (64, "top62", TRIV, "rep", True, False, 5, 5),
    (64, "p28", TRIV, "r32", False, False, 9, 5),                # R = 32, three row blocks
    (1 << 12, "p28", TRIV, "three", True, True, 5, 5),           # several wavefronts; a keyed ring
    (1 << 12, "top31", POW2_4, "rep", False, False, 2, 5),
    (1 << 12, "top62", BASE2, "three", True, False, 4, 1),       # one 62-bit limb
    (1 << 12, "top62", TRIV, "r32", False, False, 1, 5),
    (1 << 17, "top31", TRIV, "three", False, False, 1, 5),       # n = 2^16: the split size of 4-byte words
    (9, "top31", TRIV, "three", False, False, 5, 5),             # n = 6: the one-word form
    (9, "p28", POW2_4, "rep", True, False, 9, 1),
    (9, "mix64", BASE2, "three", True, False, 2, 5),
    (45, "p28", TRIV, "three", False, True, 9, 5),               # n = 24: 16-byte pieces through the table
    (45, "top31", BASE2, "rep", True, False, 4, 5),
    (45, "top62", POW2_4, "r32", False, False, 2, 1),
    (45, "mix64", TRIV, "three", True, False, 5, 5),
    (21, "p28", TRIV, "three", True, False, 5, 5),
    (21, "mix64", POW2_4, "rep", False, False, 4, 5),
    (11648, "top31", TRIV, "three", False, False, 2, 5),         # n = 4608, two limbs
]


@pytest.mark.parametrize("m,kind,gadget,units,neg,keyed,n_out,batch", CASES, ids=lambda v: str(v))
def test_lincomb_equals_the_composition(m, kind, gadget, units, neg, keyed, n_out, batch):
    ring, qs = make_ring(m, kind)
    if keyed:
        ring.set_rng_key(KEY)
    js = unit_set(m, units)
    R, D = len(js), ring.gadget_digits(gadget)
    rng = np.random.default_rng(m + gadget + R + n_out)
    ks = ring.upload(uniform(rng, 2 * D * R, ring.n, qs))
    cts_host = uniform(rng, 2 * batch, ring.n, qs)
    w_first = 1 + m % 3                                          # the weights start inside their buffer
    w_host = extreme_words(rng, w_first + n_out * R + 1, ring.n, qs)
    cts, wts = ring.upload(cts_host), ring.upload(w_host)
    s_pre = [q - 1 for q in qs] if neg else None
    aset = A.AutomorphSet(ring, js, ks, gadget)
    want = reference(ring, aset, wts, w_first, n_out, cts, batch, s_pre)
    assert_reduced(want, qs)
    out = run(ring, qs, aset, wts, w_first, n_out, cts, batch, s_pre, want)
    assert np.array_equal(cts.download(), cts_host)              # the input and the weights are not modified
    assert np.array_equal(wts.download(), w_host)
    # the weights are read at call time, not later: overwritten once the call has returned and been synced, the result stands
    got = out.download(0, 2 * batch * n_out)
    ring.sync()
    wts.fill_uniform(77)
    ring.sync()
    assert np.array_equal(out.download(0, 2 * batch * n_out), got)
    # batch = 0 and n_out = 0: nothing queued
    lib = capi.load_library()
    before = out.download()
    assert lib.alch_ct_automorph_lincomb(aset._h, wts._h, w_first, n_out, cts._h, out._h, 0, None, 0) == capi.ALCH_OK
    assert lib.alch_ct_automorph_lincomb(aset._h, wts._h, w_first, 0, cts._h, out._h, batch, None, 0) == capi.ALCH_OK
    assert np.array_equal(out.download(), before)
    aset.free()


# ---- 2. the two corollaries ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,kind,gadget", [(64, "p28", TRIV), (1 << 12, "top62", BASE2), (45, "top31", POW2_4), (9, "mix64", TRIV)],
                         ids=lambda v: str(v))
def test_all_ones_is_the_sum_form_and_a_unit_row_is_one_rotation(m, kind, gadget):
    batch = 5
    ring, qs = make_ring(m, kind)
    js = unit_set(m, "three")
    R, D = len(js), ring.gadget_digits(gadget)
    rng = np.random.default_rng(m)
    ks = ring.upload(uniform(rng, 2 * D * R, ring.n, qs))
    cts = ring.upload(uniform(rng, 2 * batch, ring.n, qs))
    s_pre = [q - 1 for q in qs]
    aset = A.AutomorphSet(ring, js, ks, gadget)
    rot = A.ct_automorph_hoisted(aset, cts, batch, s_pre=s_pre).download(0, 2 * batch * R).reshape(R, 2 * batch, ring.n, ring.L)
    summed = A.ct_automorph_hoisted(aset, cts, batch, s_pre=s_pre, sum=True).download(0, 2 * batch)
    ones = ring.upload(np.ones((R, ring.n, ring.L), dtype=np.int64))               # crt(1): 1 in every slot
    assert np.array_equal(A.ct_automorph_lincomb(aset, ones, cts, batch, s_pre=s_pre).download(0, 2 * batch), summed)
    # row g picks rotation g: weight crt(1) at r0 = g, zero elsewhere (R + 1 rows: the last one is all zero)
    pick = np.zeros(((R + 1) * R, ring.n, ring.L), dtype=np.int64)
    for g in range(R):
        pick[g * R + g] = 1
    got = A.ct_automorph_lincomb(aset, ring.upload(pick), cts, batch, n_out=R + 1, s_pre=s_pre).download(0, 2 * batch * (R + 1))
    got = got.reshape(R + 1, 2 * batch, ring.n, ring.L)
    assert np.array_equal(got[:R], rot) and not got[R].any()
    aset.free()


# ---- 3. the lazy groups of the rows --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [64, 45])
@pytest.mark.parametrize("R", [7, 8, 9, 16, 17])
def test_row_groups_at_their_worst(m, R):
    """Two limbs just above 2^28: K = 8 weighted products per 64-bit group, so R = 7, 8, 9, 16, 17 lies on either side of K, at 2 K
    and beyond it.  TrivGad, c0 = c1 = q - 1 in every slot (crt(-1), whose centred digits are the constant -1:
    tests/test_lincomb_host.py checks that on the C restatement), hints b_t = 0, a_0 = crt(1), a_t = 0 for t > 0: every y_r is q - 1
    in every slot of both components, and with every weight word q - 1 every product is (q - 1)^2 and every output word R mod q."""
    batch, n_out = 5, 2
    ring, qs = make_ring(m, "p28")
    K, D = lazy_group(qs[0]), ring.gadget_digits(TRIV)
    assert K == 8 and D == 2 and (R < K or R == K or K < R <= 2 * K or R > 2 * K)
    us = all_units(m)
    js = [us[(3 * r + 1) % len(us)] for r in range(R)]
    qv = np.array(qs, dtype=np.int64)
    hint = np.zeros((2 * D, ring.n, ring.L), dtype=np.int64)     # (b_0, a_0, b_1, a_1)
    hint[1] = 1
    ks = ring.upload(np.concatenate([hint] * R))
    cts = ring.upload(np.ascontiguousarray(np.broadcast_to(qv - 1, (2 * batch, ring.n, ring.L))))
    wts = ring.upload(np.ascontiguousarray(np.broadcast_to(qv - 1, (n_out * R, ring.n, ring.L))))
    aset = A.AutomorphSet(ring, js, ks, TRIV)
    rot = A.ct_automorph_hoisted(aset, cts, batch).download(0, 2 * batch * R)
    assert np.array_equal(rot, np.broadcast_to(qv - 1, rot.shape))                  # every y_r is q - 1 everywhere
    want = reference(ring, aset, wts, 0, n_out, cts, batch, None)
    assert np.array_equal(want, np.broadcast_to(R % qv, want.shape))                # the closed form
    run(ring, qs, aset, wts, 0, n_out, cts, batch, None, want)
    # and extreme words throughout, against the reference alone
    rng = np.random.default_rng(R)
    ks2 = ring.upload(np.ascontiguousarray(np.broadcast_to(qv - 1, (2 * D * R, ring.n, ring.L))))
    cts2 = ring.upload(extreme_words(rng, 2 * batch, ring.n, qs))
    wts2 = ring.upload(extreme_words(rng, n_out * R, ring.n, qs))
    aset2 = A.AutomorphSet(ring, js, ks2, TRIV)
    s_pre = [q - 1 for q in qs]
    run(ring, qs, aset2, wts2, 0, n_out, cts2, batch, s_pre, reference(ring, aset2, wts2, 0, n_out, cts2, batch, s_pre))
    aset.free()
    aset2.free()


# ---- 4. the scratch walk -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,per_ct_elems", [(1 << 12, 2 + 4), (5824, 2 + 2 + 4)], ids=lambda v: str(v))
def test_chunked_walk_equals_the_unchunked_call(m, per_ct_elems):
    """scratch_mib = 1: chunks of a few ciphertexts with a ragged last one (the carve of alch_ct_automorph_hoisted: 5 ciphertexts at
    n = 2^11, 3 at 5824 = 2^6 7 13), rows in two blocks, against the same call on the default budget and against the reference."""
    qs = moduli(m, "top31x4")
    ring, small = A.Ring(m, qs), A.Ring(m, qs)
    assert ring.word_bytes == 4
    small.set_option("scratch_mib", 1)
    chunk = (1 << 20) // (per_ct_elems * ring.n * ring.L * ring.word_bytes)
    batch, n_out = 2 * chunk + 2, ROWS + 1
    assert chunk >= 3 and batch % chunk
    js = unit_set(m, "three")
    D = ring.gadget_digits(TRIV)
    rng = np.random.default_rng(m)
    ks_host, cts_host = uniform(rng, 2 * D * 3, ring.n, qs), uniform(rng, 2 * batch, ring.n, qs)
    w_host = uniform(rng, n_out * 3, ring.n, qs)
    s_pre = [q - 1 for q in qs]
    outs = []
    for r in (ring, small):
        aset = A.AutomorphSet(r, js, r.upload(ks_host), TRIV)
        outs.append(A.ct_automorph_lincomb(aset, r.upload(w_host), r.upload(cts_host), batch, n_out=n_out, s_pre=s_pre).download(0, 2 * batch * n_out))
        aset.free()
    assert np.array_equal(outs[0], outs[1])
    aset = A.AutomorphSet(ring, js, ring.upload(ks_host), TRIV)
    want = reference(ring, aset, ring.upload(w_host), 0, n_out, ring.upload(cts_host), batch, s_pre)
    assert np.array_equal(outs[1].reshape(want.shape), want)
    aset.free()


# ---- 5. footprint --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,kind,gadget", [(64, "p28", TRIV), (45, "top31", POW2_4), (9, "mix64", TRIV), (1 << 12, "top62", TRIV)], ids=lambda v: str(v))
def test_footprint_inside_one_parent(m, kind, gadget):
    batch, R, n_out = 3, 2, ROWS + 1
    ring, qs = make_ring(m, kind)
    js = unit_set(m, "three")[:R]
    D = ring.gadget_digits(gadget)
    rng = np.random.default_rng(m)
    ks = ring.upload(uniform(rng, 2 * D * R, ring.n, qs))
    # parent: 3 before | in (2 batch) | 3 between | weights (n_out R) | 3 between | out (2 n_out batch) | 3 behind
    i0 = 3
    w0 = i0 + 2 * batch + 3
    o0 = w0 + n_out * R + 3
    total = o0 + 2 * n_out * batch + 3
    host = uniform(rng, total, ring.n, qs)
    parent = ring.upload(host)
    vin, vout = parent.view(i0, 2 * batch), parent.view(o0, 2 * n_out * batch)
    aset = A.AutomorphSet(ring, js, ks, gadget)
    want = reference(ring, aset, ring.upload(host[w0:w0 + n_out * R]), 0, n_out, ring.upload(host[i0:i0 + 2 * batch]), batch, None)
    # the weights once as a view of their own, once as a range of the parent addressed through w_first
    for wbuf, w_first in ((parent.view(w0, n_out * R), 0), (parent, w0)):
        parent.upload(host)
        A.ct_automorph_lincomb(aset, wbuf, vin, batch, n_out=n_out, w_first=w_first, out=vout)
        got = assert_parent_unchanged(parent, host, [(o0, 2 * n_out * batch)])
        assert_reduced(got[o0:o0 + 2 * n_out * batch], qs)
        assert np.array_equal(got[o0:o0 + 2 * n_out * batch].reshape(want.shape), want)
    # one ciphertext, one row or one weight more than a view holds is refused, nothing written
    parent.upload(host)
    lib = capi.load_library()
    wv = parent.view(w0, n_out * R)
    for args in ((wv._h, 0, n_out, vin._h, vout._h, batch + 1), (wv._h, 0, n_out + 1, vin._h, vout._h, batch),
                 (wv._h, 1, n_out, vin._h, vout._h, batch), (parent.view(w0, n_out * R - 1)._h, 0, n_out, vin._h, vout._h, batch)):
        assert lib.alch_ct_automorph_lincomb(aset._h, *args, None, 0) == capi.ALCH_E_INVALID
        assert lib.alch_last_error().decode().startswith("alch_ct_automorph_lincomb:")
    assert_parent_unchanged(parent, host)
    aset.free()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_statuses():
    m, batch, n_out = 45, 2, 2
    qs = moduli(m, "p28")
    ring, other = A.Ring(m, qs), A.Ring(m, qs[:1])
    D = ring.gadget_digits(TRIV)
    ks = ring.alloc(4 * D)
    ks.fill_uniform(1)
    aset = A.AutomorphSet(ring, [2, 7 + 45], ks)
    R = 2
    # parent: in (2 batch) | weights (n_out R) | out (2 n_out batch) | 2 spare
    w0, o0 = 2 * batch, 2 * batch + n_out * R
    host = uniform(np.random.default_rng(1), o0 + 2 * n_out * batch + 2, ring.n, qs)
    parent = ring.upload(host)
    vin, vw, vout = parent.view(0, 2 * batch), parent.view(w0, n_out * R), parent.view(o0, 2 * n_out * batch)
    lib = capi.load_library()

    def call(a, w, i, o, want, b=batch, g=n_out, w_first=0, flags=0):
        rc = lib.alch_ct_automorph_lincomb(a, w._h if w else None, w_first, g, i._h if i else None, o._h if o else None, b, None, flags)
        msg = lib.alch_last_error().decode()
        assert rc == want, (rc, msg)
        if rc != capi.ALCH_OK:
            assert msg.startswith("alch_ct_automorph_lincomb:"), msg

    INV, UNS = capi.ALCH_E_INVALID, capi.ALCH_E_UNSUPPORTED
    call(None, vw, vin, vout, INV)                                                       # 1. null
    call(aset._h, None, vin, vout, INV)
    call(aset._h, vw, None, vout, INV)
    call(aset._h, vw, vin, None, INV)
    oc = other.alloc(4 * n_out * batch)
    call(aset._h, oc, vin, vout, INV)                                                    #    buffers of another ring
    call(aset._h, vw, oc, vout, INV)
    call(aset._h, vw, vin, oc, INV)
    call(aset._h, vw, vin, vout, INV, flags=8)                                           #    an unknown flag; ALCH_AUTO_SUM is one here
    call(aset._h, vw, vin, vout, INV, flags=capi.ALCH_AUTO_SUM)
    call(aset._h, vw, vin, vout, INV, flags=capi.ALCH_AUTO_SUM | capi.ALCH_POW_IN)       #    ... and comes before UNSUPPORTED
    call(aset._h, None, vin, vout, INV, flags=capi.ALCH_POW_IN)
    for flags in (capi.ALCH_POW_IN, capi.ALCH_POW_OUT, capi.ALCH_POW_IN | capi.ALCH_POW_OUT):
        call(aset._h, vw, vin, vout, UNS, flags=flags)                                   # 2.
        call(aset._h, vw, vin, vout, UNS, flags=flags, b=batch + 1)                      #    ... before the lengths
    call(aset._h, vw, vin, vout, INV, b=batch + 1)                                       # 3. short buffers
    call(aset._h, vw, vin, vout, INV, g=n_out + 1)
    call(aset._h, vw, vin, vout, INV, w_first=1)
    call(aset._h, vw, vin, vout, INV, w_first=2**63)
    call(aset._h, vw, vin, vout, INV, g=2**62)
    call(aset._h, vw, vin, parent.view(2 * batch - 1, 2 * n_out * batch), INV)           #    out overlapping in by one element
    call(aset._h, vw, vin, vin, INV, g=1)
    call(aset._h, vw, vin, parent.view(o0 - 1, 2 * n_out * batch), INV)                  #    out overlapping the weights by one element
    call(aset._h, parent, vin, vout, INV, w_first=o0 - n_out * R + 1)                    #    ... the weight range shifted into out
    assert_parent_unchanged(parent, host)
    call(aset._h, vw, vin, vout, capi.ALCH_OK, b=0)                                      # nothing queued
    call(aset._h, vw, vin, vout, capi.ALCH_OK, g=0)
    call(aset._h, vw, vin, vout, capi.ALCH_OK, b=0, g=2**62)
    assert_parent_unchanged(parent, host)
    call(aset._h, vw, vin, vout, capi.ALCH_OK)                                           # out adjacent to the weights: accepted
    got = assert_parent_unchanged(parent, host, [(o0, 2 * n_out * batch)])
    want = reference(ring, aset, ring.upload(host[w0:o0]), 0, n_out, ring.upload(host[:2 * batch]), batch, None)
    assert np.array_equal(got[o0:o0 + 2 * n_out * batch].reshape(want.shape), want)
    aset.free()


# ---- 7. a loaded stream --------------------------------------------------------------------------------------------------------------------
def test_weights_and_input_produced_behind_ballast():
    """The input and the weights are copied into place behind ballast on the ring's stream; the decomposition and the kernel must run
    after them, and the download right behind the call must see their words."""
    from stream_load import Ballast, busy
    m, batch, n_out = 1 << 12, 5, ROWS + 1
    ring, qs = make_ring(m, "p28")
    js = unit_set(m, "three")
    D = ring.gadget_digits(TRIV)
    rng = np.random.default_rng(12)
    ks = ring.upload(uniform(rng, 2 * D * 3, ring.n, qs))
    staged_ct = ring.upload(uniform(rng, 2 * batch, ring.n, qs))
    staged_w = ring.upload(uniform(rng, n_out * 3, ring.n, qs))
    aset = A.AutomorphSet(ring, js, ks, TRIV)
    want = reference(ring, aset, staged_w, 0, n_out, staged_ct, batch, None)
    cts, wts, out = ring.alloc(2 * batch), ring.alloc(n_out * 3), ring.alloc(2 * n_out * batch)
    cts.fill_uniform(1)
    wts.fill_uniform(5)
    out.fill_uniform(2)
    A.ct_automorph_lincomb(aset, wts, cts, batch, n_out=n_out, out=out)                  # warm: the scratch is reserved before the ballast
    out.fill_uniform(2)
    ring.sync()
    ballast = Ballast(ring)
    ballast.push()
    cts.copy_from(staged_ct, 2 * batch)
    wts.copy_from(staged_w, n_out * 3)
    A.ct_automorph_lincomb(aset, wts, cts, batch, n_out=n_out, out=out)
    assert busy(ring), "the ballast drained before the call returned: the case proved nothing"
    got = out.download()
    assert np.array_equal(got.reshape(want.shape), want)
    ring.sync()
    ballast.close()
    aset.free()
