"""GPU: hoisted automorphisms -- several sigma_j of one batch at one gadget decomposition (include/alchemy_hip.h, "Hoisted
automorphisms"; kernel_hoist.hpp).

The reference is built from calls that already exist.  For a unit j with inverse j' mod m and h' = alch_buf_automorph by j' of the hint
for j, the hoisted result for j is, word for word,

    alch_buf_automorph_j( alch_ct_tunnel( identity tunnel made from crt(1) and h' )(ct, s_pre) )

because the inner product is slot-wise and every stored word is the canonical residue (tests/test_hoist_model.py restates this in
Python integers; the identity tunnel itself is pinned to the C restatement by tests/test_gpu_tunnel*.py).  Two corollaries: for j = 1
the result is alch_ct_automorph's for every gadget, and for TrivGad on two-power rings it is alch_ct_automorph's for every j.  No
equality with alch_ct_automorph is claimed elsewhere: there the digits legitimately differ.  The sum form is the sum of the R
references mod q_i.  Every comparison is exact and every stored word is below its modulus."""
import ctypes as C
import math
import random

import numpy as np
import pytest

import alchemy_amd as A
import automorph_model as M
from alchemy_amd import capi
from alchemy_amd import encrypt as E
from helpers import assert_parent_unchanged, assert_reduced, extreme_words, lazy_group, primes_1_mod, primes_below
from oracle import model_gen as G

pytestmark = pytest.mark.gpu

TRIV, BASE2, POW2_4 = capi.ALCH_GAD_TRIV, capi.ALCH_GAD_BASE2, capi.ALCH_GAD_BASEPOW2(4)
KEY = bytes(range(32))


def moduli(m, kind):
    if kind == "top31":                                          # two 31-bit limbs at the top of 2^31: K = 0, product-at-a-time
        qs = primes_below(m, 2, 1 << 31)
        assert all(lazy_group(q) == 0 for q in qs)
        return qs
    if kind == "top31x4":
        return primes_below(m, 4, 1 << 31)
    if kind == "p28":                                            # the first primes above 2^28: lazy groups of 8
        qs = primes_1_mod(m, 2, 1 << 28)
        assert all(lazy_group(q) == 8 for q in qs)
        return qs
    if kind == "p29":                                            # three 29-bit limbs: room for a key switch's noise
        return primes_1_mod(m, 3, 1 << 28)
    if kind == "top62":                                          # one prime just below 2^62: 8-byte words
        return primes_below(m, 1, 1 << 62)
    if kind == "mix64":                                          # 62 + 17 + 32 bits
        qs = [primes_below(m, 1, 1 << 62)[0], primes_1_mod(m, 1, 1 << 16)[0], primes_1_mod(m, 1, 1 << 31)[0]]
        assert [(q - 1).bit_length() for q in qs] == [62, 17, 32]
        return qs
    raise AssertionError(kind)


def uniform(rng, count, n, qs):
    return np.ascontiguousarray(np.stack([rng.integers(0, q, size=(count, n), dtype=np.int64) for q in qs], axis=2))


def all_units(m):
    return [j for j in range(1, m) if math.gcd(j, m) == 1] if m > 1 else [1]


def unit_set(m, name):
    us = all_units(m)
    rnd = random.Random(m)
    if name == "one":
        return [1]
    if name == "three":                                          # two-power: {5, m - 1, 25}
        return [5, m - 1, 25] if m & (m - 1) == 0 else [us[1], m - 1, rnd.choice(us[2:-1])]
    if name == "rep":                                            # a repeated unit, one of them unreduced
        j = rnd.choice(us[1:])
        return [j, us[1], j + m]
    if name == "r32":
        return [rnd.choice(us) for _ in range(32)]
    raise AssertionError(name)


def pow2(m):
    return m >= 32 and m & (m - 1) == 0


def add_mod(a, b, qs):
    """(a + b) mod q_j per limb; the words are below 2^62, so the int64 sum does not wrap."""
    return np.ascontiguousarray(np.stack([(a[..., l] + b[..., l]) % q for l, q in enumerate(qs)], axis=-1))


def reference(ring, gadget, js, ks, cts, batch, s_pre):
    """(R, 2 * batch, n, L): per unit, sigma_j of the identity tunnel under the hint moved by sigma_(1/j) -- existing calls only."""
    D = ring.gadget_digits(gadget)
    lin = ring.upload(np.ones((1, ring.n, ring.L), dtype=np.int64))
    hp, mid, res = ring.alloc(2 * D), ring.alloc(2 * batch), ring.alloc(2 * batch)
    out = []
    for r, j in enumerate(js):
        A.buf_automorph(hp, ks, pow(j, -1, ring.m), 2 * D, 0, 2 * D * r)
        tun = A.Tunnel(ring, ring, lin, hp, gadget=gadget)
        tun.apply(cts, mid, batch, s_pre=s_pre)
        A.buf_automorph(res, mid, j % ring.m, 2 * batch)
        out.append(res.download(0, 2 * batch))
        tun.free()
    return np.stack(out)


def sum_of(refs, qs):
    acc = refs[0]
    for x in refs[1:]:
        acc = add_mod(acc, x, qs)
    return acc


def run_both_forms(ring, gadget, js, ks, cts, batch, s_pre, want, qs):
    """The per-rotation form and the sum form against `want` ((R, 2 * batch, n, L)), with a guard element behind either output."""
    R = len(js)
    aset = A.AutomorphSet(ring, js, ks, gadget)
    out = ring.alloc(2 * batch * R + 1)
    out.fill_uniform(3)
    guard = out.download(2 * batch * R, 1)
    assert A.ct_automorph_hoisted(aset, cts, batch, s_pre=s_pre, out=out) is out
    got = out.download(0, 2 * batch * R)
    assert_reduced(got, qs)
    assert np.array_equal(got.reshape(want.shape), want)
    assert np.array_equal(out.download(2 * batch * R, 1), guard)           # nothing past 2 * R * batch elements
    ssum = ring.alloc(2 * batch + 1)
    ssum.fill_uniform(4)
    guard = ssum.download(2 * batch, 1)
    A.ct_automorph_hoisted(aset, cts, batch, s_pre=s_pre, out=ssum, sum=True)
    got = ssum.download(0, 2 * batch)
    assert_reduced(got, qs)
    assert np.array_equal(got, sum_of(want, qs))
    assert np.array_equal(ssum.download(2 * batch, 1), guard)
    return aset


# ---- 1. both forms against the reference ----------------------------------------------------------------------------------------------
ROWS = [
    # m', moduli, gadget, unit set, s_pre = -1, keyed
    (64, "top31", TRIV, "three", False, False),                  # n = 32: one workgroup
    (64, "p28", BASE2, "three", True, False),
    (64, "p28", POW2_4, "one", False, False),
    (64, "top62", TRIV, "rep", True, False),
    (64, "mix64", POW2_4, "three", False, False),
    (1 << 12, "p28", TRIV, "three", True, True),                 # several wavefronts
    (1 << 12, "top31", POW2_4, "rep", False, False),
    (1 << 12, "mix64", BASE2, "one", True, False),
    (1 << 17, "top31", TRIV, "three", False, False),             # n = 2^16: the split size of 4-byte words
    (1 << 16, "top62", TRIV, "three", True, False),              # n = 2^15: the split size of 8-byte words
    (1 << 16, "top62", POW2_4, "one", False, False),             #   and its k_decompose_base2 + crt digit tail
    (9, "top31", TRIV, "three", False, False),                   # n = 6: the one-word form
    (9, "p28", POW2_4, "rep", True, False),
    (9, "mix64", BASE2, "three", True, False),
    (45, "p28", TRIV, "three", False, True),                     # n = 24: 16-byte packs
    (45, "top31", BASE2, "rep", True, False),
    (45, "top62", POW2_4, "three", False, False),
    (21, "p28", TRIV, "three", True, False),
    (21, "mix64", TRIV, "rep", False, False),
    (11648, "top31", TRIV, "three", False, False),               # n = 4608, two limbs
    (11648, "top31", POW2_4, "one", True, False),
]


@pytest.mark.parametrize("m,kind,gadget,units,neg,keyed", ROWS, ids=lambda v: str(v))
def test_hoisted_equals_permuted_identity_tunnel(m, kind, gadget, units, neg, keyed):
    batch = 5                                                    # a tile of four and a tail
    qs = moduli(m, kind)
    ring = A.Ring(m, qs)
    if keyed:
        ring.set_rng_key(KEY)
    js = unit_set(m, units)
    R, D = len(js), ring.gadget_digits(gadget)
    rng = np.random.default_rng(m + gadget + R)
    ks_host = uniform(rng, 2 * D * R, ring.n, qs)
    cts_host = uniform(rng, 2 * batch, ring.n, qs)
    ks, cts = ring.upload(ks_host), ring.upload(cts_host)
    s_pre = [q - 1 for q in qs] if neg else None
    want = reference(ring, gadget, js, ks, cts, batch, s_pre)
    assert_reduced(want, qs)
    aset = A.AutomorphSet(ring, js, ks, gadget)
    assert aset.js == [j % m for j in js]
    ks.fill_uniform(12345)                                       # the hints were copied at create time
    out = ring.alloc(2 * batch * R + 1)
    out.fill_uniform(3)
    guard = out.download(2 * batch * R, 1)
    assert A.ct_automorph_hoisted(aset, cts, batch, s_pre=s_pre, out=out) is out
    got = out.download(0, 2 * batch * R)
    assert_reduced(got, qs)
    assert np.array_equal(got.reshape(want.shape), want)
    assert np.array_equal(out.download(2 * batch * R, 1), guard)
    assert np.array_equal(cts.download(), cts_host)              # the input is not modified
    ssum = A.ct_automorph_hoisted(aset, cts, batch, s_pre=s_pre, sum=True)
    got = ssum.download(0, 2 * batch)
    assert_reduced(got, qs)
    assert np.array_equal(got, sum_of(want, qs))
    # the corollaries: alch_ct_automorph's words for j = 1 (any gadget), and for every j under TrivGad on a two-power ring
    ks.upload(ks_host)
    for r, j in enumerate(js):
        if j % m == 1 or (gadget == TRIV and pow2(m)):
            one = ring.alloc(2 * D)
            one.copy_from(ks, 2 * D, 0, 2 * D * r)
            auto = A.Automorph(ring, j, one, gadget)
            assert np.array_equal(A.ct_automorph(auto, cts, batch, s_pre=s_pre).download(0, 2 * batch), want[r]), (m, j)
            auto.free()
    # batch = 0: nothing queued
    lib = capi.load_library()
    before = out.download()
    assert lib.alch_ct_automorph_hoisted(aset._h, cts._h, out._h, 0, None, 0) == capi.ALCH_OK
    assert np.array_equal(out.download(), before)
    aset.free()


@pytest.mark.parametrize("m,kind,gadget", [(64, "p28", TRIV), (1 << 12, "top31", BASE2), (45, "p28", POW2_4)], ids=lambda v: str(v))
def test_thirty_two_units_and_no_more(m, kind, gadget):
    batch = 5
    qs = moduli(m, kind)
    ring = A.Ring(m, qs)
    js = unit_set(m, "r32")
    D = ring.gadget_digits(gadget)
    rng = np.random.default_rng(m)
    ks = ring.upload(uniform(rng, 2 * D * 33, ring.n, qs))
    cts = ring.upload(uniform(rng, 2 * batch, ring.n, qs))
    want = reference(ring, gadget, js, ks, cts, batch, None)
    run_both_forms(ring, gadget, js, ks, cts, batch, None, want, qs).free()
    h = C.c_void_p()
    arr = (C.c_uint32 * 33)(*(js + [1]))
    lib = capi.load_library()
    assert lib.alch_automorph_set_create(ring._h, 33, arr, gadget, ks._h, C.byref(h)) == capi.ALCH_E_INVALID
    assert lib.alch_last_error().decode().startswith("alch_automorph_set_create:") and h.value is None


# ---- 2. the scratch walk ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,gadget,per_ct_elems", [(1 << 12, TRIV, 2 + 4), (5824, TRIV, 2 + 2 + 4)], ids=lambda v: str(v))
def test_chunked_walk_equals_the_unchunked_call(m, gadget, per_ct_elems):
    """scratch_mib = 1: chunks of a few ciphertexts with a ragged last one, against the same call on the default budget.  Per
    ciphertext the scratch holds the Pow copy (2 elements), on the general engine the scaled (c0, c1) the gather writes (2), and the
    four TrivGad digits: 192 KiB at n = 2^11 and 288 KiB at 5824 = 2^6 7 13 (n = 2304), so chunks of 5 and of 3."""
    qs = moduli(m, "top31x4")
    ring, small = A.Ring(m, qs), A.Ring(m, qs)
    small.set_option("scratch_mib", 1)
    chunk = (1 << 20) // (per_ct_elems * ring.n * ring.L * ring.word_bytes)
    batch = 2 * chunk + 2
    assert chunk >= 3 and batch % chunk
    js = unit_set(m, "three")
    D = ring.gadget_digits(gadget)
    rng = np.random.default_rng(m)
    ks_host, cts_host = uniform(rng, 2 * D * 3, ring.n, qs), uniform(rng, 2 * batch, ring.n, qs)
    outs = []
    for r in (ring, small):
        aset = A.AutomorphSet(r, js, r.upload(ks_host), gadget)
        cts = r.upload(cts_host)
        full = A.ct_automorph_hoisted(aset, cts, batch, s_pre=[q - 1 for q in qs]).download(0, 6 * batch)
        summed = A.ct_automorph_hoisted(aset, cts, batch, s_pre=[q - 1 for q in qs], sum=True).download(0, 2 * batch)
        outs.append((full, summed))
        aset.free()
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert np.array_equal(outs[0][1], sum_of(outs[0][0].reshape(3, 2 * batch, ring.n, ring.L), qs))
    # and against the reference on the first and the last ciphertext of the batch
    ks, cts = ring.upload(ks_host), ring.upload(cts_host)
    want = reference(ring, gadget, js, ks, cts, batch, [q - 1 for q in qs])
    assert np.array_equal(outs[1][0].reshape(want.shape), want)


# ---- 3. the lazy groups of the sum form ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [64, 45])
@pytest.mark.parametrize("R", [3, 4, 5, 8, 9])
def test_sum_form_lazy_groups_at_their_worst(m, R):
    """Two limbs just above 2^28: K = 8 products per 64-bit group, TrivGad D = 2, so R D = 6, 8, 10, 16, 18 lies on either side of K,
    at 2 K and beyond it.  Every hint word is q - 1; the inputs are extreme residues, and c1 of the even ciphertexts is crt(-1), whose
    digits are the constant -1: q - 1 in every slot, so every product of those ciphertexts is (q - 1)^2."""
    batch = 5
    qs = moduli(m, "p28")
    ring = A.Ring(m, qs)
    K, D = lazy_group(qs[0]), ring.gadget_digits(TRIV)
    assert K == 8 and D == 2 and (R * D < K or R * D == K or K < R * D <= 2 * K or R * D > 2 * K)
    us = all_units(m)
    js = [us[(3 * r + 1) % len(us)] for r in range(R)]
    rng = np.random.default_rng(R)
    qv = np.array(qs, dtype=np.int64)
    ks_host = np.ascontiguousarray(np.broadcast_to(qv - 1, (2 * D * R, ring.n, ring.L)))
    cts_host = extreme_words(rng, 2 * batch, ring.n, qs)
    for b in range(0, batch, 2):
        cts_host[2 * b + 1] = qv - 1
    ks, cts = ring.upload(ks_host), ring.upload(cts_host)
    for s_pre in (None, [q - 1 for q in qs]):
        want = reference(ring, TRIV, js, ks, cts, batch, s_pre)
        run_both_forms(ring, TRIV, js, ks, cts, batch, s_pre, want, qs).free()


# ---- 4. footprint ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,kind,gadget", [(64, "p28", TRIV), (45, "top31", POW2_4), (9, "mix64", TRIV), (1 << 12, "top62", TRIV)], ids=lambda v: str(v))
def test_footprint_inside_one_parent(m, kind, gadget):
    batch, R = 3, 2
    qs = moduli(m, kind)
    ring = A.Ring(m, qs)
    js = unit_set(m, "three")[:R]
    D = ring.gadget_digits(gadget)
    rng = np.random.default_rng(m)
    ks = ring.upload(uniform(rng, 2 * D * R, ring.n, qs))
    # parent: 2 before | in (2 batch) | 3 between | out (2 R batch) | 2 behind
    i0, o0 = 2, 2 + 2 * batch + 3
    total = o0 + 2 * R * batch + 2
    host = uniform(rng, total, ring.n, qs)
    parent = ring.upload(host)
    vin, vout, vsum = parent.view(i0, 2 * batch), parent.view(o0, 2 * R * batch), parent.view(o0, 2 * batch)
    plain = ring.upload(host[i0:i0 + 2 * batch])
    want = reference(ring, gadget, js, ks, plain, batch, None)
    aset = A.AutomorphSet(ring, js, ks, gadget)
    A.ct_automorph_hoisted(aset, vin, batch, out=vout)
    got = assert_parent_unchanged(parent, host, [(o0, 2 * R * batch)])
    assert np.array_equal(got[o0:o0 + 2 * R * batch].reshape(want.shape), want)
    parent.upload(host)
    A.ct_automorph_hoisted(aset, vin, batch, out=vsum, sum=True)
    got = assert_parent_unchanged(parent, host, [(o0, 2 * batch)])
    assert np.array_equal(got[o0:o0 + 2 * batch], sum_of(want, qs))
    # one ciphertext more than either view holds is refused, nothing written
    parent.upload(host)
    lib = capi.load_library()
    for v_in, v_out, flags in ((vin, vout, 0), (vin, vsum, capi.ALCH_AUTO_SUM)):
        assert lib.alch_ct_automorph_hoisted(aset._h, v_in._h, v_out._h, batch + 1, None, flags) == capi.ALCH_E_INVALID
        assert lib.alch_last_error().decode().startswith("alch_ct_automorph_hoisted:")
    assert lib.alch_ct_automorph_hoisted(aset._h, vin._h, vsum._h, batch, None, 0) == capi.ALCH_E_INVALID     # R batch do not fit
    assert_parent_unchanged(parent, host)
    aset.free()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_statuses():
    m, batch = 45, 2
    qs = moduli(m, "p28")
    ring, other = A.Ring(m, qs), A.Ring(m, qs[:1])
    zp = A.Ring(m, [8], nocrt=True)
    D = ring.gadget_digits(TRIV)
    ks, short, ko, kz = ring.alloc(4 * D), ring.alloc(4 * D - 1), other.alloc(8), zp.alloc(8)
    ks.fill_uniform(1)
    lib = capi.load_library()
    h = C.c_void_p()

    def create(r, js, gadget, k, n_j=None):
        arr = (C.c_uint32 * max(1, len(js)))(*js)
        rc = lib.alch_automorph_set_create(r._h if r else None, len(js) if n_j is None else n_j, arr, gadget, k._h if k else None, C.byref(h))
        return rc, lib.alch_last_error().decode()

    def invalid(*args, **kw):
        rc, msg = create(*args, **kw)
        assert rc == capi.ALCH_E_INVALID and msg.startswith("alch_automorph_set_create:"), (rc, msg)
        assert h.value is None
        return msg

    invalid(None, [2, 7], TRIV, ks)                                                      # null
    invalid(ring, [2, 7], TRIV, None)
    assert lib.alch_automorph_set_create(ring._h, 2, None, TRIV, ks._h, C.byref(h)) == capi.ALCH_E_INVALID
    assert lib.alch_automorph_set_create(ring._h, 2, (C.c_uint32 * 2)(2, 7), TRIV, ks._h, None) == capi.ALCH_E_INVALID
    invalid(ring, [2, 7], TRIV, ks, n_j=0)                                               # n_j = 0
    for bad in (3, 0, 45, 48):                                                           # a non-unit, before and after reduction
        assert "unit" in invalid(ring, [2, bad], TRIV, ks)
    invalid(ring, [2, 7], TRIV, short)                                                   # a short hint
    invalid(ring, [2, 7], TRIV, ko)                                                      # a hint of another ring
    invalid(ring, [2, 7], 99, ks)
    invalid(ring, [2, 7], capi.ALCH_GAD_BASEPOW2(17), ks)
    assert create(zp, [2, 7], TRIV, kz)[0] == capi.ALCH_E_NO_CRT
    assert lib.alch_automorph_set_free(None) == capi.ALCH_OK
    aset = A.AutomorphSet(ring, [2, 7 + 45], ks)
    assert aset.js == [2, 7]
    host = uniform(np.random.default_rng(1), 2 * batch + 4 * batch + 2, ring.n, qs)
    parent = ring.upload(host)
    vin, vout = parent.view(0, 2 * batch), parent.view(2 * batch, 4 * batch)

    def call(a, i, o, b, flags, want):
        rc = lib.alch_ct_automorph_hoisted(a, i._h if i else None, o._h if o else None, b, None, flags)
        msg = lib.alch_last_error().decode()
        assert rc == want, (rc, msg)
        if rc != capi.ALCH_OK:
            assert msg.startswith("alch_ct_automorph_hoisted:"), msg

    call(None, vin, vout, batch, 0, capi.ALCH_E_INVALID)                                 # null
    call(aset._h, None, vout, batch, 0, capi.ALCH_E_INVALID)
    call(aset._h, vin, None, batch, 0, capi.ALCH_E_INVALID)
    oc = other.alloc(4 * batch)
    call(aset._h, oc, vout, batch, 0, capi.ALCH_E_INVALID)                               # buffers of another ring
    call(aset._h, vin, oc, batch, 0, capi.ALCH_E_INVALID)
    call(aset._h, vin, vout, batch, 8, capi.ALCH_E_INVALID)                              # an unknown flag
    call(aset._h, vin, vout, batch, 16 | capi.ALCH_AUTO_SUM, capi.ALCH_E_INVALID)
    for flags in (capi.ALCH_POW_IN, capi.ALCH_POW_OUT, capi.ALCH_POW_IN | capi.ALCH_POW_OUT, capi.ALCH_POW_OUT | capi.ALCH_AUTO_SUM):
        call(aset._h, vin, vout, batch, flags, capi.ALCH_E_UNSUPPORTED)
    # out overlapping in by one element, on either side
    call(aset._h, vin, parent.view(2 * batch - 1, 4 * batch), batch, 0, capi.ALCH_E_INVALID)
    call(aset._h, parent.view(4 * batch - 1, 2 * batch), parent.view(0, 4 * batch), batch, 0, capi.ALCH_E_INVALID)
    call(aset._h, vin, parent.view(2 * batch - 1, 2 * batch), batch, capi.ALCH_AUTO_SUM, capi.ALCH_E_INVALID)
    call(aset._h, vin, vin, batch, capi.ALCH_AUTO_SUM, capi.ALCH_E_INVALID)
    assert_parent_unchanged(parent, host)
    call(aset._h, vin, vout, 0, 0, capi.ALCH_OK)                                         # batch = 0: nothing queued
    assert_parent_unchanged(parent, host)
    call(aset._h, vin, vout, batch, 0, capi.ALCH_OK)                                     # adjacent views are fine
    assert_parent_unchanged(parent, host, [(2 * batch, 4 * batch)])
    aset.free()


# ---- 6. end to end ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mp,m,p,js,gadget,keyed", [(64, 16, 8, [5, 63, 25 + 64], TRIV, False), (64, 16, 8, [3, 1], POW2_4, True),
                                                   (45, 9, 4, [7, 44, 2], BASE2, False), (45, 9, 4, [2, 2], TRIV, False)], ids=lambda v: str(v))
def test_encrypt_hoisted_decrypt(mp, m, p, js, gadget, keyed):
    """gen_sk -> automorph_set_hints -> encrypt_batch -> ct_automorph_hoisted -> decrypt_batch: rotation r decrypts to sigma_(j_r mod m)
    of the plaintext, the sum form to the sum of those.  The error rates are printed next to alch_ct_automorph's, not asserted."""
    batch, seed = 4, 9000 + mp + len(js)
    qs = moduli(mp, "p29")
    big, sm = G.Index(mp), G.Index(m)
    svar = 3.0 / np.sqrt(float(big.n))
    ring = A.Ring(mp, qs)
    if keyed:
        ring.set_rng_key(KEY)
    zp_big = A.Ring(mp, [p], nocrt=True)
    zp_small = A.Ring(m, [p], nocrt=True)
    sk = E.gen_sk(ring, svar, seed)
    R, D = len(js), ring.gadget_digits(gadget)
    hints = A.automorph_set_hints(ring, sk, js, gadget, svar, seed + 10)
    assert hints.n_elems == 2 * D * R
    aset = A.AutomorphSet(ring, js, hints, gadget)
    rnd = random.Random(seed)
    pts = np.array([[[rnd.randrange(p)] for _ in range(sm.n)] for _ in range(batch)], dtype=np.int64)
    cts = E.encrypt_batch(ring, sk, zp_small.upload(pts), zp_small, zp_big, svar, seed + 3)
    to_msd, to_lsd = [pow(p, -1, q) for q in qs], [p % q for q in qs]
    meta = A.CtMeta("LSD", 0, 1, p)
    out, meta_out = A.ct_automorph_hoisted(aset, cts, batch, s_pre=to_msd, meta=meta)
    assert meta_out is meta
    want = [[M.sigma_pow([int(x) for x in pts[b, :, 0]], sm, j % m, p) for b in range(batch)] for j in js]
    for r, j in enumerate(js):
        rot = out.view(2 * batch * r, 2 * batch)
        one = ring.alloc(2 * D)
        one.copy_from(hints, 2 * D, 0, 2 * D * r)
        auto = A.Automorph(ring, j, one, gadget)
        plain = A.ct_automorph(auto, cts, batch, s_pre=to_msd)
        print(f"m'={mp} j={j} gadget={gadget}: error rates hoisted {A.error_rates(rot, batch, sk, s_pre=to_lsd)}"
              f" / alch_ct_automorph {A.error_rates(plain, batch, sk, s_pre=to_lsd)}")
        got = A.decrypt_batch(rot, batch, sk, zp_big, zp_small, 0, 1, s_pre=to_lsd).download(0, batch)
        for b in range(batch):
            assert got[b, :, 0].tolist() == want[r][b], (j, b)
        auto.free()
    ssum = A.ct_automorph_hoisted(aset, cts, batch, s_pre=to_msd, sum=True)
    print(f"m'={mp} js={js} gadget={gadget}: error rates of the sum form {A.error_rates(ssum, batch, sk, s_pre=to_lsd)}")
    got = A.decrypt_batch(ssum, batch, sk, zp_big, zp_small, 0, 1, s_pre=to_lsd).download(0, batch)
    for b in range(batch):
        assert got[b, :, 0].tolist() == [sum(want[r][b][i] for r in range(R)) % p for i in range(sm.n)], b
    aset.free()


# ---- 7. a loaded stream -----------------------------------------------------------------------------------------------------------------------
def test_input_produced_behind_ballast():
    """The input is copied into place behind ballast on the ring's stream; the decomposition and the inner products must run after it,
    and the download right behind the call must see their words."""
    from stream_load import Ballast, busy
    m, batch, gadget = 1 << 12, 5, TRIV
    qs = moduli(m, "p28")
    ring = A.Ring(m, qs)
    js = unit_set(m, "three")
    D = ring.gadget_digits(gadget)
    rng = np.random.default_rng(12)
    ks = ring.upload(uniform(rng, 2 * D * 3, ring.n, qs))
    staged = ring.upload(uniform(rng, 2 * batch, ring.n, qs))
    want = reference(ring, gadget, js, ks, staged, batch, None)
    aset = A.AutomorphSet(ring, js, ks, gadget)
    cts, out = ring.alloc(2 * batch), ring.alloc(6 * batch)
    cts.fill_uniform(1)
    out.fill_uniform(2)
    A.ct_automorph_hoisted(aset, cts, batch, out=out)            # warm: the scratch is reserved before the ballast
    out.fill_uniform(2)
    ring.sync()
    ballast = Ballast(ring)
    ballast.push()
    cts.copy_from(staged, 2 * batch)
    A.ct_automorph_hoisted(aset, cts, batch, out=out)
    assert busy(ring), "the ballast drained before the call returned: the case proved nothing"
    got = out.download()
    assert np.array_equal(got.reshape(want.shape), want)
    ring.sync()
    ballast.close()
    aset.free()
