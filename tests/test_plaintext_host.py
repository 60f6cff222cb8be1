"""CPU: the plaintext-side entry points (alch_pt_bound, alch_pt_mul, alch_pt_linear_create / _free, alch_pt_eval_lin, alch_pt_rescale,
alch_buf_add_bcast) exist at every layer a host reaches them through, answer their argument checks without a device, and the
exactness bound the header states really bounds the integer coefficients of products on the powerful basis.  None of the names
exists before the feature, so the tests fail on the parent commit."""
import ctypes as C
import random

import pytest

from oracle import model_gen as G

ENTRY = {
    "alch_pt_bound": ["uint32_t", "uint64_t", "uint32_t", "uint64_t*", "uint64_t*"],
    "alch_pt_mul": ["alch_ring*", "alch_buf*", "alch_buf*", "alch_buf*", "size_t", "unsigned"],
    "alch_pt_linear_create": ["alch_ring*", "alch_buf*", "uint32_t", "void**"],
    "alch_pt_linear_free": ["void*"],
    "alch_pt_eval_lin": ["void*", "alch_buf*", "alch_buf*", "size_t", "unsigned"],
    "alch_pt_rescale": ["alch_buf*", "alch_buf*", "size_t"],
    "alch_buf_add_bcast": ["alch_buf*", "alch_buf*", "alch_buf*", "size_t", "size_t"],
}


def test_header_library_binding_and_haskell_agree():
    from alchemy_amd import capi
    from test_haskell_shim import CTYPE, haskell_imports, header_prototypes
    protos, imps, lib = header_prototypes(), haskell_imports(), capi.load_library()
    for name, params in ENTRY.items():
        assert protos.get(name) == ("int", params), (name, protos.get(name))
        assert name in capi.SYMBOLS and hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == len(params) and getattr(lib, name).restype is C.c_int
        safety, sig = imps[name]
        assert safety == "safe" and sig == [CTYPE[p] for p in params] + ["IO CInt"], (name, sig)
    assert lib.alch_version() == (1 << 16) | 8                        # added within 1.8: hosts probe for the symbols


def test_package_exports_the_plaintext_functions():
    import alchemy_amd as A
    from alchemy_amd import plaintext
    for name in ("pt_mul", "pt_linear", "pt_eval_lin", "pt_rescale", "add_bcast", "ring_round_plain", "coeff_bound", "PtLinear"):
        assert getattr(A, name) is getattr(plaintext, name)


def test_argument_checks_come_before_any_device_work():
    """Null handles give ALCH_E_INVALID and a message on a machine without a GPU; freeing a null linear function is ALCH_OK; a ring
    cannot be made without a device (ALCH_E_NO_DEVICE), so no later status is reachable there."""
    from alchemy_amd import capi
    lib = capi.load_library()
    assert lib.alch_pt_mul(None, None, None, None, 1, 0) == capi.ALCH_E_INVALID and lib.alch_last_error()
    h = C.c_void_p()
    assert lib.alch_pt_linear_create(None, None, 128, C.byref(h)) == capi.ALCH_E_INVALID and not h.value
    assert lib.alch_pt_linear_create(None, None, 128, None) == capi.ALCH_E_INVALID
    assert lib.alch_pt_linear_free(None) == capi.ALCH_OK
    assert lib.alch_pt_eval_lin(None, None, None, 1, 0) == capi.ALCH_E_INVALID
    assert lib.alch_pt_rescale(None, None, 1) == capi.ALCH_E_INVALID
    assert lib.alch_buf_add_bcast(None, None, None, 0, 1) == capi.ALCH_E_INVALID
    lo, hi = C.c_uint64(), C.c_uint64()
    assert lib.alch_pt_bound(448, 32, 1, None, None) == capi.ALCH_E_INVALID
    assert lib.alch_pt_bound(448, 1 << 31, 1, C.byref(lo), C.byref(hi)) == capi.ALCH_E_INVALID        # p < 2^31
    assert lib.alch_pt_bound(448, 32, 0, C.byref(lo), C.byref(hi)) == capi.ALCH_E_INVALID
    r = C.c_void_p()
    rc = lib.alch_ring_create_nocrt(448, 1, (C.c_uint64 * 1)(32), C.byref(r))
    assert rc in (capi.ALCH_E_NO_DEVICE, capi.ALCH_OK)                # the only way to a non-null handle needs the device
    if rc == capi.ALCH_OK:
        lib.alch_ring_destroy(r)


def phi(m):
    return G.Index(m).n


def odd_primes(m):
    return sum(1 for p, _ in G.Index(m).pps if p != 2)


@pytest.mark.parametrize("m,p,terms", [(448, 32, 1), (448, 32, 2), (91, 7, 6), (45, 2, 1), (28, 4, 3), (32, 32, 1), (4, 7, 1), (20475, 32, 8)])
def test_bound_formula(m, p, terms):
    from alchemy_amd import plaintext
    assert plaintext.coeff_bound(m, p, terms) == terms * phi(m) * 2 ** odd_primes(m) * (p // 2) ** 2


@pytest.mark.parametrize("m", [28, 45, 91, 448])
def test_bound_covers_every_exact_coefficient(m):
    """Python integers throughout (ring_mul_def with modulus None): the all-p/2 element against itself and random sign patterns of
    magnitude p/2, as sums of up to 6 products."""
    from alchemy_amd import plaintext
    idx, rng = G.Index(m), random.Random(m)
    for p in (32, 7):
        h = p // 2
        worst = [h] * idx.n
        prods = [G.ring_mul_def(worst, worst, idx, None), G.ring_mul_def(worst, [-h] * idx.n, idx, None)]
        for _ in range(4):
            a = [rng.choice((-h, h)) for _ in range(idx.n)]
            b = [rng.choice((-h, h)) for _ in range(idx.n)]
            prods.append(G.ring_mul_def(a, b, idx, None))
        for d_rel in range(1, 7):
            # the largest coefficient a d_rel-term sum of these products can have: every term contributing its own maximum
            peak = sum(sorted((max(abs(c) for c in pr) for pr in prods), reverse=True)[:d_rel])
            total = [sum(pr[k] for pr in prods[:d_rel]) for k in range(idx.n)]
            bound = plaintext.coeff_bound(m, p, d_rel)
            assert peak <= bound and max(abs(c) for c in total) <= bound, (m, p, d_rel)
