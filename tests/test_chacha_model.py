"""CPU: the keyed ChaCha20 streams -- known answers through the public addressing, for the Python model
(tests/chacha_model.py) and for the library's host-only entry point alch_rng_words, and the two against each other."""
import ctypes as C

import numpy as np
import pytest

import alchemy_amd
from alchemy_amd import capi
import chacha_model as CM

KEY_RFC = bytes(range(32))
# RFC 8439 section 2.3.2: key 00 .. 1f, counter 1, nonce 00 00 00 09 00 00 00 4a 00 00 00 00.  In the original layout the words 12 .. 15
# are (1, 0x09000000, 0x4a000000, 0): block counter 0x0900000000000001 = domain 9, x = 4 .. 7, and nonce 0x000000004a000000.
RFC_BLOCK = ("e4e7f110 15593bd1 1fdd0f50 c47120a3 c7f4d1c7 0368c033 9aaa2204 4e6cd4c3 "
             "466482d2 09aa9f07 05d7c214 a2028bd9 d19c12b5 b94e16de e883d0cb 4e3c50a2")
RFC_WORDS = [int(w, 16) for w in RFC_BLOCK.split()]
RFC_NONCE, RFC_DOMAIN = 0x000000004A000000, 9


def lib_words(key, nonce, domain, x0, count):
    lib = alchemy_amd.load_library()
    out = (C.c_uint64 * max(1, 2 * count))()
    capi._check(lib.alch_rng_words(key, nonce, domain, x0, count, out))
    a = np.array(out[:2 * count], dtype=np.uint64).reshape(count, 2)
    return a[:, 0], a[:, 1]


def rfc_pairs():
    u64 = [RFC_WORDS[2 * t] | RFC_WORDS[2 * t + 1] << 32 for t in range(8)]
    return u64[0::2], u64[1::2]


def test_model_rfc8439_block_through_the_addressing():
    assert [int(w) for w in CM.blocks(KEY_RFC, RFC_NONCE, [0x0900000000000001])[0]] == RFC_WORDS
    A, B = CM.pairs(KEY_RFC, RFC_NONCE, RFC_DOMAIN, [4, 5, 6, 7])
    ea, eb = rfc_pairs()
    assert [int(a) for a in A] == ea and [int(b) for b in B] == eb
    assert int(A[0]) == 0x15593BD1E4E7F110 and int(B[0]) == 0xC47120A31FDD0F50


def test_model_zero_key_blocks():
    w = CM.blocks(bytes(32), 0, [0, 1])
    assert w[0, :4].astype("<u4").tobytes().hex() == "76b8e0ada0f13d90405d6ae55386bd28"
    assert w[1, :2].astype("<u4").tobytes().hex() == "9f07e7be5551387a"


def test_library_rfc8439_and_zero_key():
    A, B = lib_words(KEY_RFC, RFC_NONCE, RFC_DOMAIN, 4, 4)
    ea, eb = rfc_pairs()
    assert [int(a) for a in A] == ea and [int(b) for b in B] == eb
    A, B = lib_words(bytes(32), 0, 0, 0, 5)
    first = np.array([A[0], B[0]], dtype="<u8").tobytes().hex()
    assert first == "76b8e0ada0f13d90405d6ae55386bd28"
    assert np.array([A[4]], dtype="<u8").tobytes().hex() == "9f07e7be5551387a"


@pytest.mark.parametrize("domain", [0, 1, 2, 3, 255])
@pytest.mark.parametrize("x0,count", [(0, 9), (1, 1), (2, 5), (3, 6), (7, 2), ((1 << 40) + 1, 11), ((1 << 58) - 6, 6)])
def test_library_equals_model(domain, x0, count):
    key = bytes((7 * i + 3) & 255 for i in range(32))
    nonce = 0xFEDCBA9876543210
    A, B = lib_words(key, nonce, domain, x0, count)
    ma, mb = CM.pairs(key, nonce, domain, [x0 + i for i in range(count)])
    assert np.array_equal(A, ma) and np.array_equal(B, mb)


def test_domains_and_nonces_separate_the_streams():
    key = bytes(range(1, 33))
    seen = {tuple(int(v) for v in np.concatenate(lib_words(key, 5, d, 0, 4))) for d in (1, 2, 3)}
    seen |= {tuple(int(v) for v in np.concatenate(lib_words(key, 6, 1, 0, 4)))}
    assert len(seen) == 4


def test_last_position_and_the_refusals():
    lib = alchemy_amd.load_library()
    key = bytes(range(32))
    A, B = lib_words(key, 1, 3, (1 << 58) - 1, 1)
    ma, mb = CM.pairs(key, 1, 3, [(1 << 58) - 1])
    assert int(A[0]) == int(ma[0]) and int(B[0]) == int(mb[0])
    out = (C.c_uint64 * 4)()
    assert lib.alch_rng_words(key, 1, 3, (1 << 58) - 1, 2, out) == capi.ALCH_E_INVALID
    assert lib.alch_rng_words(key, 1, 3, 1 << 58, 1, out) == capi.ALCH_E_INVALID
    assert lib.alch_rng_words(key, 1, 3, (1 << 64) - 1, 2, out) == capi.ALCH_E_INVALID      # x0 + count does not wrap
    assert lib.alch_rng_words(key, 1, 256, 0, 1, out) == capi.ALCH_E_INVALID
    assert lib.alch_rng_words(None, 1, 3, 0, 1, out) == capi.ALCH_E_INVALID
    assert lib.alch_rng_words(key, 1, 3, 0, 1, None) == capi.ALCH_E_INVALID
    assert lib.alch_rng_words(key, 1, 3, 1 << 58, 0, None) == capi.ALCH_OK                  # nothing asked for, nothing past the end


def test_symbols_and_constants():
    lib = alchemy_amd.load_library()
    for s in ("alch_ring_set_rng_key", "alch_ring_rng", "alch_rng_words"):
        assert s in capi.SYMBOLS and hasattr(lib, s)
    assert (capi.ALCH_RNG_SPLITMIX, capi.ALCH_RNG_CHACHA20) == (0, 1)
    assert lib.alch_version() == (1 << 16) | 8
