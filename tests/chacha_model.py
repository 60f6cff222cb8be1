"""Python model of the keyed ChaCha20 streams (include/alchemy_hip.h, "keyed streams"), written from the definition
and vectorised over blocks with numpy uint32: nothing here calls the library.

    blocks(key, nonce, counters)            the 16 words of each block
    pairs(key, nonce, domain, xs)           (A, B) of each position
    uniform(key, nonce, domain, xs, q)      (B 2^64 + A) mod q as Python integers
    gauss_dec(...), c1_words(...)           what alch_buf_gauss_dec / alch_ct_encrypt / alch_ct_ks_hint store under a key"""
import numpy as np

import gauss_model as GM

U32, U64 = np.uint32, np.uint64
CONST = (0x61707865, 0x3320646e, 0x79622d32, 0x6b206574)
DOM_GAUSS, DOM_ENCRYPT, DOM_HINT = 1, 2, 3
X_END = 1 << 58


def _rotl(x, r):
    return (x << U32(r)) | (x >> U32(32 - r))


def _qr(s, a, b, c, d):
    s[a] = s[a] + s[b]; s[d] = _rotl(s[d] ^ s[a], 16)
    s[c] = s[c] + s[d]; s[b] = _rotl(s[b] ^ s[c], 12)
    s[a] = s[a] + s[b]; s[d] = _rotl(s[d] ^ s[a], 8)
    s[c] = s[c] + s[d]; s[b] = _rotl(s[b] ^ s[c], 7)


def blocks(key: bytes, nonce: int, counters) -> np.ndarray:
    """counters: integers below 2^64.  Returns uint32 (len(counters), 16): output = working state + input state."""
    assert len(key) == 32
    ctr = np.array([int(c) for c in np.asarray(counters, dtype=object).ravel()], dtype=U64)
    k = np.frombuffer(bytes(key), dtype="<u4")
    init = [np.full(ctr.shape, v, dtype=U32) for v in CONST] + [np.full(ctr.shape, v, dtype=U32) for v in k]
    init += [(ctr & U64(0xFFFFFFFF)).astype(U32), (ctr >> U64(32)).astype(U32),
             np.full(ctr.shape, nonce & 0xFFFFFFFF, dtype=U32), np.full(ctr.shape, (nonce >> 32) & 0xFFFFFFFF, dtype=U32)]
    s = [v.copy() for v in init]
    with np.errstate(over="ignore"):
        for _ in range(10):
            _qr(s, 0, 4, 8, 12); _qr(s, 1, 5, 9, 13); _qr(s, 2, 6, 10, 14); _qr(s, 3, 7, 11, 15)
            _qr(s, 0, 5, 10, 15); _qr(s, 1, 6, 11, 12); _qr(s, 2, 7, 8, 13); _qr(s, 3, 4, 9, 14)
        return np.stack([a + b for a, b in zip(s, init)], axis=1)


def pairs(key: bytes, nonce: int, domain: int, xs):
    """xs: positions (Python integers or a uint64 array), each below 2^58.  Returns (A, B) as uint64 arrays."""
    xs = np.asarray(xs, dtype=U64).ravel()
    assert 0 <= domain < 256 and (xs.size == 0 or int(xs.max()) < X_END)
    blk = xs >> U64(2)
    ub, inv = np.unique(blk, return_inverse=True)
    w = blocks(key, nonce, [(domain << 56) | int(b) for b in ub]).astype(U64)
    u64 = w[:, 0::2] | (w[:, 1::2] << U64(32))                                  # (blocks, 8)
    s = (xs & U64(3)).astype(np.int64)
    return u64[inv, 2 * s], u64[inv, 2 * s + 1]


def uniform(key: bytes, nonce: int, domain: int, xs, q: int):
    """(B 2^64 + A) mod q for every position, as a list of Python integers."""
    A, B = pairs(key, nonce, domain, xs)
    return [((int(b) << 64) | int(a)) % q for a, b in zip(A, B)]


def odd_positions(pair0: int, count: int, L: int, n: int) -> np.ndarray:
    """x of word (pair b, limb j, slot k), shape (count, L, n): ((2 (pair0 + b) + 1) L + j) n + k."""
    b = np.arange(count, dtype=object).reshape(count, 1, 1) + pair0
    j = np.arange(L, dtype=object).reshape(1, L, 1)
    k = np.arange(n, dtype=object).reshape(1, 1, n)
    return ((2 * b + 1) * L + j) * n + k


def c1_words(key: bytes, nonce: int, domain: int, pair0: int, count: int, qs, n: int) -> np.ndarray:
    """The odd elements of `count` pairs from pair counter pair0 on, in the library's download layout (count, n, L), dtype object."""
    L = len(qs)
    pos = odd_positions(pair0, count, L, n)
    out = np.empty((count, n, L), dtype=object)
    for j, q in enumerate(qs):
        out[:, :, j] = np.array(uniform(key, nonce, domain, [int(x) for x in pos[:, j, :].ravel()], q), dtype=object).reshape(count, n)
    return out


def raw(key: bytes, m: int, svar: float, nonce: int, elem0: int, count: int) -> np.ndarray:
    """gauss_model.raw with the two words of coefficient c taken from the pair of position c, domain 1."""
    n, scale, axes = GM.plan(m, svar)
    c = [elem0 * n + i for i in range(count * n)]
    w0, w1 = pairs(key, nonce, DOM_GAUSS, np.array(c, dtype=U64))
    x = (GM.deviate(w0, w1).astype(np.float64) * np.float64(scale)).reshape(count, n)
    for p, mp, stride, Lc in axes:
        h = p - 1
        X = x.reshape(count, n // (h * mp * stride), h, mp * stride)
        Y = np.empty_like(X)
        for i in range(h):
            s = np.zeros_like(X[:, :, 0, :])
            for k in range(i + 1):
                t = np.float64(Lc[i][k]) * X[:, :, k, :]
                s = s + t
            Y[:, :, i, :] = s
        x = Y.reshape(count, n)
    return x


def gauss_dec(key: bytes, m: int, svar: float, nonce: int, elem0: int, count: int, p=None, coset=None) -> np.ndarray:
    """The integers z, shape (count, n) int64 (gauss_model.gauss_dec's rounding)."""
    x = raw(key, m, svar, nonce, elem0, count)
    if p is None:
        return GM.round_half_away(x)
    v = np.asarray(coset, dtype=np.int64).reshape(x.shape)
    c = np.where(v > (p - 1) // 2, v - p, v)
    return c + p * GM.round_half_away((x - c.astype(np.float64)) / np.float64(p))
