"""Python model of the counter-based error sampler (include/alchemy_hip.h, "encrypt on resident batches"), written from
the definition and vectorised with numpy uint64 / float64: a few hundred thousand deviates take about a second.  Every float operation
is one numpy (or Python float) operation, so each is rounded on its own, as the definition demands; nothing here calls the library.

    table(), splitmix64(), plan(m, svar), raw(...) (the doubles before rounding), gauss_dec(...) (the integers z), words(z, qs)"""
import math
from decimal import Decimal, getcontext
from functools import lru_cache

import numpy as np

M64 = (1 << 64) - 1
U = np.uint64


@lru_cache(maxsize=None)
def table():
    """T[t] = floor(2^63 P(|K| <= t)), K ~ D_{Z,64}, up to and including the first entry >= 2^63 - 1."""
    getcontext().prec = 100
    rho = [(-(Decimal(t) * Decimal(t)) / Decimal(8192)).exp() for t in range(6000)]
    total = rho[0] + 2 * sum(rho[1:], Decimal(0))
    out, acc, t = [], rho[0], 0
    while True:
        v = int((Decimal(1 << 63) * acc / total).to_integral_value(rounding="ROUND_FLOOR"))
        out.append(v)
        if v >= (1 << 63) - 1:
            return tuple(out)
        t += 1
        acc += 2 * rho[t]


def splitmix64(x):
    """numpy uint64 array -> numpy uint64 array (wrapping arithmetic)."""
    with np.errstate(over="ignore"):
        x = x + U(0x9E3779B97F4A7C15)
        x = (x ^ (x >> U(30))) * U(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> U(27))) * U(0x94D049BB133111EB)
        return x ^ (x >> U(31))


def splitmix64_int(x: int) -> int:
    return int(splitmix64(np.array([x & M64], dtype=U))[0])


def factor(m):
    f, p = [], 2
    while m > 1:
        if p * p > m:
            p = m
        if m % p == 0:
            e = 0
            while m % p == 0:
                m //= p
                e += 1
            f.append((p, e))
        p += 1
    return f


def totient(m):
    n = 1
    for p, e in factor(m):
        n *= (p - 1) * p ** (e - 1)
    return n


def cholesky(p):
    """Lower Cholesky factor of p I - J, (p-1) x (p-1), every operation rounded on its own (Python floats)."""
    h = p - 1
    L = [[0.0] * h for _ in range(h)]
    for i in range(h):
        for j in range(i + 1):
            s = float(p) - 1.0 if i == j else -1.0
            for k in range(j):
                t = L[i][k] * L[j][k]
                s = s - t
            L[i][j] = math.sqrt(s) if i == j else s / L[j][j]
    return L


def plan(m, svar):
    """(n, scale, axes): axes = [(p, m_p', stride, Lc)] for the odd primes of m, ascending."""
    fs = factor(m)
    rad = 1
    for p, _ in fs:
        rad *= p
    n = totient(m)
    sigma = math.sqrt(svar * float(m // rad) / (2.0 * math.pi))
    scale = sigma / (math.sqrt(4096.0 + 1.0 / 12.0) * 4294967296.0)
    axes, stride = [], n
    for p, e in fs:
        mp = p ** (e - 1)
        stride //= (p - 1) * mp
        if p != 2:
            axes.append((p, mp, stride, cholesky(p)))
    return n, scale, axes


def deviate(w0, w1):
    """The scalar deviate f of two 64-bit words (numpy uint64 arrays) as int64."""
    T = np.array(table(), dtype=U)
    t = np.searchsorted(T, w0 >> U(1), side="right").astype(np.int64)          # #{ j : T[j] <= u }
    k = np.where((w0 & U(1)) == U(1), -t, t)
    return k * (1 << 32) + (w1 >> U(32)).astype(np.int64) - (1 << 31)


def raw(m, svar, seed, elem0, count):
    """The doubles x after the correlation, shape (count, n)."""
    n, scale, axes = plan(m, svar)
    with np.errstate(over="ignore"):
        c = U((elem0 * n) & M64) + np.arange(count * n, dtype=U)
        a = U(seed & M64) + U(2) * c
        f = deviate(splitmix64(a), splitmix64(a + U(1)))
    x = (f.astype(np.float64) * np.float64(scale)).reshape(count, n)
    for p, mp, stride, Lc in axes:
        h = p - 1
        X = x.reshape(count, n // (h * mp * stride), h, mp * stride)           # column entries along axis 2
        Y = np.empty_like(X)
        for i in range(h):
            s = np.zeros_like(X[:, :, 0, :])
            for k in range(i + 1):
                t = np.float64(Lc[i][k]) * X[:, :, k, :]
                s = s + t
            Y[:, :, i, :] = s
        x = Y.reshape(count, n)
    return x


def round_half_away(x):
    r = np.floor(np.abs(x) + 0.5).astype(np.int64)
    return np.where(x < 0, -r, r)


def gauss_dec(m, svar, seed, elem0, count, p=None, coset=None):
    """The integers z, shape (count, n) int64.  coset: (count, n) residues in [0, p)."""
    x = raw(m, svar, seed, elem0, count)
    if p is None:
        return round_half_away(x)
    v = np.asarray(coset, dtype=np.int64).reshape(x.shape)
    c = np.where(v > (p - 1) // 2, v - p, v)
    return c + p * round_half_away((x - c.astype(np.float64)) / np.float64(p))


def words(z, qs):
    """(count, n) integers -> (count, n, L) residues in [0, q_j) (the library's download layout)."""
    return np.stack([np.mod(z, np.int64(q)) for q in qs], axis=2).astype(np.int64)


def bits(x: float) -> int:
    return int(np.array([x], dtype=np.float64).view(U)[0])
