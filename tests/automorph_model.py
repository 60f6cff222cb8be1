"""The slot permutation of a Galois automorphism sigma_j : zeta_m -> zeta_m^j on the CRT basis, restated from the slot rule at the
top of include/alchemy_hip.h in Python integers -- no library call, no table of the library.

    crt(sigma_j a)[slot(u)] = (sigma_j a)(omega^u) = a(omega^(u j)) = crt(a)[slot(u j mod m)]

    m = prod_l p_l^e_l, primes ascending, first factor outermost in the slot index; on the axis of p^e, with m' = p^(e-1),
    slot s = (i0 - 1) m' + digitrev_p(i1) holds the unit u = i0 + p i1 (mod p^e); a two-power index: slot k holds 2 brev(k) + 1.

table(m, j)[k] is the SOURCE slot of destination slot k.  Also: sigma_j on powerful-basis coefficients of a two-power ring (the
substitution X -> X^j with X^n = -1) and of any index (through the oracle's reduction of zeta_m^t to the powerful basis)."""
import math


def factor(m):
    out, p = [], 2
    while m > 1:
        if m % p == 0:
            e = 0
            while m % p == 0:
                m //= p
                e += 1
            out.append((p, e))
        p += 1
    return out


def digitrev(x, p, digits):
    r = 0
    for _ in range(digits):
        r, x = r * p + x % p, x // p
    return r


def axis_unit(p, e, s):
    mp = p ** (e - 1)
    return (s // mp + 1 + p * digitrev(s % mp, p, e - 1)) % p ** e


def axis_dims(m):
    return [(p - 1) * p ** (e - 1) for p, e in factor(m)]


def phi(m):
    return math.prod(axis_dims(m))


def units(m):
    return [j for j in range(1, m + 1) if math.gcd(j, m) == 1] if m > 1 else [1]


def slot_unit(m, k, _f=None):
    """The unit u of Z_m^* whose evaluation omega_m^u slot k holds: Chinese remaindering of the per-axis units."""
    f = _f or factor(m)
    dims = [(p - 1) * p ** (e - 1) for p, e in f]
    digits = []
    for d in reversed(dims):
        digits.append(k % d)
        k //= d
    digits.reverse()
    u, mod = 0, 1
    for (p, e), s in zip(f, digits):
        ml = p ** e
        ul = axis_unit(p, e, s)
        u += mod * ((ul - u) * pow(mod, -1, ml) % ml)
        mod *= ml
    return u % m if m > 1 else 0


def table(m, j):
    """[source slot of destination slot k for k < phi(m)], by the definition: the slot that holds the unit u(k) j mod m."""
    assert math.gcd(j, m) == 1
    n, f = phi(m), factor(m)
    us = [slot_unit(m, k, f) for k in range(n)]
    where = {u: k for k, u in enumerate(us)}
    assert len(where) == n
    return [where[u * j % m] for u in us]


def sigma_pow_twopower(a, j, q=None):
    """sigma_j on the coefficient vector of Z[X]/(X^n + 1): X^i -> X^(i j), X^n = -1."""
    n = len(a)
    out = [0] * n
    for i, x in enumerate(a):
        t = i * j % (2 * n)
        out[t % n] += -x if t >= n else x
    return [x % q for x in out] if q else out


def sigma_pow(a, idx, j, q=None):
    """sigma_j on powerful-basis coefficients of any index: p_i = zeta_m^e(i) goes to zeta_m^(e(i) j), reduced to the powerful basis
    by the oracle's by-definition rule (oracle/model_gen.py, read only)."""
    from oracle import model_gen as G
    acc = {}
    for i, x in enumerate(a):
        t = idx.pow_exponent(i) * j % idx.m
        acc[t] = acc.get(t, 0) + int(x)
    return G._reduce_to_pow(acc, idx, q)
