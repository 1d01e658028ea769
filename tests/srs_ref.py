"""A plain reference for the structured reference string: the Lagrange-basis scalars in Python integers and the two point sets through
the oracle's double-and-add (oracle.binding.g1_mul).  Nothing here touches the device, the device's MSM or its NTT.

    g[i]  = [s^i] G
    gl[i] = [c_i] G,   c_i = L_i(s) = (1/n) * sum_{j<n} (s * w^-i)^j  (mod r),   w = ROOT^(2^(28-k)),  n = 2^k

The sum is the definition of the i-th Lagrange polynomial of the 2^k-point domain evaluated at s (its coefficients are w^(-ij) / n): it
divides by nothing that depends on s, so a secret inside the domain (s^n = 1) needs no special case.  Past k = 10 the sum costs too much
(n^2 products) and the closed form (s^n - 1) w^i / (n (s - w^i)) takes over, with the in-domain secrets answered explicitly;
tests/test_srs_reference_cpu.py holds the two against each other and against the oracle's g1_to_lagrange."""
from concurrent.futures import ThreadPoolExecutor
import numpy as np
from conftest import R, Q, MONT, fe_from_int as fe, rand_fr
from oracle import binding as ob

ROOT = pow(7, (R - 1) >> 28, R)                       # a primitive 2^28-th root of unity of Fr (halo2curves' ROOT_OF_UNITY)
G = np.frombuffer((MONT % Q).to_bytes(32, "little") + (2 * MONT % Q).to_bytes(32, "little"), np.uint64).copy()      # (1, 2)
SUM_MAX_K = 10


def fes(xs, mod=R):
    """canonical integers -> (len, 4) Montgomery u64"""
    return np.frombuffer(b"".join((x % mod * MONT % mod).to_bytes(32, "little") for x in xs), np.uint64).reshape(-1, 4).copy()


def omega(k):
    return pow(ROOT, 1 << (28 - k), R)


def lagrange_scalars_sum(s, k):
    n, winv, ninv = 1 << k, pow(omega(k), -1, R), pow(1 << k, -1, R)
    out, x = [], s % R                                # x = s * w^-i
    for _ in range(n):
        acc, p = 0, 1
        for _ in range(n):
            acc += p
            p = p * x % R
        out.append(acc % R * ninv % R)
        x = x * winv % R
    return out


def lagrange_scalars_closed(s, k):
    n, w, s = 1 << k, omega(k), s % R
    in_domain = pow(s, n, R) == 1
    f = (pow(s, n, R) - 1) * pow(n, -1, R) % R
    out, wi = [], 1
    for _ in range(n):
        if wi == s:
            out.append(1)
        elif in_domain:
            out.append(0)
        else:
            out.append(f * wi % R * pow(s - wi, -1, R) % R)
        wi = wi * w % R
    return out


def lagrange_scalars(s, k):
    """[L_i(s) for i < 2^k] as canonical integers"""
    return lagrange_scalars_sum(s, k) if k <= SUM_MAX_K else lagrange_scalars_closed(s, k)


def power_scalars(s, n):
    out, p = [], 1
    for _ in range(n):
        out.append(p)
        p = p * s % R
    return out


def _threads():
    return max(1, min(16, ob.effective_cpus()))


def mul_many(base, scalars):
    """[[c] base for c in scalars] through the oracle, (len, 8) u64 (ctypes drops the GIL during the call: threads do run side by side)"""
    sc = fes(scalars)
    out = np.empty((len(scalars), 8), np.uint64)

    def work(lo):
        for i in range(lo, min(lo + 64, len(scalars))):
            out[i] = ob.g1_mul(base, sc[i])
    with ThreadPoolExecutor(_threads()) as ex:
        list(ex.map(work, range(0, len(scalars), 64)))
    return out


_powers, _lagrange = {}, {}


def powers_set(s, k):
    """g[i] = [s^i] G for i < 2^k (cached per (s, k); treat as read-only)"""
    if (s, k) not in _powers:
        a = mul_many(G, power_scalars(s, 1 << k))
        a.setflags(write=False)
        _powers[(s, k)] = a
    return _powers[(s, k)]


def structured_set(s, k):
    """(g, gl) of the 2^k-point SRS with secret s (cached per (s, k); treat as read-only)"""
    if (s, k) not in _lagrange:
        a = mul_many(G, lagrange_scalars(s, k))
        a.setflags(write=False)
        _lagrange[(s, k)] = a
    return powers_set(s, k), _lagrange[(s, k)]


def neg(p):
    """-P of an affine point (8 x u64); the identity stays (0, 0)"""
    o = np.array(p, np.uint64)
    y = int.from_bytes(o[4:].tobytes(), "little")
    o[4:] = np.frombuffer(((Q - y) % Q).to_bytes(32, "little"), np.uint64)
    return o


def functional_check(g, gl, k, seed):
    """commit_lagrange(v) == commit(iNTT v) on the host, for three seeded uniform v: for a uniform v a single wrong point of gl (or a
    gl that is the Lagrange basis of other points than g) changes the left side alone.  The complement of the row comparisons."""
    rng = np.random.default_rng(seed)
    for _ in range(3):
        v = rand_fr(rng, 1 << k)
        if not (ob.msm(v, gl) == ob.msm(ob.lagrange_to_coeff(v, k), g)).all():
            return False
    return True
