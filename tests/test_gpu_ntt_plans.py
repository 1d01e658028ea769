"""GPU parity of the NTT (ezkl_amd/csrc/ntt.hip) with the oracle over the WHOLE output, byte for byte, for what tests/test_gpu_ntt.py leaves
out: the default plans it skips (forward, scaled inverse, the natural-order coset pair), strided and grouped batches, words at and above
the modulus on every path that takes 256-bit input, and the EZKL_NTT_MAXR variants (each in a child process: the variable is read once).
The plans these cases are written for are pinned, without a GPU, by tests/test_ntt_plan_cpu.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
from conftest import ROOT, json_lines, rand_fr
from ntt_inputs import edge_column, sentinel, to_coset_major
from oracle import binding as ob

pytestmark = pytest.mark.gpu


def _columns(rng, n, both=True):
    """[(raw, reduced)]: a random column and one that carries the edge words"""
    cols = []
    if both:
        a = rand_fr(rng, n)
        cols.append((a, a))
    cols.append(edge_column(rng, n))
    return cols


# ---- default plans: forward and scaled inverse ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [15, 19, 21, 23])
def test_forward_whole_output(hip, k):
    """8+7, 7+6+6, 7+7+7, 8+8+7 (2^23: the edge column only, one oracle transform)"""
    rng = np.random.default_rng(4100 + k)
    w = ob.omega(k)
    for raw, red in _columns(rng, 1 << k, both=k < 23):
        assert (hip.ntt(raw, k, w) == ob.fft(red, k, w)).all()


@pytest.mark.parametrize("k", [12, 14, 15, 16, 18, 19, 20, 21, 23])
def test_scaled_inverse_whole_output(hip, k):
    """the product by 1 / n and the conditional subtraction after it in the last pass, for every default radix multiset up to 2^21 and 2^23"""
    rng = np.random.default_rng(4200 + k)
    d = hip.EvaluationDomain(2, k)
    for raw, red in _columns(rng, 1 << k, both=k < 23):
        assert (d.lagrange_to_coeff(raw) == ob.lagrange_to_coeff(red, k)).all()


# ---- the natural-order coset pair -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,ek", [(10, 11), (11, 12), (12, 13), (13, 15), (15, 17)])
def test_coset_pair_natural_order(hip, k, ek):
    """coeff_to_extended (zeta^(i mod 3) on the way in, zero padding from 2^k), divide_by_vanishing on its output, extended_to_coeff
    (zeta^-(i mod 3) / n on the way out) out of place and in place: single -> single pass, single -> two, two -> two with
    ext_k = k + 1, two -> three"""
    from ezkl_amd import backend as B
    rng = np.random.default_rng(4300 + 32 * k + ek)
    n, ne = 1 << k, 1 << ek
    for (raw, red), (eraw, ered) in zip(_columns(rng, n), _columns(rng, ne)):
        din = B.DeviceBuffer.from_numpy(raw)
        dext = B.DeviceBuffer.from_numpy(sentinel(ne))
        B.coset_ntt_dev(din.ptr, dext.ptr, k, ek)
        ext = dext.to_numpy(shape=(ne, 4))
        assert (ext == ob.coeff_to_extended(red, k, ek)).all()
        assert (din.to_numpy(shape=(n, 4)) == raw).all()                              # the input stays as it was
        B.divide_by_vanishing_dev(dext.ptr, k, ek)
        assert (dext.to_numpy(shape=(ne, 4)) == ob.divide_by_vanishing(ext, k, ek)).all()
        # the inverse: of evaluations that carry the edge words, and of the extended column just computed
        for e_in, e_red in ((eraw, ered), (ext, ext)):
            want = ob.extended_to_coeff(e_red, ek)
            dsrc = B.DeviceBuffer.from_numpy(e_in)
            dout = B.DeviceBuffer.from_numpy(sentinel(ne))
            B.coset_ntt_dev(dsrc.ptr, dout.ptr, k, ek, inverse=True)
            assert (dout.to_numpy(shape=(ne, 4)) == want).all()
            assert (dsrc.to_numpy(shape=(ne, 4)) == e_in).all()
            B.coset_ntt_dev(dsrc.ptr, dsrc.ptr, k, ek, inverse=True)                  # in == out
            assert (dsrc.to_numpy(shape=(ne, 4)) == want).all()
        back = ob.extended_to_coeff(ext, ek)
        assert (back[:n] == red).all() and not back[n:].any()                         # the oracle's own round trip: the reference is sane


# ---- batch layouts --------------------------------------------------------------------------------------------------------------------
def _strided(cols, stride, salt):
    """the columns `stride` words apart in a buffer of sentinel words; returns (buffer, mask of the gap words)"""
    buf = sentinel(len(cols) * stride, salt)
    gap = np.ones(len(buf), bool)
    for b, c in enumerate(cols):
        buf[b * stride:b * stride + len(c)] = c
        gap[b * stride:b * stride + len(c)] = False
    return buf, gap


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("k", [9, 13, 17])
def test_strided_batch_in_place(hip, k, inverse):
    """ezkl_hip_ntt_dev, three columns 2^k + 5 words apart (one, two and three passes): the five words after each column -- the last
    included -- are not touched"""
    from ezkl_amd import backend as B
    rng = np.random.default_rng(4400 + 2 * k + inverse)
    n, batch, stride = 1 << k, 3, (1 << k) + 5
    cols = [_columns(rng, n, both=False)[0] if b == 1 else (rand_fr(rng, n),) * 2 for b in range(batch)]
    buf, gap = _strided([raw for raw, _ in cols], stride, 17)
    d = hip.EvaluationDomain(2, k)
    dbuf = B.DeviceBuffer.from_numpy(buf)
    B.ntt_dev(dbuf.ptr, k, d.omega_inv if inverse else d.omega, inverse=inverse, batch=batch, stride=stride)
    got = dbuf.to_numpy(shape=buf.shape)
    for b, (_, red) in enumerate(cols):
        want = ob.lagrange_to_coeff(red, k) if inverse else ob.fft(red, k, ob.omega(k))
        assert (got[b * stride:b * stride + n] == want).all(), b
    assert gap.sum() == 5 * batch and (got[gap] == buf[gap]).all()


@pytest.mark.parametrize("k,ek,inverse", [(9, 11, False), (12, 14, False), (12, 14, True)], ids=["forward-9-11", "forward-12-14", "inverse-14"])
def test_strided_batch_coset(hip, k, ek, inverse):
    """ezkl_hip_coset_ntt_dev, three columns, input and output strides larger than the columns by different odd numbers"""
    from ezkl_amd import backend as B
    rng = np.random.default_rng(4500 + 32 * k + ek + inverse)
    nin, nout, batch = 1 << (ek if inverse else k), 1 << ek, 3
    in_stride, out_stride = nin + 3, nout + 7
    cols = [_columns(rng, nin, both=False)[0] if b == 1 else (rand_fr(rng, nin),) * 2 for b in range(batch)]
    ibuf, _ = _strided([raw for raw, _ in cols], in_stride, 29)
    obuf, ogap = _strided([np.zeros((nout, 4), np.uint64)] * batch, out_stride, 31)
    din, dout = B.DeviceBuffer.from_numpy(ibuf), B.DeviceBuffer.from_numpy(obuf)
    B.coset_ntt_dev(din.ptr, dout.ptr, k, ek, inverse=inverse, batch=batch, in_stride=in_stride, out_stride=out_stride)
    got = dout.to_numpy(shape=obuf.shape)
    for b, (_, red) in enumerate(cols):
        want = ob.extended_to_coeff(red, ek) if inverse else ob.coeff_to_extended(red, k, ek)
        assert (got[b * out_stride:b * out_stride + nout] == want).all(), b
    assert ogap.sum() == 7 * batch and (got[ogap] == obuf[ogap]).all()
    assert (din.to_numpy(shape=ibuf.shape) == ibuf).all()                             # input columns and their gaps stay as they were


def _mod7(rng, n, batch):
    """`batch` columns, column j = base column j mod 7: seven is coprime to the group size, so an offset error at the second group of a
    batch lands on a column with another expectation"""
    base = [rand_fr(rng, n) for _ in range(7)]
    reps = -(-batch // 7)
    return base, np.tile(np.stack(base), (reps, 1, 1))[:batch]


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
def test_batch_past_one_group_ntt(hip, inverse):
    """ntt_run transforms at most 32768 columns per launch: 32769 columns of 2^3 make it take a second group"""
    from ezkl_amd import backend as B
    k, batch = 3, 32769
    rng = np.random.default_rng(4600 + inverse)
    base, data = _mod7(rng, 1 << k, batch)
    d = hip.EvaluationDomain(2, k)
    dbuf = B.DeviceBuffer.from_numpy(data)
    B.ntt_dev(dbuf.ptr, k, d.omega_inv if inverse else d.omega, inverse=inverse, batch=batch)
    got = dbuf.to_numpy(shape=data.shape)
    for r in range(7):
        want = ob.lagrange_to_coeff(base[r], k) if inverse else ob.fft(base[r], k, ob.omega(k))
        assert (got[r::7] == want).all(), r


@pytest.mark.parametrize("first,n_cosets,batch", [(0, 4, 8193), (2, 2, 16385)], ids=["all-cosets", "range"])
def test_batch_past_one_group_coset_major(hip, first, n_cosets, batch):
    """coset_cm_run launches at most 32768 (column, coset) pairs at a time: 8193 columns x 4 cosets, and 16385 columns x a range of 2"""
    from ezkl_amd import backend as B
    k, ek = 3, 5
    n = 1 << k
    rng = np.random.default_rng(4700 + n_cosets)
    base, data = _mod7(rng, n, batch)
    din = B.DeviceBuffer.from_numpy(data)
    dout = B.DeviceBuffer.from_numpy(sentinel(batch * n_cosets * n, 41))
    if n_cosets == 4:
        B.coeff_to_cosets_dev(din.ptr, dout.ptr, k, ek, batch=batch)
    else:
        B.coeff_to_cosets_range_dev(din.ptr, dout.ptr, k, ek, first, n_cosets, batch=batch)
    got = dout.to_numpy(shape=(batch, n_cosets * n, 4))
    for r in range(7):
        want = to_coset_major(ob.coeff_to_extended(base[r], k, ek), k, ek)[first * n:(first + n_cosets) * n]
        assert (got[r::7] == want).all(), r


# ---- the EZKL_NTT_MAXR variants: one child process per value --------------------------------------------------------------------------
CHILD = r'''
import json, os, sys
root = os.environ["EZKL_ROOT"]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import numpy as np
import ezkl_amd
from ezkl_amd import backend as B
from conftest import rand_fr
from ntt_inputs import edge_column, sentinel, to_coset_major
from oracle import binding as ob
spec = json.loads(sys.argv[1])
ezkl_amd.init()
# the variable took effect, and every case runs the plan (radices and workgroup sizes = kernel instances) it is meant for
for log_n, (radices, threads) in sorted((int(k), v) for k, v in spec["plans"].items()):
    p = B.ntt_plan_info(log_n, 0)
    assert (p["max_radix"], p["log_radix"], p["threads"]) == (spec["in_force"], radices, threads), (log_n, p)
print(json.dumps({"case": "plans", "log_n": 0, "equal": True}), flush=True)

def report(case, log_n, equal):
    print(json.dumps({"case": case, "log_n": log_n, "equal": bool(equal)}), flush=True)

def columns(rng, n, both):
    a = rand_fr(rng, n)
    return ([(a, a)] if both else []) + [edge_column(rng, n)]

for log_n in spec["sizes"]:
    rng = np.random.default_rng(4800 + log_n)
    n, both = 1 << log_n, log_n <= 20
    d = ezkl_amd.EvaluationDomain(2, log_n)
    w = ob.omega(log_n)
    cols = columns(rng, n, both)
    report("forward", log_n, all((ezkl_amd.ntt(raw, log_n, w) == ob.fft(red, log_n, w)).all() for raw, red in cols))
    report("inverse", log_n, all((d.lagrange_to_coeff(raw) == ob.lagrange_to_coeff(red, log_n)).all() for raw, red in cols))
    k = log_n - 2                                           # natural order: 2^k coefficients -> 2^log_n evaluations -> coefficients
    ok_ext, ok_back = True, True
    for raw, red in columns(rng, 1 << k, both):
        din, dext = B.DeviceBuffer.from_numpy(raw), B.DeviceBuffer.from_numpy(sentinel(n))
        B.coset_ntt_dev(din.ptr, dext.ptr, k, log_n)
        ext = dext.to_numpy(shape=(n, 4))
        ok_ext &= bool((ext == ob.coeff_to_extended(red, k, log_n)).all())
        B.coset_ntt_dev(dext.ptr, dext.ptr, k, log_n, inverse=True)
        ok_back &= bool((dext.to_numpy(shape=(n, 4)) == ob.extended_to_coeff(ext, log_n)).all())
        din.free(); dext.free()
    report("coeff_to_extended", log_n, ok_ext)
    report("extended_to_coeff", log_n, ok_back)
    if log_n in spec["coset_major"]:                        # E = 4 transforms of 2^log_n points, two columns
        ek = log_n + 2
        polys = [rand_fr(rng, n), edge_column(rng, n)]
        din = B.DeviceBuffer.from_numpy(np.stack([polys[0], polys[1][0]]))
        dout = B.DeviceBuffer.from_numpy(sentinel(2 << ek))
        B.coeff_to_cosets_dev(din.ptr, dout.ptr, log_n, ek, batch=2)
        got = dout.to_numpy(shape=(2, 1 << ek, 4))
        ok = True
        for b, red in enumerate((polys[0], polys[1][1])):
            ok &= bool((got[b] == to_coset_major(ob.coeff_to_extended(red, log_n, ek), log_n, ek)).all())
        report("coset_major", log_n, ok)
        din.free(); dout.free()
'''

R256 = ([256, 256], [256] * 3, [256] * 4)
# EZKL_NTT_MAXR -> the value in force, the sizes, the plan (radices, workgroup sizes) of every size, and the sizes the coset-major case runs at
# (2^log_n points per coset, ext_k = log_n + 2; where that passes 2^22 the smaller size of the row stands in)
VARIANTS = {
    "6": dict(in_force=6, sizes=[13, 19, 20], plans={13: ([5, 4, 4], R256[1]), 19: ([5, 5, 5, 4], R256[2]), 20: ([5, 5, 5, 5], R256[2])}, coset_major=[13, 19, 20]),
    "7": dict(in_force=7, sizes=[15, 22], plans={15: ([5, 5, 5], R256[1]), 22: ([6, 6, 5, 5], R256[2])}, coset_major=[15]),
    "9": dict(in_force=9, sizes=[17, 18], plans={17: ([9, 8], [512, 256]), 18: ([9, 9], [512, 512])}, coset_major=[17, 18]),
    "10": dict(in_force=10, sizes=[19, 20], plans={19: ([10, 9], [1024, 512]), 20: ([10, 10], [1024, 1024])}, coset_major=[19, 20]),
    "11": dict(in_force=11, sizes=[21, 22], plans={21: ([11, 10], [512, 1024]), 22: ([11, 11], [512, 512])}, coset_major=[21]),
    # out of range: 8 stays in force
    "5": dict(in_force=8, sizes=[13], plans={13: ([7, 6], R256[0])}, coset_major=[13]),
    "12": dict(in_force=8, sizes=[13], plans={13: ([7, 6], R256[0])}, coset_major=[13]),
    "junk": dict(in_force=8, sizes=[13], plans={13: ([7, 6], R256[0])}, coset_major=[13]),
}
# a stop for a hang, not a performance assertion: a child starts the library, builds the twiddle tables of its sizes and spends at most a
# few seconds in the oracle
CHILD_TIMEOUT = 180
_child_died = []                      # a child ended by a signal or by the timeout: no later variant starts a process


@pytest.mark.parametrize("value", list(VARIANTS))
def test_max_radix_variant(hip, value):
    assert not _child_died, "an earlier EZKL_NTT_MAXR child (%s) was killed: not starting another" % _child_died[0]
    spec = VARIANTS[value]
    env = dict(os.environ, EZKL_ROOT=ROOT, EZKL_NTT_MAXR=value)
    try:
        r = subprocess.run([sys.executable, "-c", CHILD, json.dumps(spec)], env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        _child_died.append(value)
        pytest.fail("EZKL_NTT_MAXR=%s: the child did not end in %d s\n%s" % (value, CHILD_TIMEOUT, (e.stderr or b"")[-3000:]))
    if r.returncode < 0:
        _child_died.append(value)
    assert r.returncode == 0, "EZKL_NTT_MAXR=%s: exit %d\n%s\n%s" % (value, r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    got = {(j["case"], j["log_n"]): j["equal"] for j in json_lines(r.stdout)}
    want = {("plans", 0)}
    for log_n in spec["sizes"]:
        want |= {(c, log_n) for c in ("forward", "inverse", "coeff_to_extended", "extended_to_coeff")}
    want |= {("coset_major", log_n) for log_n in spec["coset_major"]}
    assert set(got) == want
    assert all(got.values()), sorted(k for k, v in got.items() if not v)
