"""Plain references and input builders for tests/test_gpu_lookup_copy_edges.py: the mv-lookup multiplicity column, the mock prover's
miss and copy reports, and keys that collide in the device hash table.

Everything expected comes from dicts and sets keyed by the 32 stored bytes of an element (multiplicity, miss_records) or from one numpy
comparison (copy_bad).  colliding_keys and slot know the shape of the device hash (csrc/vecops.hip: ht_hash); they build INPUTS only."""
import numpy as np
from conftest import R, fe_from_int


def table_cap(usable):
    """slots of the device hash table, as lookup_multiplicity_batch sizes it: the smallest power of two >= 16 and >= 2 * usable"""
    cap = 16
    while cap < 2 * usable:
        cap <<= 1
    return cap


def multiplicity(table, inputs, n_rows, usable):
    """(counts[n_rows], missing): every input value on a usable row counts on the FIRST usable table row that holds it, or is missing"""
    first = {}
    for i in range(usable):
        first.setdefault(table[i].tobytes(), i)
    counts, missing = np.zeros(n_rows, np.int64), 0
    for x in inputs:
        for r in range(usable):
            i = first.get(x[r].tobytes())
            if i is None:
                missing += 1
            else:
                counts[i] += 1
    return counts, missing


def miss_records(tables, inputs_per_lookup, usable):
    """{(lookup, input, row)}: the usable input rows whose value is on no usable row of their argument's table"""
    out = set()
    for l, (table, inputs) in enumerate(zip(tables, inputs_per_lookup)):
        have = {table[i].tobytes() for i in range(usable)}
        out |= {(l, s, r) for s, x in enumerate(inputs) for r in range(usable) if x[r].tobytes() not in have}
    return out


def counts_to_fr(counts):
    """the (n, 4) u64 Montgomery column of an integer column: the words the device must write"""
    out = np.zeros((len(counts), 4), np.uint64)
    for v in np.unique(counts):
        out[counts == v] = fe_from_int(int(v))
    return out


def copy_bad(cols, nxt, log_n):
    """{(column, row)}: the cells of cols (m, n, 4) whose stored words differ from their successor's; a successor outside the m columns
    is bad without being read"""
    m, n = cols.shape[0], 1 << log_n
    flat = cols.reshape(m * n, 4)
    nxt = nxt.astype(np.int64)
    outside = nxt >= m * n
    bad = outside | (flat != flat[np.where(outside, 0, nxt)]).any(axis=1)
    return {(int(t) >> log_n, int(t) & (n - 1)) for t in np.nonzero(bad)[0]}


def _words(keys):
    return np.ascontiguousarray(keys, np.uint64).reshape(-1, 4).view(np.uint32).reshape(-1, 8)


def slot(keys, cap):
    """the first slot the device probes for each stored element (ht_hash over the eight little-endian 32-bit words that ld_fe in
    csrc/field.hpp loads in memory order).  For AIMING only: it places a collision chain at a chosen slot, such as cap - 1.  Every
    expected value comes from the dict reference above, so a changed device hash loses the aim of these cases, not their correctness."""
    w = _words(keys)
    h = w[:, 0] * np.uint32(0x9e3779b1) ^ w[:, 1] * np.uint32(0x85ebca77) ^ w[:, 2] * np.uint32(0xc2b2ae3d) \
        ^ w[:, 3] * np.uint32(0x27d4eb2f) ^ w[:, 5] * np.uint32(0x165667b1) ^ w[:, 7]
    h ^= h >> np.uint32(15)
    return h & np.uint32(cap - 1)


def colliding_keys(count, base_words, first=0):
    """`count` stored elements (count, 4) u64 that differ only in 32-bit words 4 and 6 -- the two words the device hash does not read --,
    numbered from `first`, so that disjoint ranges give disjoint keys.  Word 7 of base_words is far below r's top word 0x30644e72, so
    every key is a stored value below r."""
    base = np.asarray(base_words, np.uint32)
    assert base.shape == (8,) and int(base[7]) < 0x20000000
    w = np.tile(base, (count, 1))
    j = np.arange(first, first + count, dtype=np.uint64)
    w[:, 4] = (j & np.uint64(0xffffffff)).astype(np.uint32)
    w[:, 6] = (j * np.uint64(0x9e3779b1) >> np.uint64(7) & np.uint64(0xffffffff)).astype(np.uint32)
    keys = w.view(np.uint64).reshape(count, 4)
    assert all(int.from_bytes(k.tobytes(), "little") < R for k in keys[:: max(1, count // 8)])
    return keys


def aim(base_words, cap, want_slot):
    """base_words with word 0 replaced by the smallest value that sends the keys of colliding_keys to want_slot"""
    base = np.asarray(base_words, np.uint32).copy()
    tries = np.tile(base, (1 << 18, 1))
    tries[:, 0] = np.arange(1 << 18, dtype=np.uint32)
    hit = np.nonzero(slot(tries.view(np.uint64).reshape(-1, 4), cap) == want_slot)[0]
    assert len(hit), "no word 0 below 2^18 reaches slot %d of %d" % (want_slot, cap)
    base[0] = hit[0]
    return base
