"""Host-side mirror of the reference interface for the prove hot path, on top of the C ABI.

Names follow halo2 (the reference's proving stack):
  ParamsKZG.commit_lagrange / commit      <- halo2_proofs::poly::kzg::commitment::ParamsKZG (A10;
                                             call site /root/reference/src/circuit/modules/polycommit.rs:71)
  EvaluationDomain.{lagrange_to_coeff, coeff_to_lagrange, coeff_to_extended, extended_to_coeff,
                    divide_by_vanishing_poly}  <- halo2_proofs::poly::EvaluationDomain (A11)
  GraphProgram.evaluate_h                 <- plonk::evaluation::GraphEvaluator / evaluate_h (A12)
All field data are numpy uint64 arrays (..., 4) in Montgomery form = the bytes halo2 holds in memory.
"""
import ctypes as C
import numpy as np
from . import lib as _l

_vp = C.c_void_p


def _p(a):
    return a.ctypes.data_as(_vp)


def _fe(a, shape_last=4):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.shape[-1] != shape_last:
        raise ValueError("expected trailing dimension %d" % shape_last)
    return a


def init(device=-1):
    _l.check(_l.load().ezkl_hip_init(C.c_int(device)), "ezkl_hip_init")


def synchronize():
    _l.check(_l.load().ezkl_hip_synchronize(), "ezkl_hip_synchronize")


def device_count():
    return int(_l.load().ezkl_hip_device_count())


def _stream_ptr(stream):
    return _vp(stream) if stream else _vp(None)


class DeviceBuffer:
    """A library-owned HBM allocation (resident column / scalar vector)."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        p = _vp()
        _l.check(_l.load().ezkl_hip_malloc(C.byref(p), C.c_size_t(self.nbytes)), "ezkl_hip_malloc")
        self.ptr = p.value

    @classmethod
    def from_numpy(cls, a):
        a = np.ascontiguousarray(a)
        b = cls(a.nbytes)
        _l.check(_l.load().ezkl_hip_memcpy_h2d(_vp(b.ptr), _p(a), C.c_size_t(a.nbytes)), "h2d")
        return b

    def to_numpy(self, dtype=np.uint64, shape=None):
        out = np.empty(self.nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        _l.check(_l.load().ezkl_hip_memcpy_d2h(_p(out), _vp(self.ptr), C.c_size_t(self.nbytes)), "d2h")
        return out.reshape(shape) if shape is not None else out

    def words(self, first, count=1):
        """`count` 32-byte words from word `first` on: (count, 4) uint64 -- a few cells of a resident column without the column"""
        if not 0 <= first <= first + count <= self.nbytes // 32:
            raise ValueError("words %d .. %d of a buffer of %d" % (first, first + count, self.nbytes // 32))
        out = np.empty((count, 4), np.uint64)
        _l.check(_l.load().ezkl_hip_memcpy_d2h(_p(out), _vp(self.ptr + 32 * first), C.c_size_t(32 * count)), "d2h")
        return out

    def free(self):
        if self.ptr:
            _l.load().ezkl_hip_free(_vp(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceView:
    """a window of another resident buffer (no ownership): .ptr / .nbytes like DeviceBuffer, keeps its parent alive"""

    def __init__(self, ptr, nbytes, parent):
        self.ptr, self.nbytes, self._parent = ptr, nbytes, parent


class PinnedArray:
    """a numpy view of page-locked host memory (ezkl_hip_host_malloc): witness columns filled here upload at PCIe speed"""

    def __init__(self, shape, dtype=np.uint64):
        self.nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self._p = _vp()
        _l.check(_l.load().ezkl_hip_host_malloc(C.byref(self._p), C.c_size_t(self.nbytes)), "ezkl_hip_host_malloc")
        buf = (C.c_uint8 * max(1, self.nbytes)).from_address(self._p.value)
        self.array = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def free(self):
        if self._p:
            self.array = None
            _l.load().ezkl_hip_host_free(self._p)
            self._p = None


class _Bases:
    def __init__(self, pts):
        pts = _fe(pts, 8)
        self.n = pts.shape[0]
        h = _vp()
        _l.check(_l.load().ezkl_hip_bases_upload(_p(pts), C.c_size_t(self.n), C.byref(h)), "ezkl_hip_bases_upload")
        self.h = h

    @classmethod
    def generate(cls, seed, n, first=0):
        self = cls.__new__(cls)
        self.n = n
        h = _vp()
        _l.check(_l.load().ezkl_hip_bases_generate(C.c_uint64(seed), C.c_size_t(first), C.c_size_t(n), C.byref(h)),
                 "ezkl_hip_bases_generate")
        self.h = h
        return self

    @classmethod
    def from_scalars(cls, base_point, scalars_ptr, n):
        """bases[i] = scalars[i] * base_point (SRS generation)"""
        self = cls.__new__(cls)
        self.n = n
        h = _vp()
        _l.check(_l.load().ezkl_hip_bases_from_scalars(_p(_fe(base_point, 8)), _vp(scalars_ptr), C.c_size_t(n), C.byref(h)),
                 "ezkl_hip_bases_from_scalars")
        self.h = h
        return self

    def downsize(self, new_k):
        """halo2 ParamsKZG::downsize on a coefficient-basis set: (first 2^new_k points, Lagrange basis of the 2^new_k domain) as new
        resident base sets -- the Lagrange basis is an inverse NTT over G1 on the device (ezkl_hip_bases_downsize)"""
        hg, hl = _vp(), _vp()
        _l.check(_l.load().ezkl_hip_bases_downsize(self.h, C.c_uint32(new_k), C.byref(hg), C.byref(hl)), "ezkl_hip_bases_downsize")
        out = []
        for h in (hg, hl):
            b = type(self).__new__(type(self))
            b.n, b.h = 1 << new_k, h
            out.append(b)
        return tuple(out)

    def mul_scalars(self, scalars_ptr, first=0, n=None):
        """a new resident set of n points, out[i] = scalars[i] * self[first + i], for n resident Montgomery scalars: the per-row product
        of an SRS update (ezkl_hip_bases_mul_scalars).  Reads the resident records; builds no window table; self is unchanged."""
        n = self.n - first if n is None else n
        h = _vp()
        _l.check(_l.load().ezkl_hip_bases_mul_scalars(self.h, _vp(scalars_ptr), C.c_size_t(first), C.c_size_t(n), C.byref(h)),
                 "ezkl_hip_bases_mul_scalars")
        b = type(self).__new__(type(self))
        b.n, b.h = n, h
        return b

    def download(self):
        out = np.empty((self.n, 8), np.uint64)
        _l.check(_l.load().ezkl_hip_bases_download(self.h, _p(out)), "ezkl_hip_bases_download")
        return out

    def check(self, first=0, n=None):
        """is every record in [first, first + n) a point of G1, as halo2's raw-bytes reader decides it (ezkl_hip_bases_check)?  ->
        dict(bad: how many are not, first_bad: the smallest such index in the set or None, reason: 1 x >= q / 2 y >= q / 3 off the curve
        (0: none), identities: all-zero records, which are valid).  Reads the resident records; builds no window table."""
        n = self.n - first if n is None else n
        out = np.zeros(4, np.uint64)
        _l.check(_l.load().ezkl_hip_bases_check(self.h, C.c_size_t(first), C.c_size_t(n), _p(out)), "ezkl_hip_bases_check")
        bad = int(out[0])
        return dict(bad=bad, first_bad=int(out[1]) if bad else None, reason=int(out[2]), identities=int(out[3]))

    def prepare(self):
        """start the window-table precompute now, without waiting (ezkl_hip_bases_prepare)"""
        _l.check(_l.load().ezkl_hip_bases_prepare(self.h), "ezkl_hip_bases_prepare")
        return self

    def has_table(self):
        """does the handle have a window table, built or being built (ezkl_hip_bases_has_table)?"""
        return bool(_l.load().ezkl_hip_bases_has_table(self.h))

    def msm(self, scalars_ptr, first=0, n=None, stream=None):
        """sum_i scalars[i] * self[first + i] over n resident Montgomery scalars, fixed-base: builds the window tables at first use"""
        return msm_g1_dev(self, scalars_ptr, self._count(first, n), first, stream)

    def msm_once(self, scalars, first=0, n=None, stream=None):
        """the same point WITHOUT window tables (ezkl_hip_msm_g1_once_dev): none is read, built or kept -- for a set that serves a few MSMs
        and is freed.  `scalars`: a device pointer (or a DeviceBuffer) of n resident Montgomery scalars."""
        n = self._count(first, n)
        out = np.zeros(8, np.uint64)
        _l.check(_l.load().ezkl_hip_msm_g1_once_dev(self.h, C.c_size_t(first), _vp(getattr(scalars, "ptr", scalars)), C.c_size_t(n), _p(out),
                                                     _stream_ptr(stream)), "ezkl_hip_msm_g1_once_dev")
        return out

    def _count(self, first, n):
        first = int(first)
        n = self.n - first if n is None else int(n)
        if first < 0 or n < 0 or first + n > self.n:
            raise ValueError("records [%d, %d) of a set of %d points" % (first, first + n, self.n))
        return n

    def free(self):
        if self.h:
            _l.load().ezkl_hip_bases_free(self.h)
            self.h = None


Bases = _Bases

# Below this many points a set that is used once still builds its tables (0: the table-free path wins at every measured size, 2^16 and 2^20:
# profiles/r15_msm_once.json, DESIGN.md §4.1 "MSM without window tables").  check_srs, execute.gen_witness and pk_recommit read it.
MSM_ONCE_MIN_POINTS = 0


def msm_used_once(bases, scalars_ptr, n, offset=0):
    """an MSM on a set that will serve a few MSMs and be freed: table-free from MSM_ONCE_MIN_POINTS points on"""
    if n and n >= MSM_ONCE_MIN_POINTS:
        return bases.msm_once(scalars_ptr, offset, n)
    return msm_g1_dev(bases, scalars_ptr, n, offset)


def msm_points(points_dev, scalars_dev, n, stream=None):
    """sum_i scalars[i] * points[i] over n resident 64-byte affine Montgomery records that are no base set (ezkl_hip_msm_g1_points_dev)"""
    out = np.zeros(8, np.uint64)
    _l.check(_l.load().ezkl_hip_msm_g1_points_dev(_vp(getattr(points_dev, "ptr", points_dev)), _vp(getattr(scalars_dev, "ptr", scalars_dev)),
                                                   C.c_size_t(int(n)), _p(out), _stream_ptr(stream)), "ezkl_hip_msm_g1_points_dev")
    return out


def msm_g1_dev(bases, scalars_ptr, n, offset=0, stream=None):
    out = np.zeros(8, np.uint64)
    _l.check(_l.load().ezkl_hip_msm_g1_dev(bases.h, C.c_size_t(offset), _vp(scalars_ptr), C.c_size_t(n), _p(out),
                                            _stream_ptr(stream)), "ezkl_hip_msm_g1_dev")
    return out


def msm_g1_start_dev(bases, scalars_ptr, n, offset=0):
    """the first half of msm_g1_dev: queues the MSM on a call slot of its own and returns a token (ezkl_hip_msm_g1_start_dev; at most four in
    flight per context -- a fifth from the thread that holds all four raises EzklHipError with code EZKL_ERR_BUSY = -6)"""
    tok = C.c_int(-1)
    _l.check(_l.load().ezkl_hip_msm_g1_start_dev(bases.h, C.c_size_t(offset), _vp(scalars_ptr), C.c_size_t(n), C.byref(tok)), "ezkl_hip_msm_g1_start_dev")
    return int(tok.value)


def msm_g1_finish(token):
    """waits for the MSM behind `token` and returns its affine point; a token is spent by its first finish"""
    out = np.zeros(8, np.uint64)
    _l.check(_l.load().ezkl_hip_msm_g1_finish(C.c_int(token), _p(out)), "ezkl_hip_msm_g1_finish")
    return out


def msm_g1_batch_dev(bases, scalar_ptrs, n, offset=0, stream=None):
    """batch of MSMs over resident scalar vectors (one commit phase); returns (batch, 8) affine points"""
    out = np.zeros((len(scalar_ptrs), 8), np.uint64)
    arr = (C.c_void_p * len(scalar_ptrs))(*scalar_ptrs)
    _l.check(_l.load().ezkl_hip_msm_g1_batch_dev(bases.h, C.c_size_t(offset), arr, C.c_size_t(len(scalar_ptrs)), C.c_size_t(n),
                                                  _p(out), _stream_ptr(stream)), "ezkl_hip_msm_g1_batch_dev")
    return out


class MsmBatch:
    """incremental commit batch: push resident columns one at a time (uploads of the next column overlap the MSMs of
    the previous ones), finish() -> (count, 8) affine points"""

    def __init__(self, bases, n, offset=0):
        self.h = _vp()
        self.count = 0
        _l.check(_l.load().ezkl_hip_msm_batch_begin(bases.h, C.c_size_t(offset), C.c_size_t(n), C.byref(self.h)), "ezkl_hip_msm_batch_begin")

    def push(self, scalars_ptr):
        _l.check(_l.load().ezkl_hip_msm_batch_push_dev(self.h, _vp(scalars_ptr)), "ezkl_hip_msm_batch_push_dev")
        self.count += 1

    def push_many(self, scalar_ptrs):
        """several columns at once (fused into groups like a one-call batch); returns once their MSMs are queued"""
        arr = (C.c_void_p * max(1, len(scalar_ptrs)))(*[_vp(p) for p in scalar_ptrs])
        _l.check(_l.load().ezkl_hip_msm_batch_push_many_dev(self.h, arr, C.c_size_t(len(scalar_ptrs))), "ezkl_hip_msm_batch_push_many_dev")
        self.count += len(scalar_ptrs)

    def finish(self, capacity=None):
        cap = self.count if capacity is None else capacity
        out = np.zeros((max(cap, 1), 8), np.uint64)
        h, self.h = self.h, None
        _l.check(_l.load().ezkl_hip_msm_batch_finish(h, _p(out), C.c_size_t(cap)), "ezkl_hip_msm_batch_finish")
        return out[:self.count]


class Stream:
    """a caller stream for the `stream=` arguments (pass `.ptr`): work queued on it is asynchronous until synchronize()"""

    def __init__(self):
        p = _vp()
        _l.check(_l.load().ezkl_hip_stream_create(C.byref(p)), "ezkl_hip_stream_create")
        self.ptr = p.value

    def synchronize(self):
        _l.check(_l.load().ezkl_hip_stream_synchronize(_vp(self.ptr)), "ezkl_hip_stream_synchronize")

    def free(self):
        if self.ptr:
            _l.check(_l.load().ezkl_hip_stream_destroy(_vp(self.ptr)), "ezkl_hip_stream_destroy")
            self.ptr = None


class UploadPhase:
    """upload_commit_batch in steps (ezkl_hip_upload_begin / _wait / _commit / _end): the copies are queued by the
    constructor; wait(j, stream) orders a caller stream behind column j; commit(bases) returns the (batch, 8) points;
    end() closes the phase.  The host columns are kept alive until end()."""

    def __init__(self, host_cols, tails=None, tail_start=0):
        self.cols = [np.ascontiguousarray(a, np.uint64) for a in host_cols]
        self.n = self.cols[0].shape[0]
        self.devs = [DeviceBuffer(32 * self.n) for _ in self.cols]
        m = len(self.cols)
        hp = (C.c_void_p * m)(*[a.ctypes.data for a in self.cols])
        dp = (C.c_void_p * m)(*[d.ptr for d in self.devs])
        tp, tcount, self._tails = None, 0, []
        if tails is not None:
            self._tails = [np.ascontiguousarray(t, np.uint64) for t in tails]
            tcount = self._tails[0].shape[0]
            tp = (C.c_void_p * m)(*[t.ctypes.data for t in self._tails])
        self.h = _vp()
        _l.check(_l.load().ezkl_hip_upload_begin(hp, dp, C.c_size_t(m), C.c_size_t(self.n), tp, C.c_size_t(tail_start), C.c_size_t(tcount), C.byref(self.h)),
                 "ezkl_hip_upload_begin")

    def wait(self, j, stream):
        _l.check(_l.load().ezkl_hip_upload_wait(self.h, C.c_size_t(j), _vp(stream.ptr if isinstance(stream, Stream) else stream)), "ezkl_hip_upload_wait")

    def commit(self, bases, commit_range=None):
        lo, hi = commit_range if commit_range is not None else (0, self.n)
        out = np.zeros((len(self.cols), 8), np.uint64)
        _l.check(_l.load().ezkl_hip_upload_commit(self.h, bases.h, C.c_size_t(lo), C.c_size_t(hi - lo), _p(out)), "ezkl_hip_upload_commit")
        return out

    def end(self):
        if self.h:
            h, self.h = self.h, None
            _l.check(_l.load().ezkl_hip_upload_end(h), "ezkl_hip_upload_end")


def upload_commit_batch(bases, host_cols, tails=None, tail_start=0, commit_range=None):
    """one prover phase: upload the host columns ((n,4) u64 arrays, ideally PinnedArray views), overwrite rows
    [tail_start, tail_start + t) of column j with tails[j] ((t,4) arrays), commit each (commit_range = (lo, hi): only rows [lo, hi)
    against bases [0, hi - lo), a rank's slice of a sharded SRS).  Returns (device columns, (batch, 8) points)."""
    cols = [np.ascontiguousarray(a, np.uint64) for a in host_cols]
    n = cols[0].shape[0]
    devs = [DeviceBuffer(32 * n) for _ in cols]
    hp = (C.c_void_p * len(cols))(*[a.ctypes.data for a in cols])
    dp = (C.c_void_p * len(cols))(*[d.ptr for d in devs])
    tp, tcount, keep = None, 0, []
    if tails is not None:
        keep = [np.ascontiguousarray(t, np.uint64) for t in tails]
        tcount = keep[0].shape[0]
        tp = (C.c_void_p * len(cols))(*[t.ctypes.data for t in keep])
    out = np.zeros((len(cols), 8), np.uint64)
    lo, hi = commit_range if commit_range is not None else (0, n)
    _l.check(_l.load().ezkl_hip_upload_commit_batch(bases.h, hp, dp, C.c_size_t(len(cols)), C.c_size_t(n), tp, C.c_size_t(tail_start), C.c_size_t(tcount),
                                                    C.c_size_t(lo), C.c_size_t(hi - lo), _p(out)), "ezkl_hip_upload_commit_batch")
    return devs, out


def msm_g1(bases, scalars):
    """sum_i scalars[i]*bases[i]; scalars numpy (n,4) or a DeviceBuffer-resident vector via msm_dev."""
    s = _fe(scalars)
    out = np.zeros(8, np.uint64)
    _l.check(_l.load().ezkl_hip_msm_g1(bases.h, _p(s), C.c_size_t(s.shape[0]), _p(out)), "ezkl_hip_msm_g1")
    return out


class ParamsKZG:
    """KZG SRS with both base sets resident in HBM (g: coefficient basis, g_lagrange: Lagrange basis)."""

    def __init__(self, k, g, g_lagrange):
        self.k, self.n = k, 1 << k
        self._g = _Bases(g)
        self._gl = _Bases(g_lagrange)

    @classmethod
    def from_bases(cls, k, g, g_lagrange):
        """around two base sets that are resident already (and are this object's to free from here on)"""
        self = cls.__new__(cls)
        self.k, self.n, self._g, self._gl = k, 1 << k, g, g_lagrange
        return self

    @classmethod
    def read(cls, buf):
        """raw-bytes SRS file: u32 LE k | 2^k G1 g | 2^k G1 g_lagrange | g2 | s_g2 (SURVEY.md §8(c) item 1;
        the reader being mirrored is /root/reference/src/pfsys/srs.rs:40-47 -> ParamsKZG::read)."""
        k = int.from_bytes(buf[0:4], "little")
        n = 1 << k
        if len(buf) != 4 + 2 * 64 * n + 256:
            raise ValueError("bad SRS length")
        g = np.frombuffer(buf, np.uint64, count=8 * n, offset=4).reshape(n, 8)
        gl = np.frombuffer(buf, np.uint64, count=8 * n, offset=4 + 64 * n).reshape(n, 8)
        return cls(k, g, gl)

    def downsize(self, new_k):
        """ParamsKZG::downsize (halo2; /root/reference/src/execute.rs:1739-1750 calls it whenever the SRS file is larger than the circuit):
        truncate g, rebuild g_lagrange for the smaller domain (an inverse NTT over G1, on the device).  In place, like halo2's."""
        if new_k > self.k:
            raise ValueError("cannot downsize a k=%d SRS to k=%d" % (self.k, new_k))
        if new_k == self.k:
            return self
        g, gl = self._g.downsize(new_k)
        self._g.free(); self._gl.free()
        self._g, self._gl, self.k, self.n = g, gl, new_k, 1 << new_k
        return self

    def commit_lagrange(self, poly):
        """MSM against g_lagrange; returns the canonical affine point (8 x u64). Blind is ignored by KZG."""
        return msm_g1(self._gl, poly)

    def commit(self, poly):
        return msm_g1(self._g, poly)

    def commit_dev(self, scalars_dev, n, lagrange=True, offset=0, stream=None):
        out = np.zeros(8, np.uint64)
        b = self._gl if lagrange else self._g
        _l.check(_l.load().ezkl_hip_msm_g1_dev(b.h, C.c_size_t(offset), _vp(scalars_dev), C.c_size_t(n), _p(out),
                                                _stream_ptr(stream)), "ezkl_hip_msm_g1_dev")
        return out

    def free(self):
        self._g.free()
        self._gl.free()


def polycommit_commit(message, num_unusable_rows, params, once=False):
    """PolyCommitChip::commit (/root/reference/src/circuit/modules/polycommit.rs:46-81): pad the message into
    ceil-ish(len / (2^k - u)) Lagrange-basis columns (num_poly = len / n + 1 as the reference computes it), leave
    the u unusable rows at Blind::default().0 (= Fr::ONE in halo2, passed here as `blind`), commit each column with
    commit_lagrange and return the normalised affine points.  The batch goes through the pipelined MSM path; once=True: `params` was
    loaded for these few columns alone (execute.gen_witness), and each is committed without window tables (msm_used_once)."""
    message = _fe(message)
    n_rows = 1 << params.k
    n = n_rows - num_unusable_rows
    num_poly = message.shape[0] // n + 1
    polys = np.zeros((num_poly, n_rows, 4), np.uint64)
    polys[:, n:, :] = _to_mont(1)                       # Blind::default() == Blind(Fr::ONE)
    for i in range(message.shape[0]):
        polys[i // n, i % n] = message[i]
    out = np.zeros((num_poly, 8), np.uint64)
    if once:
        for j in range(num_poly):
            col = DeviceBuffer.from_numpy(polys[j])
            try:
                out[j] = msm_used_once(params._gl, col.ptr, n_rows)
            finally:
                col.free()
        return out
    arr = (C.c_void_p * num_poly)(*[polys[j].ctypes.data for j in range(num_poly)])
    _l.check(_l.load().ezkl_hip_msm_g1_batch(params._gl.h, arr, C.c_size_t(num_poly), C.c_size_t(n_rows), _p(out)),
             "ezkl_hip_msm_g1_batch")
    return out


def polycommit_commit_dev(columns, length, num_unusable_rows, params):
    """PolyCommitChip::commit of a message that is RESIDENT already, laid out as a circuit's module columns hold it (VarTensor::assign
    from row 0, n = 2^k - num_unusable_rows values a column, every other usable row zero: what a witness plan's replay leaves): the
    unusable rows of each of the length // n + 1 columns are filled with Blind::default() = 1 in place (vec_fill) and the column is committed
    against g_lagrange without window tables (msm_once).  columns: DeviceBuffers of 2^k Montgomery words, at least length // n + 1 of
    them.  -> (length // n + 1, 8) affine points, the same as polycommit_commit gives for the message."""
    n_rows = 1 << params.k
    u = int(num_unusable_rows)
    if not 0 < u < n_rows:
        raise ValueError("%d unusable rows of %d" % (u, n_rows))
    n = n_rows - u
    num_poly = int(length) // n + 1
    if length < 0 or num_poly > len(columns):
        raise ValueError("a message of %d values takes %d columns of %d, got %d" % (length, num_poly, n, len(columns)))
    if any(c.nbytes < 32 * n_rows for c in columns[:num_poly]):
        raise ValueError("a column holds %d words of 32 bytes" % n_rows)
    out = np.zeros((num_poly, 8), np.uint64)
    for j in range(num_poly):
        vec_fill(columns[j].ptr + 32 * n, _to_mont(1), u)
        out[j] = params._gl.msm_once(columns[j], 0, n_rows)
    return out


def msm_g2(points, scalars):
    """sum_i scalars[i] * points[i] over G2: points (n, 16) u64 affine (x.c0, x.c1, y.c0, y.c1 Montgomery Fq, the SRS file's layout),
    scalars (n, 4) Montgomery Fr -> (16,) u64 affine (ezkl_hip_msm_g2)"""
    points, scalars = _fe(points, 16), _fe(scalars)
    if points.shape[0] != scalars.shape[0]:
        raise ValueError("one scalar per point")
    out = np.zeros(16, np.uint64)
    _l.check(_l.load().ezkl_hip_msm_g2(_p(points), _p(scalars), C.c_size_t(points.shape[0]), _p(out)), "ezkl_hip_msm_g2")
    return out


def g1_add_affine(a, b):
    a, b = _fe(a, 8), _fe(b, 8)
    out = np.zeros(8, np.uint64)
    _l.check(_l.load().ezkl_hip_g1_add_affine(_p(a), _p(b), _p(out)), "ezkl_hip_g1_add_affine")
    return out


def ntt(a, log_n, omega, inverse=False):
    """best_fft(a, omega, log_n) on a host array (copy in, transform, copy out)."""
    a = _fe(a).copy()
    w = _fe(omega)
    _l.check(_l.load().ezkl_hip_ntt(_p(a), C.c_uint32(log_n), _p(w), C.c_int(1 if inverse else 0)), "ezkl_hip_ntt")
    return a


def ntt_dev(ptr, log_n, omega, inverse=False, batch=1, stride=None, stream=None):
    w = _fe(omega)
    stride = (1 << log_n) if stride is None else stride
    _l.check(_l.load().ezkl_hip_ntt_dev(_vp(ptr), C.c_uint32(log_n), _p(w), C.c_int(1 if inverse else 0),
                                         C.c_size_t(batch), C.c_size_t(stride), _stream_ptr(stream)), "ezkl_hip_ntt_dev")


def set_async(on):
    """ezkl_hip_set_async for the calling thread: library-stream calls return once queued (True) / when done (False, which drains the
    stream).  Returns the previous setting."""
    prev = C.c_int(0)
    _l.check(_l.load().ezkl_hip_set_async(C.c_int(1 if on else 0), C.byref(prev)), "ezkl_hip_set_async")
    return bool(prev.value)


def vec_op(op, a_ptr, b_ptr, out_ptr, n, stream=None):
    code = {"add": 0, "sub": 1, "mul": 2}[op]
    _l.check(_l.load().ezkl_hip_vec_op_dev(C.c_int(code), _vp(a_ptr), _vp(b_ptr), _vp(out_ptr), C.c_size_t(n),
                                            _stream_ptr(stream)), "ezkl_hip_vec_op_dev")


def permutation_sigma_dev(next_ptr, omega_col_ptr, delta_pows_ptr, n_columns, log_n, out_ptr, stream=None):
    """out[r] = delta^(t >> log_n) * omega^(t mod 2^log_n), t = next[r]: one sigma column from the cycle successors of its cells (u32, device)"""
    _l.check(_l.load().ezkl_hip_permutation_sigma_dev(_vp(next_ptr), _vp(omega_col_ptr), _vp(delta_pows_ptr), C.c_uint32(n_columns), C.c_uint32(log_n),
                                                      _vp(out_ptr), _stream_ptr(stream)), "ezkl_hip_permutation_sigma_dev")


def vec_scale(a_ptr, scalar, out_ptr, n, stream=None):
    _l.check(_l.load().ezkl_hip_vec_scale_dev(_vp(a_ptr), _p(_fe(scalar)), _vp(out_ptr), C.c_size_t(n), _stream_ptr(stream)), "ezkl_hip_vec_scale_dev")


def vec_fill(out_ptr, value, n, stream=None):
    _l.check(_l.load().ezkl_hip_vec_fill_dev(_vp(out_ptr), _p(_fe(value)), C.c_size_t(n), _stream_ptr(stream)), "ezkl_hip_vec_fill_dev")


def coset_ntt_dev(in_ptr, out_ptr, k, ext_k, inverse=False, in_len=None, batch=1, stream=None):
    """coeff_to_extended (inverse=False: 2^k coefficients in, 2^ext_k evaluations out) / extended_to_coeff on resident columns"""
    nin = (1 << ext_k) if inverse else (1 << k)
    _l.check(_l.load().ezkl_hip_coset_ntt_dev(_vp(in_ptr), _vp(out_ptr), C.c_size_t(batch), C.c_size_t(nin), C.c_size_t(1 << ext_k),
                                               C.c_uint32(k), C.c_uint32(ext_k), C.c_int(1 if inverse else 0), _stream_ptr(stream)),
             "ezkl_hip_coset_ntt_dev")


def coeff_to_cosets_dev(in_ptr, out_ptr, k, ext_k, batch=1, stream=None):
    """coeff_to_extended with the 2^(ext_k - k) cosets of the extended domain stored one after the other (coset-major): out[b 2^k + j]
    = p(zeta w_ext^b omega^j) = natural-order element E j + b"""
    _l.check(_l.load().ezkl_hip_coeff_to_cosets_dev(_vp(in_ptr), _vp(out_ptr), C.c_size_t(batch), C.c_size_t(1 << k), C.c_size_t(1 << ext_k),
                                                     C.c_uint32(k), C.c_uint32(ext_k), _stream_ptr(stream)), "ezkl_hip_coeff_to_cosets_dev")


def coeff_to_cosets_range_dev(in_ptr, out_ptr, k, ext_k, first_coset, n_cosets, batch=1, stream=None):
    """cosets [first_coset, first_coset + n_cosets) of coeff_to_cosets_dev only (n_cosets a power of two): out[(b - first) 2^k + j]"""
    _l.check(_l.load().ezkl_hip_coeff_to_cosets_range_dev(_vp(in_ptr), _vp(out_ptr), C.c_size_t(batch), C.c_size_t(1 << k), C.c_size_t(n_cosets << k),
                                                           C.c_uint32(k), C.c_uint32(ext_k), C.c_uint32(first_coset), C.c_uint32(n_cosets), _stream_ptr(stream)),
             "ezkl_hip_coeff_to_cosets_range_dev")


def cosets_transpose_dev(in_ptr, out_ptr, k, ext_k, to_natural=True, stream=None):
    _l.check(_l.load().ezkl_hip_cosets_transpose_dev(_vp(in_ptr), _vp(out_ptr), C.c_uint32(k), C.c_uint32(ext_k), C.c_int(1 if to_natural else 0),
                                                      _stream_ptr(stream)), "ezkl_hip_cosets_transpose_dev")


def divide_by_vanishing_dev(ptr, k, ext_k, stream=None):
    _l.check(_l.load().ezkl_hip_divide_by_vanishing_dev(_vp(ptr), C.c_uint32(k), C.c_uint32(ext_k), _stream_ptr(stream)),
             "ezkl_hip_divide_by_vanishing_dev")


def memcpy_h2d(dst_ptr, arr):
    arr = np.ascontiguousarray(arr)
    _l.check(_l.load().ezkl_hip_memcpy_h2d(_vp(dst_ptr), _p(arr), C.c_size_t(arr.nbytes)), "h2d")


def memcpy_d2h(src_ptr, nbytes):
    out = np.empty(nbytes, np.uint8)
    _l.check(_l.load().ezkl_hip_memcpy_d2h(_p(out), _vp(src_ptr), C.c_size_t(nbytes)), "d2h")
    return out


def prefix_scan(op, in_ptr, out_ptr, n, exclusive=False, stream=None):
    code = {"add": 0, "mul": 2}[op]
    _l.check(_l.load().ezkl_hip_prefix_scan_dev(C.c_int(code), C.c_int(1 if exclusive else 0), _vp(in_ptr), _vp(out_ptr),
                                                 C.c_size_t(n), _stream_ptr(stream)), "ezkl_hip_prefix_scan_dev")


def lookup_multiplicity(input_ptrs, table_ptr, n_rows, usable_rows, stream=None):
    """m(X) of mv-lookup: returns (DeviceBuffer with the Fr column, number of input values missing from the table)"""
    out = DeviceBuffer(n_rows * 32)
    miss = C.c_uint32(0)
    arr = (C.c_void_p * max(1, len(input_ptrs)))(*input_ptrs)
    _l.check(_l.load().ezkl_hip_lookup_multiplicity_dev(arr, C.c_uint32(len(input_ptrs)), _vp(table_ptr), C.c_uint32(n_rows),
                                                         C.c_uint32(usable_rows), _vp(out.ptr), C.byref(miss), _stream_ptr(stream)),
             "ezkl_hip_lookup_multiplicity_dev")
    return out, int(miss.value)


def lookup_multiplicity_batch(inputs_per_lookup, table_ptrs, n_rows, usable_rows, stream=None):
    """m(X) of every lookup argument in one call: inputs_per_lookup[l] = the input column pointers of argument l.  Returns
    ([DeviceBuffer per argument], total number of input values missing from their tables)"""
    L = len(table_ptrs)
    outs = [DeviceBuffer(n_rows * 32) for _ in range(L)]
    flat = [p for ins in inputs_per_lookup for p in ins]
    which = [l for l, ins in enumerate(inputs_per_lookup) for _ in ins]
    miss = DeviceBuffer.from_numpy(np.zeros(1, np.uint32))
    a_in = (C.c_void_p * max(1, len(flat)))(*flat)
    a_which = (C.c_uint32 * max(1, len(which)))(*which)
    a_tab = (C.c_void_p * L)(*table_ptrs)
    a_out = (C.c_void_p * L)(*[o.ptr for o in outs])
    _l.check(_l.load().ezkl_hip_lookup_multiplicity_batch_dev(a_in, a_which, C.c_uint32(len(flat)), a_tab, C.c_uint32(L), C.c_uint32(n_rows), C.c_uint32(usable_rows),
                                                               a_out, _vp(miss.ptr), _stream_ptr(stream)), "ezkl_hip_lookup_multiplicity_batch_dev")
    return outs, int(miss.to_numpy(np.uint32, (1,))[0])


def _records(rec, counters, cap):
    """(records as (kind, index, sub, row) tuples -- at most cap of them, in the order the kernel appended them --, counters)"""
    cnt = counters.to_numpy(np.uint64)
    m = int(min(cnt[0], cap))
    r = rec.to_numpy(np.uint32)[:4 * m].reshape(m, 4) if m else np.zeros((0, 4), np.uint32)
    return [tuple(int(x) for x in row) for row in r], [int(x) for x in cnt]


def lookup_missing_rows(inputs_per_lookup, table_ptrs, n_rows, usable_rows, cap=1024, stream=None):
    """the mock prover's lookup check (ezkl_hip_lookup_missing_rows_dev): every usable input row absent from its table.  Returns
    (records (2, lookup, input, row), [total, misses of argument 0, ...])"""
    L = len(table_ptrs)
    flat = [p for ins in inputs_per_lookup for p in ins]
    which = [l for l, ins in enumerate(inputs_per_lookup) for _ in ins]
    rec, cnt = DeviceBuffer(max(1, cap) * 16), DeviceBuffer.from_numpy(np.zeros(1 + L, np.uint64))
    a_in = (C.c_void_p * max(1, len(flat)))(*flat)
    a_which = (C.c_uint32 * max(1, len(which)))(*which)
    a_tab = (C.c_void_p * L)(*table_ptrs)
    _l.check(_l.load().ezkl_hip_lookup_missing_rows_dev(a_in, a_which, C.c_uint32(len(flat)), a_tab, C.c_uint32(L), C.c_uint32(n_rows), C.c_uint32(usable_rows),
                                                         _vp(rec.ptr), C.c_uint32(cap), _vp(cnt.ptr), _stream_ptr(stream)), "ezkl_hip_lookup_missing_rows_dev")
    return _records(rec, cnt, cap)


def copy_check(col_ptrs, next_ptr, log_n, cap=1024, stream=None):
    """the mock prover's copy check (ezkl_hip_copy_check_dev): every cell that differs from its cycle successor.  Returns
    (records (3, column, 0, row), [total])"""
    rec, cnt = DeviceBuffer(max(1, cap) * 16), DeviceBuffer.from_numpy(np.zeros(1, np.uint64))
    a = (C.c_void_p * max(1, len(col_ptrs)))(*col_ptrs)
    _l.check(_l.load().ezkl_hip_copy_check_dev(a, C.c_uint32(len(col_ptrs)), _vp(next_ptr), C.c_uint32(log_n), _vp(rec.ptr), C.c_uint32(cap), _vp(cnt.ptr),
                                                _stream_ptr(stream)), "ezkl_hip_copy_check_dev")
    return _records(rec, cnt, cap)


def eval_polynomial(coeffs_ptr, n, x, stream=None):
    """halo2 eval_polynomial on a resident coefficient vector"""
    out = np.zeros(4, np.uint64)
    _l.check(_l.load().ezkl_hip_eval_poly_dev(_vp(coeffs_ptr), C.c_size_t(n), _p(_fe(x)), _p(out), _stream_ptr(stream)),
             "ezkl_hip_eval_poly_dev")
    return out


def eval_polynomial_batch(coeff_ptrs, n, xs, stream=None):
    """[eval_polynomial(poly_j, xs[j])] for resident polynomials, one round trip for the whole batch"""
    m = len(coeff_ptrs)
    out = np.zeros((m, 4), np.uint64)
    if m == 0:
        return out
    arr = (C.c_void_p * m)(*coeff_ptrs)
    x = _fe(np.asarray(xs, np.uint64).reshape(m, 4))
    _l.check(_l.load().ezkl_hip_eval_poly_batch_dev(arr, _p(x), C.c_uint32(m), C.c_size_t(n), _p(out), _stream_ptr(stream)), "ezkl_hip_eval_poly_batch_dev")
    return out


def lincomb(input_ptrs, coeffs, out_ptr, n, accumulate=False, stream=None):
    """out = (out if accumulate else 0) + sum_j coeffs[j] * inputs[j], fused"""
    m = len(input_ptrs)
    arr = (C.c_void_p * max(1, m))(*input_ptrs)
    cf = _fe(np.asarray(coeffs, np.uint64).reshape(m, 4)) if m else np.zeros((1, 4), np.uint64)
    _l.check(_l.load().ezkl_hip_lincomb_dev(arr, _p(cf), C.c_uint32(m), _vp(out_ptr), C.c_size_t(n), C.c_int(1 if accumulate else 0), _stream_ptr(stream)),
             "ezkl_hip_lincomb_dev")


def kate_division(a_ptr, z, out_ptr, n, stream=None):
    """out = a(X) / (X - z) without the remainder (halo2's kate_division); out may alias a"""
    _l.check(_l.load().ezkl_hip_kate_division_dev(_vp(a_ptr), _p(_fe(z)), _vp(out_ptr), C.c_size_t(n), _stream_ptr(stream)), "ezkl_hip_kate_division_dev")


def chacha20_fr(key32, stream_id, out_ptr, n, first=0, stream=None):
    """n uniform Fr elements of ChaCha20 stream `stream_id` under the 32-byte key, starting at element `first`"""
    key = np.frombuffer(bytes(key32), np.uint8)
    assert key.size == 32
    _l.check(_l.load().ezkl_hip_chacha20_fr_dev(_p(key), C.c_uint64(stream_id), C.c_size_t(first), _vp(out_ptr), C.c_size_t(n), _stream_ptr(stream)),
             "ezkl_hip_chacha20_fr_dev")


def batch_invert(ptr, n, stream=None):
    _l.check(_l.load().ezkl_hip_batch_invert_dev(_vp(ptr), C.c_size_t(n), _stream_ptr(stream)), "ezkl_hip_batch_invert_dev")


def gen_srs(k, s):
    """test SRS with a KNOWN secret s (insecure, like the reference's gen_srs, src/pfsys/srs.rs:13-16):
    g[i] = s^i G, g_lagrange[i] = L_i(s) G with L_i(s) = (s^n - 1) w^i / (n (s - w^i)); everything on the device.
    Returns (g, g_lagrange) as Bases.  A secret inside the domain (s^n = 1: s = 1, s = w^j) is refused: the closed form is 0 / 0 at row
    j there (batch_invert maps the 0 to 0 and the common factor is 0 as well, so every point would come out as the identity), and such
    an SRS commits the vanishing polynomial to the identity.  s = 0 is not in the domain and is legal."""
    n = 1 << k
    s = int(s) % _R
    if pow(s, n, _R) == 1:
        raise ValueError("gen_srs: the secret is a point of the 2^%d-point domain (s^n = 1): L_i(s) = (s^n - 1) w^i / (n (s - w^i)) "
                         "does not apply there, and a KZG SRS with such a secret is unusable" % k)
    G = np.frombuffer((_MONT % _Q).to_bytes(32, "little") + (2 * _MONT % _Q).to_bytes(32, "little"), np.uint64).copy()
    spow = DeviceBuffer(n * 32)
    vec_fill(spow.ptr, _to_mont(s), n)
    prefix_scan("mul", spow.ptr, spow.ptr, n, exclusive=True)                 # s^i
    g = _Bases.from_scalars(G, spow.ptr, n)
    wp = omega_powers_column(k)                                               # w^i
    den = DeviceBuffer(n * 32)
    vec_fill(den.ptr, _to_mont(s), n)
    vec_op("sub", den.ptr, wp.ptr, den.ptr, n)                                # s - w^i
    batch_invert(den.ptr, n)
    vec_op("mul", den.ptr, wp.ptr, den.ptr, n)
    vec_scale(den.ptr, _to_mont((pow(s, n, _R) - 1) * pow(n, -1, _R) % _R), den.ptr, n)
    gl = _Bases.from_scalars(G, den.ptr, n)
    return g, gl


POINT_REASONS = {1: "x coordinate not below the field modulus", 2: "y coordinate not below the field modulus", 3: "point not on the curve"}


def srs_check_key(seed=None):
    """the 32-byte ChaCha20 key check_srs draws its scalars under: OS entropy, or derived from `seed` (an int) so that a run can be replayed"""
    import hashlib
    import os
    if seed is None:
        return os.urandom(32)
    return hashlib.sha256(b"ezkl_amd.check_srs" + int(seed).to_bytes(32, "little", signed=True)).digest()


def srs_power_combination(g, key):
    """(A, B) = (sum r_i g[i], sum r_i g[i + 1]) over i < n - 1 for the n - 1 scalars of ChaCha20 stream 0 under `key`: the same resident
    scalars in two MSMs on the one handle, at base offsets 0 and 1, without window tables (msm_used_once: the callers, check_srs and
    verify_srs_update, free the set after these and one more MSM).  A one-point set has no adjacent pair: both are the identity."""
    m = g.n - 1
    if m == 0:
        return np.zeros(8, np.uint64), np.zeros(8, np.uint64)
    r = DeviceBuffer(32 * m)
    try:
        chacha20_fr(key, 0, r.ptr, m)
        return msm_used_once(g, r.ptr, m, 0), msm_used_once(g, r.ptr, m, 1)
    finally:
        r.free()


def check_srs(srs, seed=None, structure=True):
    """Is a parsed SRS file (codecs.read_srs) what a prover may use?  -> dict(k, key, points=dict(g=.., g_lagrange=..), powers, lagrange,
    g2, ok, reason): `points` holds Bases.check of either set and always runs; powers / lagrange / g2 are True / False, or None where the
    check did not run; reason is None or says in words what is wrong; key is the ChaCha20 key the scalars came from (srs_check_key(seed)).
    structure=True adds, once every point is valid:
      identities  an identity anywhere in either set fails ("degenerate set"): the point check accepts it, as halo2's reader does, but no
                  power of a usable secret and no L_i(s) of one is zero;
      powers      e(A, s_g2) == e(B, g2) for (A, B) = srs_power_combination: g[i + 1] = s g[i] for every i and the s of s_g2, or the
                  pairing passes with probability 1 / r.  g2 / s_g2 are first held to be canonical points of order r of the twist;
      lagrange    commit_lagrange(v) == commit(iNTT v) byte for byte for a uniform v (stream 1): g_lagrange is the Lagrange basis of g.
    Both sets are uploaded for the duration of the call and freed on every path."""
    from . import native as _nv                            # (native imports plonk, which imports this module)
    k = int(srs["k"])
    n = 1 << k
    key = srs_check_key(seed)
    rep = dict(k=k, key=key, points={}, powers=None, lagrange=None, g2=None, ok=False, reason=None)
    sets, v = {}, None
    try:
        for name in ("g", "g_lagrange"):
            sets[name] = _Bases(np.ascontiguousarray(srs[name]))
            if sets[name].n != n:
                raise ValueError("check_srs: %s has %d points, k = %d" % (name, sets[name].n, k))
            rep["points"][name] = sets[name].check()
        for name in ("g", "g_lagrange"):
            p = rep["points"][name]
            if p["bad"]:
                rep["reason"] = "%s[%d]: %s" % (name, p["first_bad"], POINT_REASONS[p["reason"]])
                return rep
        if not structure:
            rep["ok"] = True
            return rep
        ids = sum(rep["points"][name]["identities"] for name in ("g", "g_lagrange"))
        if ids:
            rep["reason"] = "degenerate set: %d identities" % ids
            return rep
        a, b = srs_power_combination(sets["g"], key)
        try:
            rep["powers"] = _nv.srs_pairing_check(a, b, srs["g2"], srs["s_g2"])
            rep["g2"] = True
        except _nv.SrsOperandError as e:
            rep["g2"] = False
            rep["reason"] = str(e)
            return rep
        v = DeviceBuffer(32 * n)
        chacha20_fr(key, 1, v.ptr, n)
        left = msm_used_once(sets["g_lagrange"], v.ptr, n)
        w = pow(EvaluationDomain.ROOT, 1 << (28 - k), _R)
        if k:                                                  # (the one-point transform is the identity)
            ntt_dev(v.ptr, k, _to_mont(pow(w, -1, _R)), inverse=True)
        rep["lagrange"] = bool((left == msm_used_once(sets["g"], v.ptr, n)).all())
        if not rep["powers"]:
            rep["reason"] = "g: not consecutive powers of one secret"
        elif not rep["lagrange"]:
            rep["reason"] = "g_lagrange is not the Lagrange basis of g"
        else:
            rep["ok"] = True
        return rep
    finally:
        if v is not None:
            v.free()
        for b in sets.values():
            b.free()


def update_srs(srs, t, stages=None, g=None):
    """One step of an updatable SRS: multiply a fresh secret t into a parsed file (codecs.read_srs) whose own secret s nobody here knows
    -> (new_srs, proof).  All on the device:
      g'[i] = t^i g[i]                  t^i by vec_fill + an exclusive product scan, as gen_srs makes s^i; the per-row product is
                                        Bases.mul_scalars (ezkl_hip_bases_mul_scalars)
      g_lagrange'                       rebuilt from g' by the inverse NTT over G1 (Bases.downsize at the file's own k)
      g2' = g2,  s_g2' = [t] s_g2       ezkl_hip_msm_g2 with n = 1
    new_srs has the keys of read_srs; proof = dict(t_g2=[t] g2 as the 128 bytes of the file's G2 layout), what verify_srs_update links
    the two files by.  t is an integer in [1, r) and is in neither return value.  Not detected here: a t with (s t)^n = 1 puts the new
    secret inside the domain and the Lagrange basis comes out degenerate (one point and n - 1 identities); that cannot be seen without
    s, and the structural check of verify_srs_update (or check_srs) reports it as the degenerate set it is.
    stages: a dict to fill with wall seconds per stage, the device drained after each (tools/srs_update_bench.py); None: no extra waits.
    g: srs["g"] as a base set that is resident already (a loader's, checked under its policy); it is read and stays the caller's."""
    import time
    if not isinstance(t, (int, np.integer)) or isinstance(t, bool) or not 1 <= int(t) < _R:
        raise ValueError("update_srs: the secret must be an integer in [1, r)")
    t, k = int(t), int(srs["k"])
    n = 1 << k
    clock = [time.perf_counter()]

    def lap(name):
        if stages is not None:
            synchronize()
            now = time.perf_counter()
            stages[name] = now - clock[0]
            clock[0] = now
    held, tpow = [], None
    try:
        if g is None:
            g = _Bases(np.ascontiguousarray(srs["g"]))
            held.append(g)
        if g.n != n:
            raise ValueError("update_srs: g has %d points, k = %d" % (g.n, k))
        lap("upload")
        tpow = DeviceBuffer(32 * n)
        vec_fill(tpow.ptr, _to_mont(t), n)
        prefix_scan("mul", tpow.ptr, tpow.ptr, n, exclusive=True)             # t^i
        lap("powers")
        g1 = g.mul_scalars(tpow.ptr)
        held.append(g1)
        lap("mul_scalars")
        same, gl1 = g1.downsize(k)
        held += [same, gl1]
        lap("lagrange")
        tm = _to_mont(t)[None]
        g2 = np.frombuffer(bytes(srs["g2"]), np.uint64)[None]
        s_g2 = np.frombuffer(bytes(srs["s_g2"]), np.uint64)[None]
        new_s_g2, t_g2 = msm_g2(s_g2, tm), msm_g2(g2, tm)
        lap("g2")
        new = dict(k=k, g=g1.download(), g_lagrange=gl1.download(), g2=bytes(srs["g2"]), s_g2=new_s_g2.tobytes())
        lap("download")
        return new, dict(t_g2=t_g2.tobytes())
    finally:
        if tpow is not None:
            tpow.free()
        for b in held:
            b.free()


def verify_srs_update(old, new, proof, seed=None):
    """Is `new` the file `old` updated by the t behind proof["t_g2"] (update_srs)?  Both are parsed files (codecs.read_srs).  -> dict(k,
    old, new, t_g2, link, ok, reason): old / new are the reports of check_srs (None where it did not run), t_g2 / link True / False /
    None, reason None or words that begin with the step that failed.  In order:
      1  k: both files have the same k (decided on the host, before any library is loaded); g2: the same g2; g[0]: g'[0] == g[0];
      2  old: / new: check_srs with structure=True of either file -- every point, g = powers of the secret of s_g2, g_lagrange its
         Lagrange basis, no identity;
      3  t_g2: a canonical point of the twist, of order r, not the identity (what ezkl_prover_srs_pairing_check demands of s_g2);
      4  link: e(g[1], t_g2) == e(g'[1], g2), i.e. g'[1] = t g[1].
    With s, s' the secrets that step 2 proves either file to have, step 4 gives s' = t s; step 2 then gives g'[i] = (t s)^i G and
    s_g2' = t s g2 for every i.  NOT proven: that whoever made `new` knew t (there is no proof of knowledge: t_g2 may have been put
    together from other parties' points), nor that they discarded it.  A k = 0 file has no g[1] and is refused at step 4."""
    rep = dict(k=None, old=None, new=None, t_g2=None, link=None, ok=False, reason=None)
    ko, kn = int(old["k"]), int(new["k"])
    if ko != kn:
        rep["reason"] = "k: the old file has k = %d, the new one k = %d" % (ko, kn)
        return rep
    rep["k"] = ko
    if bytes(old["g2"]) != bytes(new["g2"]):
        rep["reason"] = "g2: the two files differ in g2"
        return rep
    if np.asarray(old["g"][0]).tobytes() != np.asarray(new["g"][0]).tobytes():
        rep["reason"] = "g[0]: the new file's first point is not the old file's"
        return rep
    for name, srs in (("old", old), ("new", new)):
        rep[name] = check_srs(srs, seed=seed)
        if not rep[name]["ok"]:
            rep["reason"] = "%s: %s" % (name, rep[name]["reason"])
            return rep
    if ko == 0:
        rep["reason"] = "link: a one-point file has no g[1] to link the secrets by"
        return rep
    from . import native as _nv
    t_g2 = proof["t_g2"]
    t_g2 = t_g2.tobytes() if isinstance(t_g2, np.ndarray) else bytes(t_g2)
    if len(t_g2) != 128:
        rep["t_g2"] = False
        rep["reason"] = "t_g2: %d bytes, a G2 point of the file is 128" % len(t_g2)
        return rep
    try:
        rep["link"] = _nv.srs_pairing_check(old["g"][1], new["g"][1], old["g2"], t_g2)
        rep["t_g2"] = True
    except _nv.SrsOperandError as e:                           # both files passed check_srs: g[1], g'[1] and g2 are points of their groups
        rep["t_g2"] = False
        why = str(e)
        rep["reason"] = "t_g2" + why[len("s_g2"):] if why.startswith("s_g2") else why
        return rep
    if not rep["link"]:
        rep["reason"] = "link: e(g[1], t_g2) != e(g'[1], g2): the new file is not the old one updated by the secret of t_g2"
    else:
        rep["ok"] = True
    return rep


_Q = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47

# Montgomery constants needed host-side (derived, not copied: tools/gen_constants.py)
_R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
_MONT = 1 << 256


def _to_mont(x):
    return np.frombuffer((x * _MONT % _R).to_bytes(32, "little"), np.uint64).copy()


class EvaluationDomain:
    """halo2 EvaluationDomain(j, k): n = 2^k, extended domain 2^ext_k with ext_k = k + ceil(log2(j-1))."""

    ROOT = pow(7, (_R - 1) >> 28, _R)

    def __init__(self, j, k):
        self.k = k
        quotient_poly_degree = j - 1
        self.ext_k = k
        while (1 << self.ext_k) < (1 << k) * quotient_poly_degree:
            self.ext_k += 1
        self.n, self.ne = 1 << k, 1 << self.ext_k
        w = pow(self.ROOT, 1 << (28 - k), _R)
        we = pow(self.ROOT, 1 << (28 - self.ext_k), _R)
        self.omega, self.omega_inv = _to_mont(w), _to_mont(pow(w, -1, _R))
        self.extended_omega, self.extended_omega_inv = _to_mont(we), _to_mont(pow(we, -1, _R))

    def lagrange_to_coeff(self, a):
        return ntt(a, self.k, self.omega_inv, inverse=True)

    def coeff_to_lagrange(self, a):
        return ntt(a, self.k, self.omega, inverse=False)

    def _coset(self, cols, inverse):
        cols = [_fe(c) for c in cols]
        nout = self.ne
        outs = [np.empty((nout, 4), np.uint64) for _ in cols]
        ins = (C.c_void_p * len(cols))(*[c.ctypes.data for c in cols])
        ous = (C.c_void_p * len(cols))(*[o.ctypes.data for o in outs])
        _l.check(_l.load().ezkl_hip_coset_ntt_batch(ins, ous, C.c_size_t(len(cols)), C.c_uint32(self.k),
                                                     C.c_uint32(self.ext_k), C.c_int(1 if inverse else 0)),
                 "ezkl_hip_coset_ntt_batch")
        return outs

    def coeff_to_extended(self, a):
        return self._coset([a], False)[0]

    def extended_to_coeff(self, a):
        return self._coset([a], True)[0]

    def divide_by_vanishing_poly(self, a):
        buf = DeviceBuffer.from_numpy(_fe(a))
        _l.check(_l.load().ezkl_hip_divide_by_vanishing_dev(_vp(buf.ptr), C.c_uint32(self.k), C.c_uint32(self.ext_k),
                                                             _vp(None)), "ezkl_hip_divide_by_vanishing_dev")
        out = buf.to_numpy(shape=(self.ne, 4))
        buf.free()
        return out


class _Prog(C.Structure):
    _fields_ = [("code", _vp), ("n_instr", C.c_uint32), ("n_intermediates", C.c_uint32),
                ("constants", _vp), ("n_constants", C.c_uint32),
                ("rotations", _vp), ("n_rotations", C.c_uint32),
                ("columns", _vp), ("n_columns", C.c_uint32),
                ("challenges", _vp), ("n_challenges", C.c_uint32),
                ("k", C.c_uint32), ("ext_k", C.c_uint32)]


OPS = dict(add=0, sub=1, mul=2, square=3, double=4, negate=5, store=6, horner_step=7)
CONST, INTERMEDIATE, COLUMN, CHALLENGE, PREVIOUS = range(5)


class GraphProgram:
    """Builder for the straight-line program a GraphEvaluator holds (constants, rotations, calculations).

    add_calculation mirrors GraphEvaluator::add_calculation: returns the ValueSource of the result.
    Horner(start, parts, factor) is lowered to store + horner_step, the body of Calculation::Horner."""

    def __init__(self, k, ext_k):
        self.k, self.ext_k = k, ext_k
        self.code, self.constants, self.rotations = [], [], []
        self.n_intermediates = 0

    def constant(self, fe_mont):
        fe_mont = np.asarray(fe_mont, np.uint64)
        for i, c in enumerate(self.constants):
            if (c == fe_mont).all():
                return (CONST, i, 0)
        self.constants.append(fe_mont)
        return (CONST, len(self.constants) - 1, 0)

    def rotation(self, rot):
        if rot not in self.rotations:
            self.rotations.append(rot)
        return self.rotations.index(rot)

    def column(self, idx, rot=0):
        return (COLUMN, idx, self.rotation(rot))

    def challenge(self, idx):
        return (CHALLENGE, idx, 0)

    def previous(self):
        return (PREVIOUS, 0, 0)

    def calc(self, op, s0, s1=(CONST, 0, 0), target=None):
        if target is None:
            target = self.n_intermediates
            self.n_intermediates += 1
        self.code.append([OPS[op], target, *s0, *s1])
        return (INTERMEDIATE, target, 0)

    def horner(self, start, parts, factor):
        t = self.calc("store", start)
        for p in parts:
            self.calc("horner_step", p, factor, target=t[1])
        return t

    def arrays(self):
        code = np.asarray(self.code, np.uint32).reshape(-1, 8)
        consts = np.asarray(self.constants, np.uint64).reshape(-1, 4)
        rots = np.asarray(self.rotations, np.int32)
        return code, consts, rots

    def row_sharded(self, log_world):
        """The same program for ONE row shard of a sweep split over 2^log_world ranks.  Returns
        (program, queries): every distinct (column, rotation) the code reads becomes a column of its own, read at rotation 0,
        and queries[j] = (column, row_shift) says which window of the original extended column the j-th new column is: rows
        [lo + row_shift, hi + row_shift) mod 2^ext_k for the shard [lo, hi) (dist.row_windows / reshard_columns_to_rows).
        The shard is a domain of 2^(ext_k - log_world) rows, so the existing sweep entry point runs it unchanged."""
        assert 0 <= log_world <= self.k
        step = 1 << (self.ext_k - self.k)
        sub = GraphProgram(self.k - log_world, self.ext_k - log_world)
        sub.constants, sub.n_intermediates, sub.rotations = list(self.constants), self.n_intermediates, [0]
        queries, index = [], {}

        def remap(t, idx, rot):
            if t != COLUMN:
                return [t, idx, rot]
            key = (idx, self.rotations[rot] * step)
            if key not in index:
                index[key] = len(queries)
                queries.append(key)
            return [COLUMN, index[key], 0]
        for op, target, t0, i0, r0, t1, i1, r1 in self.code:
            sub.code.append([op, target, *remap(t0, i0, r0), *remap(t1, i1, r1)])
        return sub, queries

    def _host_program(self, n_columns, challenges):
        """the program with null column pointers, for the host-only entry points.  Every entry point validates the whole program (operand
        indices included): without `challenges`, as many zero challenges as the code reads are declared"""
        code, consts, rots = self.arrays()
        cols = (C.c_void_p * max(1, n_columns))()
        if challenges is None:
            n_chal = 1 + max([int(ins[3 + 3 * q]) for ins in code.tolist() for q in (0, 1) if ins[2 + 3 * q] == CHALLENGE] + [0])
            challenges = np.zeros((n_chal, 4), np.uint64)
        ch = _fe(np.asarray(challenges, np.uint64).reshape(-1, 4))
        pr = _Prog(_p(code), code.shape[0], self.n_intermediates, _p(consts), consts.shape[0], _p(rots), rots.shape[0],
                   C.cast(cols, _vp), n_columns, _p(ch), ch.shape[0], self.k, self.ext_k)
        return pr, (code, consts, rots, cols, ch)

    def check_compiles(self, n_columns, challenges=None):
        """host-only: lower the program to HIP source and compile it for gfx950 with hiprtc (no GPU needed).  With EZKL_HIP_JIT_DUMP=<file>
        set, the library writes the source it compiles there (tools/evalh29_model.py reads it)"""
        pr, keep = self._host_program(n_columns, challenges)
        _l.check(_l.load().ezkl_hip_eval_h_check(C.byref(pr)), "ezkl_hip_eval_h_check")

    def generated_source(self, n_columns, challenges=None):
        """host-only: the HIP source the sweep JIT generates for this program (the generator EZKL_EVALH_R29 selects), not compiled
        (ezkl_hip_eval_h_source; tools/evalh29_model.py reads it)"""
        pr, keep = self._host_program(n_columns, challenges)
        n = C.c_size_t(0)
        rc = _l.load().ezkl_hip_eval_h_source(C.byref(pr), None, C.c_size_t(0), C.byref(n))
        if n.value == 0:                              # the program itself was refused (a valid one has a non-empty source)
            _l.check(rc, "ezkl_hip_eval_h_source")
        buf = C.create_string_buffer(n.value + 1)
        _l.check(_l.load().ezkl_hip_eval_h_source(C.byref(pr), buf, C.c_size_t(n.value + 1), C.byref(n)), "ezkl_hip_eval_h_source")
        return buf.value.decode()

    def scheduled_code(self, n_columns, challenges=None):
        """host-only: the instruction order the library executes this program in (ezkl_hip_eval_h_schedule)"""
        pr, keep = self._host_program(n_columns, challenges)
        code = keep[0]
        out = np.zeros_like(code)
        _l.check(_l.load().ezkl_hip_eval_h_schedule(C.byref(pr), out.ctypes.data_as(C.c_void_p)), "ezkl_hip_eval_h_schedule")
        return out

    def evaluate_h(self, column_ptrs, challenges, out_ptr, stream=None):
        """Run on device-resident columns (list of device pointers); out_ptr holds PreviousValue on entry."""
        code, consts, rots = self.arrays()
        ch = _fe(np.asarray(challenges, np.uint64).reshape(-1, 4))
        cols = (C.c_void_p * max(1, len(column_ptrs)))(*column_ptrs)
        pr = _Prog(_p(code), code.shape[0], self.n_intermediates, _p(consts), consts.shape[0], _p(rots), rots.shape[0],
                   C.cast(cols, _vp), len(column_ptrs), _p(ch), ch.shape[0], self.k, self.ext_k)
        _l.check(_l.load().ezkl_hip_eval_h_dev(C.byref(pr), _vp(out_ptr), _stream_ptr(stream)), "ezkl_hip_eval_h_dev")


    def check_source(self, n_columns, slots, challenges=None):
        """host-only: the source of the mock prover's check kernel for the intermediates `slots` (ezkl_hip_eval_check_source; k == ext_k)"""
        pr, keep = self._host_program(n_columns, challenges)
        sl = (C.c_uint32 * max(1, len(slots)))(*slots)
        n = C.c_size_t(0)
        rc = _l.load().ezkl_hip_eval_check_source(C.byref(pr), sl, C.c_uint32(len(slots)), None, C.c_size_t(0), C.byref(n))
        if n.value == 0:
            _l.check(rc, "ezkl_hip_eval_check_source")
        buf = C.create_string_buffer(n.value + 1)
        _l.check(_l.load().ezkl_hip_eval_check_source(C.byref(pr), sl, C.c_uint32(len(slots)), buf, C.c_size_t(n.value + 1), C.byref(n)),
                 "ezkl_hip_eval_check_source")
        return buf.value.decode()

    def check_rows(self, column_ptrs, challenges, slots, row_lo, row_hi, cap=1024, stream=None):
        """the mock prover's gate check on device columns of 2^k rows (ezkl_hip_eval_check_dev): every row in [row_lo, row_hi) where a
        listed intermediate is not zero.  Returns (records (1, slot, 0, row), [total])"""
        code, consts, rots = self.arrays()
        ch = _fe(np.asarray(challenges, np.uint64).reshape(-1, 4))
        cols = (C.c_void_p * max(1, len(column_ptrs)))(*column_ptrs)
        pr = _Prog(_p(code), code.shape[0], self.n_intermediates, _p(consts), consts.shape[0], _p(rots), rots.shape[0],
                   C.cast(cols, _vp), len(column_ptrs), _p(ch), ch.shape[0], self.k, self.ext_k)
        sl = (C.c_uint32 * max(1, len(slots)))(*slots)
        rec, cnt = DeviceBuffer(max(1, cap) * 16), DeviceBuffer.from_numpy(np.zeros(1, np.uint64))
        _l.check(_l.load().ezkl_hip_eval_check_dev(C.byref(pr), sl, C.c_uint32(len(slots)), C.c_uint32(row_lo), C.c_uint32(row_hi), _vp(rec.ptr),
                                                    C.c_uint32(cap), _vp(cnt.ptr), _stream_ptr(stream)), "ezkl_hip_eval_check_dev")
        return _records(rec, cnt, cap)


def jit_stats():
    """(compiled by hiprtc, loaded from the disk cache, found in memory) sweep kernels of this process"""
    a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    _l.check(_l.load().ezkl_hip_eval_h_jit_stats(C.byref(a), C.byref(b), C.byref(c)), "ezkl_hip_eval_h_jit_stats")
    return int(a.value), int(b.value), int(c.value)


def last_kernel_ms(which):
    ms = C.c_float(0)
    _l.check(_l.load().ezkl_hip_last_kernel_ms(which.encode(), C.byref(ms)), "ezkl_hip_last_kernel_ms")
    return float(ms.value)


def kernel_ms_stats(which, reset=False):
    """(sum of device ms, number of regions) of every `which` region recorded since the last reset -- read AFTER a timed loop: the
    regions of back-to-back calls each have an event pair of their own (ezkl_hip_kernel_ms_stats)"""
    s, n = C.c_double(0), C.c_uint64(0)
    _l.check(_l.load().ezkl_hip_kernel_ms_stats(which.encode(), C.byref(s), C.byref(n), C.c_int(1 if reset else 0)), "ezkl_hip_kernel_ms_stats")
    return float(s.value), int(n.value)


class WitnessError(ValueError):
    """a synthesis on the device met a value outside its decomposition range, a lookup input outside its table, a gather index outside
    its table or a sort or arg-extremum key beyond 62 bits (the layout's own assertions on the host path)"""


def witness_tile(columns, k, unit_rows, tiles, pairs, stream=None):
    """a tiled circuit from its unit (ezkl_hip_witness_tile_dev): for every (dst, src) of `pairs`, column indices into `columns`
    (DeviceBuffers of 2^k Montgomery words), rows [t * U, (t + 1) * U) of dst get rows [0, U) of src -- every t < tiles for a block copy,
    t >= 1 for a column tiled onto itself.  Rows past tiles * unit_rows and columns outside the pairs stay as they are.  One launch,
    not waited for (device time: last_kernel_ms("witness_tile")).  Raises ValueError, nothing launched, on a geometry or a pair list
    the library refuses."""
    if any(c.nbytes < (32 << k) for c in columns):
        raise ValueError("a column shorter than 2^%d words" % k)
    pairs = [(int(d), int(s)) for d, s in pairs]
    if any(not 0 <= v < 1 << 32 for p in pairs for v in p) or not (0 <= unit_rows < 1 << 32 and 0 <= tiles < 1 << 32):
        raise ValueError("witness_tile: an argument outside 32 bits")
    ptrs = (_vp * len(columns))(*[c.ptr for c in columns])
    dst, src = (np.ascontiguousarray([p[i] for p in pairs], dtype=np.uint32) for i in (0, 1))
    rc = _l.load().ezkl_hip_witness_tile_dev(ptrs, C.c_uint32(len(columns)), C.c_uint32(k), C.c_uint32(unit_rows), C.c_uint32(tiles), _p(dst), _p(src),
                                             C.c_uint32(len(pairs)), _stream_ptr(stream))
    if rc == -3:
        raise ValueError("witness_tile: refused (unit_rows %d x tiles %d at k = %d, %d pairs)" % (unit_rows, tiles, k, len(pairs)))
    _l.check(rc, "ezkl_hip_witness_tile_dev")


def witness_wide_dots(reset=False):
    """how many DOT records this process has replayed on the wide kernel (ezkl_hip_witness_wide_dots: one step of at least
    witness_plan.DOT_WIDE_MIN products, the claimed product of an einsum); reset: back to zero after the reading"""
    out = C.c_uint64(0)
    _l.check(_l.load().ezkl_hip_witness_wide_dots(C.byref(out), C.c_int(1 if reset else 0)), "ezkl_hip_witness_wide_dots")
    return int(out.value)


class WitnessPlan:
    """a witness plan (witness_plan.WitnessPlan bytes) resident on the device: `run` synthesizes the advice columns of one proof
    into DeviceBuffers (ezkl_hip_witness_run_dev) -- the columns native.create_proof takes as they are.  A plan with phases
    (n_phases > 1: second-phase advice) runs phase by phase, `run(phase=..., challenges=...)`, between the prover's commit stages:
    `advice_fn` is the callable native.create_proof takes for that."""

    def __init__(self, blob):
        blob = bytes(blob)
        self.h = _vp()
        L = _l.load()
        rc = L.ezkl_hip_witness_plan_upload(blob, C.c_size_t(len(blob)), C.byref(self.h))
        if rc == -3:
            raise ValueError(L.ezkl_hip_witness_last_error().decode() or "witness plan refused")
        _l.check(rc, "ezkl_hip_witness_plan_upload")
        info = (C.c_uint32 * 8)()
        _l.check(L.ezkl_hip_witness_plan_info(self.h, info), "ezkl_hip_witness_plan_info")
        self.k, self.n_advice, self.n_inputs, self.n_outputs, self.n_records, self.n_cells, self.n_ops, self.n_params = [int(v) for v in info]
        ph, col_phase = (C.c_uint32 * 2)(), (C.c_uint8 * self.n_advice)()
        _l.check(L.ezkl_hip_witness_plan_phases(self.h, ph, col_phase), "ezkl_hip_witness_plan_phases")
        self.n_phases, self.n_challenges = int(ph[0]), int(ph[1])
        self.column_phase = [int(v) for v in col_phase]   # the phase each advice column belongs to
        self.last = None                             # counters of the last run
        # the records of kind 11 (a static lookup's outputs): header of 20 words and the parameter hash, the parameters, the constants, then 8 words a record
        head = np.frombuffer(blob, "<u4", 20)
        recs = np.frombuffer(blob, "<u4", 8 * int(head[4]), 112 + 8 * int(head[6]) + 32 * int(head[7])).reshape(-1, 8)
        kinds = recs[:, 0]
        self.n_lookup_records, self.last_stats_ms, self.last_outputs_ms = int((kinds == 11).sum()), None, None
        self.lookup_phases = sorted(set(int(p) for p in recs[kinds == 11, 7]))      # the phases that hold such a record

    def alloc_columns(self):
        return [DeviceBuffer(32 << self.k) for _ in range(self.n_advice)]

    def run(self, inputs, columns=None, stream=None, phase=None, challenges=()):
        """inputs: the model inputs as (signed) integers -> (columns: n_advice DeviceBuffers of 2^k Montgomery words, outputs as ints).
        self.last = dict(cells_written, launches, device_ms).  Raises WitnessError, naming the op, when a value does not fit its
        decomposition or its lookup table, or an einsum operand its exact product; the process goes on and the plan can run again.
        phase = p: that phase alone (ezkl_hip_witness_run_phase_dev) with the challenges squeezed so far as canonical ints -- it fills
        the columns of its phase and leaves the others as they are; the inputs go with phase 0 (later phases ignore them), the outputs
        come with the last phase ([] before).  phase = None is the one-call run of a plan without phases."""
        if phase is not None and phase > 0:
            x = np.zeros(0, np.int64)
        else:
            x = np.ascontiguousarray(np.asarray([int(v) for v in inputs], dtype=np.int64))
            if len(x) != self.n_inputs:
                raise ValueError("the plan takes %d inputs, got %d" % (self.n_inputs, len(x)))
        cols = columns if columns is not None else self.alloc_columns()
        if len(cols) != self.n_advice or any(c.nbytes < (32 << self.k) for c in cols):
            raise ValueError("the plan writes %d columns of %d bytes" % (self.n_advice, 32 << self.k))
        ptrs = (_vp * self.n_advice)(*[c.ptr for c in cols])
        outs = np.zeros((max(1, self.n_outputs), 4), np.uint64)
        status = (C.c_uint64 * 4)()
        L = _l.load()
        if phase is None:
            rc = L.ezkl_hip_witness_run_dev(self.h, _p(x), C.c_size_t(len(x)), ptrs, _p(outs), status, _stream_ptr(stream))
        else:
            ch = b"".join((int(c) % (1 << 256)).to_bytes(32, "little") for c in challenges)      # canonical, as they are: the library refuses c >= r
            rc = L.ezkl_hip_witness_run_phase_dev(self.h, C.c_uint32(phase), _p(x), C.c_size_t(len(x)), ch, C.c_size_t(len(ch) // 32), ptrs, _p(outs), status,
                                                  _stream_ptr(stream))
        self.last = dict(failed=int(status[0]), first=(int(status[1]) >> 32, int(status[1]) & 0xffffffff), cells_written=int(status[2]), launches=int(status[3]))
        if rc == -3:
            if columns is None:
                for c in cols:
                    c.free()
            if status[0]:                            # a lane reported: the witness is refused, not the call
                raise WitnessError(L.ezkl_hip_witness_last_error().decode())
            raise ValueError(L.ezkl_hip_witness_last_error().decode() or "ezkl_hip_witness_run_dev: invalid argument")
        _l.check(rc, "ezkl_hip_witness_run_dev")
        self.last["device_ms"] = last_kernel_ms("witness")
        done = phase is None or phase == self.n_phases - 1
        return cols, [_from_mont_int(outs[i]) for i in range(self.n_outputs)] if done else []

    def lookup_stats(self, columns, stream=None):
        """(min_lookup_inputs, max_lookup_inputs) of the witness in `columns` -- the columns a `run` of this plan that raised nothing has
        just written: the least and the greatest signed input of its static lookups, folded with 0 (ezkl_hip_witness_lookup_stats_dev;
        witness_plan.lookup_stats_host is its specification).  self.last_stats_ms: the kernel's HIP-event time, None when the plan has no
        static lookup and nothing was launched.  Raises WitnessError when a source is beyond 62 bits."""
        if len(columns) != self.n_advice or any(c.nbytes < (32 << self.k) for c in columns):
            raise ValueError("the plan reads %d columns of %d bytes" % (self.n_advice, 32 << self.k))
        ptrs = (_vp * self.n_advice)(*[c.ptr for c in columns])
        out = (C.c_int64 * 2)()
        L = _l.load()
        rc = L.ezkl_hip_witness_lookup_stats_dev(self.h, ptrs, out, _stream_ptr(stream))
        if rc == -3:
            raise WitnessError(L.ezkl_hip_witness_last_error().decode() or "ezkl_hip_witness_lookup_stats_dev: invalid argument")
        _l.check(rc, "ezkl_hip_witness_lookup_stats_dev")
        self.last_stats_ms = last_kernel_ms("witness_lookup_stats") if self.n_lookup_records else None
        return int(out[0]), int(out[1])

    def outputs(self, columns, stream=None):
        """the plan's outputs as ints, gathered from `columns` once phase 0 has run to its end on them (ezkl_hip_witness_outputs_dev:
        one launch, one copy, one wait) -- `run` hands them back with the LAST phase only, the instance column is needed before the first
        commitment.  self.last_outputs_ms: the gather's HIP-event time, None for a plan without outputs.  Raises ValueError with the
        library's reason, nothing launched, before phase 0 has succeeded or on other columns than it ran on."""
        if len(columns) != self.n_advice or any(c.nbytes < (32 << self.k) for c in columns):
            raise ValueError("the plan reads %d columns of %d bytes" % (self.n_advice, 32 << self.k))
        ptrs = (_vp * self.n_advice)(*[c.ptr for c in columns])
        outs = np.zeros((max(1, self.n_outputs), 4), np.uint64)
        L = _l.load()
        rc = L.ezkl_hip_witness_outputs_dev(self.h, ptrs, _p(outs), _stream_ptr(stream))
        if rc == -3:
            raise ValueError(L.ezkl_hip_witness_last_error().decode() or "ezkl_hip_witness_outputs_dev: invalid argument")
        _l.check(rc, "ezkl_hip_witness_outputs_dev")
        self.last_outputs_ms = last_kernel_ms("witness_outputs") if self.n_outputs else None
        return [_from_mont_int(outs[i]) for i in range(self.n_outputs)]

    def advice_fn(self, inputs, columns):
        """the per-phase witness callback of native.create_proof(..., device_columns=range(n_advice)): (phase, challenges) -> {column:
        DeviceBuffer} of the phase just run, synthesized into `columns` (alloc_columns()).  self.phase_ms collects the device time of
        each phase."""
        self.phase_ms = {}
        def fn(phase, challenges):
            self.run(inputs, columns=columns, phase=int(phase), challenges=list(challenges))
            self.phase_ms[int(phase)] = self.last["device_ms"]
            return {c: columns[c] for c in range(self.n_advice) if self.column_phase[c] == phase}
        return fn

    def free(self):
        if self.h:
            _l.load().ezkl_hip_witness_plan_free(self.h)
            self.h = _vp()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def ubench(which):
    out = C.c_double(0)
    _l.check(_l.load().ezkl_hip_ubench(which.encode(), C.byref(out)), "ezkl_hip_ubench")
    return float(out.value)


def field_probe_names():
    """{name: (operands, words per operand row, words per result row)} of ezkl_hip_field_probe_dev (host only, no device needed)"""
    n = C.c_size_t(0)
    _l.check(_l.load().ezkl_hip_field_probe_names(None, C.c_size_t(0), C.byref(n)), "ezkl_hip_field_probe_names")
    buf = C.create_string_buffer(n.value + 1)
    _l.check(_l.load().ezkl_hip_field_probe_names(buf, C.c_size_t(n.value + 1), C.byref(n)), "ezkl_hip_field_probe_names")
    out = {}
    for line in buf.value.decode().splitlines():
        name, arity, w_in, w_out = line.split()
        out[name] = (int(arity), int(w_in), int(w_out))
    return out


def field_probe(name, operands):
    """test hook: one field primitive on the device.  operands: uint32 arrays (n, words per row); returns the (n, words) uint32 result"""
    arity, w_in, w_out = field_probe_names()[name]
    ops = [np.ascontiguousarray(o, dtype=np.uint32) for o in operands]
    if len(ops) != arity or any(o.ndim != 2 or o.shape != (ops[0].shape[0], w_in) for o in ops):
        raise ValueError("%s takes %d operands of shape (n, %d)" % (name, arity, w_in))
    n = ops[0].shape[0]
    bufs = [DeviceBuffer.from_numpy(o) for o in ops]
    out = DeviceBuffer(max(1, n) * w_out * 4)
    arr = (C.c_void_p * 4)(*([b.ptr for b in bufs] + [None] * (4 - arity)))
    try:
        _l.check(_l.load().ezkl_hip_field_probe_dev(name.encode(), arr, _vp(out.ptr), C.c_size_t(n), _vp(None)), "ezkl_hip_field_probe_dev")
        return out.to_numpy(np.uint32)[:n * w_out].reshape(n, w_out)
    finally:
        out.free()
        for b in bufs:
            b.free()


# ---------------------------------------------------------------------------------------------------
# A13 helpers composed from the kernels above ([UPSTREAM] halo2 permutation::prover::commit
# and mv_lookup::prover::commit_grand_sum).  Everything stays resident; blinding rows / RNG stay with the caller.
_DELTA = pow(7, 1 << 28, _R)


def omega_powers_column(k):
    """device column X[i] = omega_k^i (built with an exclusive product scan of a constant column)"""
    n = 1 << k
    w = pow(EvaluationDomain.ROOT, 1 << (28 - k), _R)
    col = DeviceBuffer(n * 32)
    vec_fill(col.ptr, _to_mont(w), n)
    prefix_scan("mul", col.ptr, col.ptr, n, exclusive=True)
    return col


def permutation_grand_product(k, value_cols, sigma_cols, beta, gamma, omega_col=None, first_column_index=0, z0=None):
    """z[0] = z0 (1), z[i+1] = z[i] * prod_j (v_j[i] + beta*delta^(j0+j)*omega^i + gamma) / (v_j[i] + beta*sigma_j[i] + gamma)
    for one chunk of permutation columns.  value_cols / sigma_cols: lists of device pointers (n rows each).
    Returns a DeviceBuffer with z[0..n) (the caller overwrites the blinding rows)."""
    n = 1 << k
    m = len(value_cols)
    omega_col = omega_col or omega_powers_column(k)
    beta_i, gamma_i = _from_mont_int(beta), _from_mont_int(gamma)
    # denominators and numerators as two straight-line programs over [values..., sigmas..., X]
    cols = list(value_cols) + list(sigma_cols) + [omega_col.ptr]
    chal = [_to_mont(beta_i), _to_mont(gamma_i)] + [_to_mont(beta_i * pow(_DELTA, first_column_index + j, _R) % _R) for j in range(m)]
    den = GraphProgram(k, k)
    acc = None
    for j in range(m):
        t = den.calc("add", den.calc("add", den.calc("mul", den.challenge(0), den.column(m + j)), den.challenge(1)), den.column(j))
        acc = t if acc is None else den.calc("mul", acc, t)
    num = GraphProgram(k, k)
    accn = None
    for j in range(m):
        t = num.calc("add", num.calc("add", num.calc("mul", num.challenge(2 + j), num.column(2 * m)), num.challenge(1)), num.column(j))
        accn = t if accn is None else num.calc("mul", accn, t)
    d_den, d_num = DeviceBuffer(n * 32), DeviceBuffer(n * 32)
    den.evaluate_h(cols, chal, d_den.ptr)
    num.evaluate_h(cols, chal, d_num.ptr)
    batch_invert(d_den.ptr, n)
    vec_op("mul", d_num.ptr, d_den.ptr, d_num.ptr, n)                   # ratio[i]
    prefix_scan("mul", d_num.ptr, d_num.ptr, n, exclusive=True)          # z[i] = prod_{r<i} ratio[r]
    if z0 is not None:
        _l.check(_l.load().ezkl_hip_vec_scale_dev(_vp(d_num.ptr), _p(_fe(z0)), _vp(d_num.ptr), C.c_size_t(n), _vp(None)), "vec_scale")
    d_den.free()
    return d_num


def lookup_grand_sum(k, input_cols, table_col, m_col, beta):
    """phi[0] = 0, phi[i+1] = phi[i] + sum_j 1/(f_j[i] + beta) - m[i]/(t[i] + beta)   (mv-lookup / logUp running sum)"""
    n = 1 << k
    nin = len(input_cols)
    chal = [_fe(beta)]
    acc = DeviceBuffer.from_numpy(np.zeros((n, 4), np.uint64))
    tmp = DeviceBuffer(n * 32)
    shift = GraphProgram(k, k)
    shift.calc("add", shift.column(0), shift.challenge(0))
    for j in range(nin):
        shift.evaluate_h([input_cols[j]], chal, tmp.ptr)
        batch_invert(tmp.ptr, n)
        vec_op("add", acc.ptr, tmp.ptr, acc.ptr, n)
    shift.evaluate_h([table_col], chal, tmp.ptr)
    batch_invert(tmp.ptr, n)
    vec_op("mul", tmp.ptr, m_col, tmp.ptr, n)
    vec_op("sub", acc.ptr, tmp.ptr, acc.ptr, n)
    prefix_scan("add", acc.ptr, acc.ptr, n, exclusive=True)
    tmp.free()
    return acc


def _from_mont_int(a):
    return int.from_bytes(np.ascontiguousarray(a, np.uint64).tobytes(), "little") * pow(_MONT, -1, _R) % _R


# ---- multi-GPU: the library's RCCL communicator (csrc/comm.hip) --------------------------------------------------------------
def comm_unique_id():
    out = (C.c_uint8 * 128)()
    _l.check(_l.load().ezkl_hip_comm_unique_id(out), "ezkl_hip_comm_unique_id")
    return bytes(out)


def comm_init(unique_id, world, rank):
    _l.check(_l.load().ezkl_hip_comm_init(bytes(unique_id), C.c_int(world), C.c_int(rank)), "ezkl_hip_comm_init")


def mem_info():
    """(free, total) bytes of the calling context's device"""
    f, t = C.c_size_t(0), C.c_size_t(0)
    _l.check(_l.load().ezkl_hip_mem_info(C.byref(f), C.byref(t)), "ezkl_hip_mem_info")
    return int(f.value), int(t.value)


def pool_stats():
    """the calling context's column pool: dict(live, live_peak, parked, bound) in bytes (ezkl_hip_pool_stats)"""
    out = (C.c_size_t * 4)()
    _l.check(_l.load().ezkl_hip_pool_stats(out), "ezkl_hip_pool_stats")
    return dict(live=int(out[0]), live_peak=int(out[1]), parked=int(out[2]), bound=int(out[3]))


def pool_trim():
    _l.check(_l.load().ezkl_hip_pool_trim(), "ezkl_hip_pool_trim")


def contexts_configure(devices):
    """the context table of libezkl_hip.so, before its first use: context i on device devices[i] (several may share a device)"""
    arr = (C.c_int * len(devices))(*devices)
    _l.check(_l.load().ezkl_hip_contexts_configure(C.c_int(len(devices)), arr), "ezkl_hip_contexts_configure")


def context_count():
    return int(_l.load().ezkl_hip_context_count())


def set_context(index):
    _l.check(_l.load().ezkl_hip_set_context(C.c_int(index)), "ezkl_hip_set_context")


def comm_init_from_torch(dist, device):
    """rank 0 creates the id, torch.distributed (any backend) broadcasts its 128 bytes, every rank joins"""
    import torch
    world, rank = dist.get_world_size(), dist.get_rank()
    t = torch.zeros(128, dtype=torch.uint8, device=device)
    if rank == 0:
        t = torch.tensor(list(comm_unique_id()), dtype=torch.uint8, device=device)
    dist.broadcast(t, 0)
    comm_init(bytes(t.cpu().numpy().tobytes()), world, rank)


def comm_info():
    w, r = C.c_int(0), C.c_int(0)
    _l.check(_l.load().ezkl_hip_comm_info(C.byref(w), C.byref(r)), "ezkl_hip_comm_info")
    return w.value, r.value


def comm_destroy():
    _l.check(_l.load().ezkl_hip_comm_destroy(), "ezkl_hip_comm_destroy")


def comm_allgather_dev(ptr, total_bytes):
    _l.check(_l.load().ezkl_hip_comm_allgather_dev(_vp(ptr), C.c_size_t(total_bytes)), "ezkl_hip_comm_allgather_dev")


def comm_fold_points(points):
    """(count, 8) u64 partial sums -> sums over all ranks (in a copy)"""
    a = np.ascontiguousarray(points, np.uint64).copy()
    _l.check(_l.load().ezkl_hip_comm_fold_points(_p(a), C.c_uint32(a.shape[0])), "ezkl_hip_comm_fold_points")
    return a


class _CommSeg(C.Structure):
    _fields_ = [("peer", C.c_int), ("ptr", C.c_void_p), ("bytes", C.c_size_t)]


def comm_alltoallv_dev(sends, recvs):
    """sends / recvs: lists of (peer, device pointer, bytes); per peer the segments are ONE byte stream in list order (totals must agree)"""
    sa = (_CommSeg * max(1, len(sends)))(*[_CommSeg(p, ptr, n) for p, ptr, n in sends])
    ra = (_CommSeg * max(1, len(recvs)))(*[_CommSeg(p, ptr, n) for p, ptr, n in recvs])
    _l.check(_l.load().ezkl_hip_comm_alltoallv_dev(sa, C.c_size_t(len(sends)), ra, C.c_size_t(len(recvs))), "ezkl_hip_comm_alltoallv_dev")


def comm_selftest():
    """ezkl_hip_comm_selftest: the library communicator tries out every collective shape the prover uses (a collective: every rank calls
    it; ezkl_hip_comm_init already ran it unless EZKL_COMM_SELFTEST=0).  Raises EzklHipError with the failing status."""
    _l.check(_l.load().ezkl_hip_comm_selftest(), "ezkl_hip_comm_selftest")


def comm_available():
    """librccl loads and exports every entry point the library communicator binds (no device touched, nothing called)"""
    return _l.load().ezkl_hip_comm_available() == 0


def comm_stats(reset=False):
    """what this process's exchanges have moved (ezkl_hip_comm_stats): calls, bytes to / from other ranks, host seconds inside the calls,
    ncclSend / ncclRecv operations issued, rounds"""
    out = (C.c_uint64 * 8)()
    _l.check(_l.load().ezkl_hip_comm_stats(out, C.c_int(1 if reset else 0)), "ezkl_hip_comm_stats")
    return dict(exchanges=int(out[0]), bytes_sent=int(out[1]), bytes_received=int(out[2]), seconds=out[3] / 1e6, nccl_sends=int(out[4]),
                nccl_recvs=int(out[5]), rounds=int(out[6]))


def comm_allgather_host(arr):
    """in place on a (world, ...) numpy array: row r valid on rank r going in, every row coming out"""
    arr = np.ascontiguousarray(arr)
    world = comm_info()[0]
    _l.check(_l.load().ezkl_hip_comm_allgather_host(_p(arr), C.c_size_t(arr.nbytes // max(1, world))), "ezkl_hip_comm_allgather_host")
    return arr


def comm_alltoall_dev(send_ptr, send_off, send_len, recv_ptr, recv_off, recv_len):
    arr = lambda v: (C.c_size_t * len(v))(*[int(x) for x in v])
    _l.check(_l.load().ezkl_hip_comm_alltoall_dev(_vp(send_ptr), arr(send_off), arr(send_len), _vp(recv_ptr), arr(recv_off), arr(recv_len)),
             "ezkl_hip_comm_alltoall_dev")
