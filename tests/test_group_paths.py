"""Device groups at range seams, with short batches, padded strides and failing members.

Every rsmi_group_* batch call (rsmi_group.cpp) splits its blocks with rsmi_partition, offsets five
pointers per member (data + st*data_block_stride, parity + st*parity_block_stride,
shards + st*block_stride, raw16_out + st*n, raw32_out + st*n), runs each non-empty range on the
member's worker thread and returns the first failing member's status in member order.  The legs:

  0 (CPU)  the group validates like member 0 with nblocks > 0, and the first-failure rule with
           the library's own "inject_host_fault" option, which throws before the device is touched
  1        every entry point with nblocks below, at and above the member count, block strides
           with padding, sentinels in every gap and one poisoned block past each raw array
  2        the copy-engine pipeline, the in-place kernel on page-locked memory, and both in one call
  3        a member that fails: the status, the survival of workers and contexts, empty parts
  4        two threads on one group beside a third on member 0's context; the caller's wait hook
  5        rsmi_group_host_alloc with one block, with every range inside one page, and with the
           member seam in the middle of a page

Shapes: RS(4,2) with S = 1000 and RS(10,4) with S = 2049 (odd: the linear upload on the pipeline
path).  Members are [i % device_count() for i in range(M)].  Block b of a case holds
splitmix64_bytes(SEED ^ b), so a range coded from another block's offset cannot compare equal.
References: oracle_lib.encode_fast, oracle_lib.reconstruct, oracle_lib.crc16_ibm, zlib.crc32.
Every byte of every buffer and every CRC slot is compared; there are no tolerances.

The rows reconstruct of leg 1 loses two data rows and one parity row where the code allows three
losses (RS(10,4)).  RS(4,2) allows two, so it runs two patterns instead: data rows 0 and 2 lost
with row 2 required, and rows 0 and k lost with the parity row k required.  Between them they
cover what the three-row pattern covers: a required data row, a required parity row and a lost
row that is not required and keeps its fill.
"""
import ctypes
import ctypes.util
import mmap
import threading
import zlib

import numpy as np
import pytest

import oracle_lib as orc
import rsmi

SEED = 0x6209A7
SHAPES = [(4, 2, 1000), (10, 4, 2049)]
REF_NB = 9            # 2 * 4 + 1: the largest batch of this module
PAD = (24, 40, 56)    # bytes after every data, parity and shards block
TAIL = 64             # sentinel bytes past the last block
GAPFILL = 0x5A        # gaps and tails
SENT = 0xEE           # parity rows and lost rows before a call
POISON = 0xA5A5A5A5   # raw CRC slots before a call


def nt_of(K, MT):
    """DESIGN.md §4.1, as in test_kernel_matrix.py."""
    return 2 if K >= 4 * MT else 1


def fast_label(K, MT):
    return "rs_fast_kernel<K=%d,MT=%d,NT=%d>" % (K, MT, nt_of(K, MT))


def first_failure(nb, statuses):
    """What a group call returns when member i's own call returns statuses[i]: the first status
    that is not OK, in member order, among the members whose part of nb blocks is not empty."""
    for i, st in enumerate(statuses):
        if rsmi.partition(nb, len(statuses), i)[1] and st != rsmi.OK:
            return st
    return rsmi.OK


def member_devices(M):
    return [i % max(1, rsmi.device_count()) for i in range(M)]


def batch_sizes(M):
    return sorted({1, M - 1, M, M + 1, 2 * M + 1})


def test_first_failure_helper_and_batch_sizes():
    OK, ND, EH = rsmi.OK, rsmi.ErrNoDevice, rsmi.ErrHost
    assert first_failure(5, [OK, OK, OK]) == OK
    assert first_failure(5, [OK, EH, ND]) == EH
    assert first_failure(5, [ND, EH, ND]) == ND
    assert first_failure(2, [OK, OK, EH]) == OK       # member 2 of 3 has no block of 2
    assert first_failure(3, [OK, OK, EH]) == EH
    assert first_failure(1, [EH, ND, ND]) == EH
    assert [rsmi.partition(2, 3, i)[1] for i in range(3)] == [1, 1, 0]
    assert batch_sizes(2) == [1, 2, 3, 5] and batch_sizes(3) == [1, 2, 3, 4, 7] and batch_sizes(4) == [1, 3, 4, 5, 9]
    assert max(batch_sizes(4)) == REF_NB


# ---------------------------------------------------------------- references, computed once
class Ref:
    """REF_NB blocks of (k, S) data, block b from splitmix64_bytes(SEED ^ b), with the oracle's
    parity, every row's CRC-16/IBM and CRC-32, and the oracle's reconstruct per loss pattern.
    Read-only."""

    def __init__(self, k, m, S, nb=REF_NB):
        self.k, self.m, self.n, self.S, self.nb = k, m, k + m, S, nb
        data = np.stack([orc.splitmix64_bytes(SEED ^ b, k * S).reshape(k, S) for b in range(nb)])
        self.rows = np.concatenate([data, orc.encode_fast(k, m, data)], axis=1)
        self.rows.setflags(write=False)
        self.data, self.parity = self.rows[:, :k], self.rows[:, k:]
        self.crc16 = [[orc.crc16_ibm(r.tobytes()) for r in blk] for blk in self.rows]
        self.crc32 = [[zlib.crc32(r.tobytes()) for r in blk] for blk in self.rows]
        assert self.crc32[0][0] == orc.crc32_ieee(self.rows[0, 0].tobytes())
        self._rebuilt = {}

    def rebuilt(self, lost):
        """(nb, n, S): every block after the oracle's Reconstruct with the rows of `lost` erased."""
        key = tuple(lost)
        if key not in self._rebuilt:
            out = np.empty_like(self.rows)
            for b in range(self.nb):
                erased = self.rows[b].copy()
                erased[list(lost)] = 0
                rc, out[b] = orc.reconstruct(self.k, self.m, erased, [i not in lost for i in range(self.n)], False)
                assert rc == 0, rc
            out.setflags(write=False)
            self._rebuilt[key] = out
        return self._rebuilt[key]


_REFS = {}


def ref_of(k, m, S):
    if (k, m, S) not in _REFS:
        _REFS[(k, m, S)] = Ref(k, m, S)
    return _REFS[(k, m, S)]


# ---------------------------------------------------------------- buffers and calls
class Arena:
    """Byte buffers over pageable memory or page-locked rsmi_host_alloc memory.  free() first
    takes the views of the cases built on it away (Case.release), so no numpy array is left over
    memory that went back to the runtime: pytest's report of a failed test prints the arguments of
    every frame, after the test's own finally has run, and would read freed memory through one."""

    def __init__(self):
        self.ptrs, self.cases = [], []

    def full(self, nbytes, fill, pinned=False):
        if not pinned:
            a = np.full(nbytes, fill, dtype=np.uint8)
            return a.ctypes.data, a
        p = rsmi.lib().rsmi_host_alloc(nbytes)
        assert p
        self.ptrs.append(p)
        a = np.ctypeslib.as_array((ctypes.c_uint8 * nbytes).from_address(p))
        a[:] = fill
        return p, a

    def free(self):
        for c in self.cases:
            c.release()
        for p in self.ptrs:
            rsmi.lib().rsmi_host_free(p)
        self.ptrs, self.cases = [], []


def _rows(buf, nb, nrows, S, bs):
    return np.lib.stride_tricks.as_strided(buf, shape=(nb, nrows, S), strides=(bs, S, 1))


def _assert_same(got, want, ctx):
    if np.array_equal(got, want):
        return
    bad = np.flatnonzero(got != want)
    raise AssertionError("%r: %d of %d bytes differ, first at %d (got %#x, want %#x), last at %d" %
                         (ctx, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]], bad[-1]))


def _mask(n, rows):
    return (ctypes.c_uint8 * n)(*[1 if i in rows else 0 for i in range(n)])


def _check_raw(ref, first, nb, raw16, raw32, ctx):
    """Every slot of the nb blocks is R / R32 of its row; the extra block is still poisoned."""
    for name, raw, want, entry in (("crc16", raw16, ref.crc16, rsmi.crc16_entry),
                                   ("crc32", raw32, ref.crc32, rsmi.crc32_entry)):
        if raw is None:
            continue
        assert (raw[nb] == POISON).all(), ctx + (name, "poison", raw[nb].tolist())
        for b in range(nb):
            for r in range(ref.n):
                v = int(raw[b, r])
                assert name == "crc32" or v < 0x10000, ctx + (name, b, r, v)
                assert entry(b"", v, ref.S) == want[first + b][r], ctx + (name, b, r)


class Case:
    """The buffers of one batch: blocks first .. first + nb - 1 of a reference in a data buffer, a
    parity buffer and a shards buffer, each with PAD bytes after every block and TAIL bytes past
    the last (pad = False: tight strides).  h is a group handle, or a context with group=False."""

    def __init__(self, ref, nb, first=0, pinned=False, arena=None, pad=True):
        self.ref, self.nb, self.first = ref, nb, first
        self.arena = arena or Arena()
        k, m, n, S = ref.k, ref.m, ref.n, ref.S
        pd = PAD if pad else (0, 0, 0)
        self.dbs, self.pbs, self.sbs = k * S + pd[0], m * S + pd[1], n * S + pd[2]
        self.dptr, self.data = self.arena.full(nb * self.dbs + TAIL, GAPFILL, pinned)
        _rows(self.data, nb, k, S, self.dbs)[:] = ref.data[first:first + nb]
        self.data0 = self.data.copy()
        self.pptr, self.par = self.arena.full(nb * self.pbs + TAIL, SENT, pinned)
        self.sptr, self.sh = self.arena.full(nb * self.sbs + TAIL, GAPFILL, pinned)
        self.arena.cases.append(self)

    def release(self):
        self.data = self.data0 = self.par = self.sh = None
        self.dptr = self.pptr = self.sptr = None

    def _ctx(self, *more):
        return (self.ref.k, self.ref.m, self.ref.S, self.nb, self.first) + more

    def call_encode(self, h, crcs=None, group=True, nb=None):
        """The status of one encode of the first nb blocks: crcs None is rsmi_(group_)encode_batch_host,
        (crc16, crc32) the _crcs form with those outputs.  The parity buffer starts as the sentinel."""
        L, S = rsmi.lib(), self.ref.S
        nb = self.nb if nb is None else nb
        self.par[:] = SENT
        self.raw16 = self.raw32 = None
        if crcs is None:
            fn = L.rsmi_group_encode_batch_host if group else L.rsmi_encode_batch_host
            return fn(h, self.dptr, self.dbs, self.pptr, self.pbs, S, nb)
        if crcs[0]:
            self.raw16 = np.full((nb + 1, self.ref.n), POISON, dtype=np.uint32)
        if crcs[1]:
            self.raw32 = np.full((nb + 1, self.ref.n), POISON, dtype=np.uint32)
        fn = L.rsmi_group_encode_batch_host_crcs if group else L.rsmi_encode_batch_host_crcs
        return fn(h, self.dptr, self.dbs, self.pptr, self.pbs, S, nb,
                  self.raw16.ctypes.data if crcs[0] else None, self.raw32.ctypes.data if crcs[1] else None)

    def check_encode(self, nb=None, ctx=()):
        """After an encode that returned OK: the whole parity buffer (rows, gaps, tail and the
        blocks past nb), the untouched data buffer, and every raw slot."""
        ref = self.ref
        nb = self.nb if nb is None else nb
        ctx = self._ctx("encode", nb) + ctx
        want = np.full(self.par.size, SENT, dtype=np.uint8)
        _rows(want, nb, ref.m, ref.S, self.pbs)[:] = ref.parity[self.first:self.first + nb]
        _assert_same(self.par.copy(), want, ctx + ("parity",))  # copies: see Arena
        _assert_same(self.data.copy(), self.data0, ctx + ("data",))
        _check_raw(ref, self.first, nb, self.raw16, self.raw32, ctx)

    def encode(self, h, crcs=None, group=True, nb=None, ctx=()):
        rc = self.call_encode(h, crcs, group, nb)
        assert rc == rsmi.OK, self._ctx("encode", crcs, rc) + ctx
        self.check_encode(nb, ctx)

    def _lose(self, lost):
        ref = self.ref
        self.sh[:] = GAPFILL
        v = _rows(self.sh, self.nb, ref.n, ref.S, self.sbs)
        v[:] = ref.rows[self.first:self.first + self.nb]
        v[:, list(lost)] = SENT
        return self.sh.copy()

    def _check_rebuilt(self, before, lost, rebuilt, ctx):
        """The shards buffer is `before` with the rows of `rebuilt` as the oracle rebuilds them:
        present rows, lost rows nobody asked for, gaps and tail are all as they were."""
        ref = self.ref
        want = before
        src = ref.rebuilt(lost)[self.first:self.first + self.nb]
        _rows(want, self.nb, ref.n, ref.S, self.sbs)[:, list(rebuilt)] = src[:, list(rebuilt)]
        _assert_same(self.sh.copy(), want, self._ctx(*ctx))  # a copy: see Arena

    def reconstruct(self, h, lost, data_only, ctx=()):
        L, ref = rsmi.lib(), self.ref
        before = self._lose(lost)
        present = _mask(ref.n, [i for i in range(ref.n) if i not in lost])
        rc = L.rsmi_group_reconstruct_batch_host(h, self.sptr, self.sbs, ref.S, self.nb, present, 1 if data_only else 0)
        assert rc == rsmi.OK, self._ctx("reconstruct", rc) + ctx
        rebuilt = [i for i in lost if i < ref.k or not data_only]
        self._check_rebuilt(before, lost, rebuilt, ("reconstruct", tuple(lost), data_only) + ctx)

    def reconstruct_rows(self, h, lost, required, ctx=()):
        L, ref = rsmi.lib(), self.ref
        before = self._lose(lost)
        present = _mask(ref.n, [i for i in range(ref.n) if i not in lost])
        rc = L.rsmi_group_reconstruct_rows_batch_host(h, self.sptr, self.sbs, ref.S, self.nb, present,
                                                      _mask(ref.n, required))
        assert rc == rsmi.OK, self._ctx("rows", rc) + ctx
        self._check_rebuilt(before, lost, required, ("rows", tuple(lost), tuple(required)) + ctx)


def rows_patterns(k, m):
    """(lost, required) of the rows reconstruct: see the module docstring."""
    if m >= 3:
        return [((0, 2, k), (2, k))]
    return [((0, 2), (2,)), ((0, k), (k,))]


def kernels(g):
    L = rsmi.lib()
    return [L.rsmi_last_kernel(L.rsmi_group_context(g._h, i)).decode() for i in range(g.size())]


def set_member_option(g, i, key, value):
    L = rsmi.lib()
    assert L.rsmi_set_option(L.rsmi_group_context(g._h, i), key.encode(), value) == rsmi.OK


# ---------------------------------------------------------------- leg 0: CPU
def _no_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")


def _validation_cases(k, m, S, d, p, s):
    """(name, group function, context function, arguments after the handle and before nblocks,
    arguments after nblocks, stated status)."""
    L = rsmi.lib()
    n = k + m
    everything = _mask(n, range(n))
    one_lost = _mask(n, range(1, n))
    too_few = _mask(n, range(n - k + 1, n))       # k - 1 present, row 0 among the lost
    row0, row1 = _mask(n, [0]), _mask(n, [1])
    INV, NODATA, FEW, OK = rsmi.ErrInvalidArg, rsmi.ErrShardNoData, rsmi.ErrTooFewShards, rsmi.OK
    enc = [("null data", (None, k * S, p, m * S, S), INV), ("null parity", (d, k * S, None, m * S, S), INV),
           ("S == 0", (d, k * S, p, m * S, 0), NODATA), ("short data stride", (d, k * S - 1, p, m * S, S), INV),
           ("short parity stride", (d, k * S, p, m * S - 1, S), INV)]
    out = []
    for name, a, want in enc:
        out.append(("encode: " + name, L.rsmi_group_encode_batch_host, L.rsmi_encode_batch_host, a, (), want))
        out.append(("encode_crcs: " + name, L.rsmi_group_encode_batch_host_crcs, L.rsmi_encode_batch_host_crcs, a,
                    (None, None), want))
    G, C = L.rsmi_group_reconstruct_batch_host, L.rsmi_reconstruct_batch_host
    for name, a, b, want in [("null shards", (None, n * S, S), (one_lost, 0), INV),
                             ("null present", (s, n * S, S), (None, 0), INV),
                             ("S == 0", (s, n * S, 0), (one_lost, 0), NODATA),
                             ("short stride", (s, n * S - 1, S), (one_lost, 0), INV),
                             ("nothing missing", (s, n * S, S), (everything, 0), OK),
                             ("no data row missing, data only", (s, n * S, S), (_mask(n, range(n - 1)), 1), OK),
                             ("too few present", (s, n * S, S), (too_few, 0), FEW)]:
        out.append(("reconstruct: " + name, G, C, a, b, want))
    G, C = L.rsmi_group_reconstruct_rows_batch_host, L.rsmi_reconstruct_rows_batch_host
    for name, a, b, want in [("null shards", (None, n * S, S), (one_lost, row0), INV),
                             ("null present", (s, n * S, S), (None, row0), INV),
                             ("null required", (s, n * S, S), (one_lost, None), INV),
                             ("S == 0", (s, n * S, 0), (one_lost, row0), NODATA),
                             ("short stride", (s, n * S - 1, S), (one_lost, row0), INV),
                             ("required rows present", (s, n * S, S), (one_lost, row1), OK),
                             ("too few present", (s, n * S, S), (too_few, row0), FEW)]:
        out.append(("rows: " + name, G, C, a, b, want))
    return out


@pytest.mark.parametrize("k,m,S", SHAPES)
def test_group_validates_like_member_zero(k, m, S):
    """nblocks > 0 and no device: every argument error, and every call with nothing to rebuild,
    comes back from the group exactly as from member 0's context on member 0's range (start 0,
    the same pointers, its count), and is the status include/rsmi.h states."""
    _no_gpu()
    L = rsmi.lib()
    n, nb, M = k + m, 5, 3
    data = np.zeros(nb * k * S, dtype=np.uint8)
    par = np.zeros(nb * m * S, dtype=np.uint8)
    sh = np.zeros(nb * n * S, dtype=np.uint8)
    st0, cnt0 = rsmi.partition(nb, M, 0)
    assert st0 == 0 and cnt0 == 2
    with rsmi.DeviceGroup(k, m, [0] * M) as g:
        ctx0 = L.rsmi_group_context(g._h, 0)
        for name, gfn, cfn, a, b, want in _validation_cases(k, m, S, data.ctypes.data, par.ctypes.data,
                                                            sh.ctypes.data):
            got = gfn(g._h, *a, nb, *b)
            assert got == cfn(ctx0, *a, cnt0, *b) == want, (name, got, want)
        assert kernels(g) == [""] * M
    assert not data.any() and not par.any() and not sh.any()


@pytest.mark.parametrize("armed,nb,stated", [(0, 5, rsmi.ErrHost), (1, 5, rsmi.ErrNoDevice), (2, 5, rsmi.ErrNoDevice),
                                             (0, 1, rsmi.ErrHost)])
def test_first_failing_member_decides_without_gpu(armed, nb, stated):
    """Three members and no device: every member's encode fails with ERR_NO_DEVICE, except the one
    armed with inject_host_fault = 1, which throws first and reports ERR_HOST once.  The group
    returns the first failure in member order, not the last and not the armed member's."""
    _no_gpu()
    k, m, S, M = 4, 2, 1000, 3
    case = Case(ref_of(k, m, S), nb, pad=False)
    with rsmi.DeviceGroup(k, m, [0] * M) as g:
        assert case.call_encode(g._h) == rsmi.ErrNoDevice
        set_member_option(g, armed, "inject_host_fault", 1)
        statuses = [rsmi.ErrHost if i == armed else rsmi.ErrNoDevice for i in range(M)]
        want = first_failure(nb, statuses)
        assert want == stated
        assert case.call_encode(g._h, (True, True)) == want
        if nb == 5:  # the hook fired once (every member ran): the next call is the plain failure
            assert case.call_encode(g._h) == rsmi.ErrNoDevice
    assert (case.par == SENT).all()


# ---------------------------------------------------------------- GPU plumbing
@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available() or rsmi.device_count() == 0:
        pytest.skip("no GPU")
    yield torch
    _REFS.clear()


def _leg1_params():
    return [pytest.param(k, m, S, M, nb, id="rs%d_%d-M%d-nb%d" % (k, m, M, nb))
            for k, m, S in SHAPES for M in (2, 3, 4) for nb in batch_sizes(M)]


# ---------------------------------------------------------------- leg 1: seams and short batches
@pytest.mark.gpu
@pytest.mark.parametrize("k,m,S,M,nb", _leg1_params())
def test_group_seams_short_batches_padded(gpu, k, m, S, M, nb):
    """Pageable memory, default options, padded strides: every entry point at nb below, at and
    above the member count.  The first call on the fresh group is the plain encode: afterwards a
    member has launched the unaligned-window encode kernel if and only if its part is not empty."""
    ref = ref_of(k, m, S)
    counts = [rsmi.partition(nb, M, i)[1] for i in range(M)]
    assert sum(counts) == nb and (nb >= M or 0 in counts)
    case = Case(ref, nb)
    with rsmi.DeviceGroup(k, m, member_devices(M)) as g:
        assert kernels(g) == [""] * M
        case.encode(g._h)
        assert kernels(g) == [fast_label(k, m) + ",UA" if c else "" for c in counts], (kernels(g), counts)
        for crcs in ((True, True), (True, False), (False, True), (False, False)):
            case.encode(g._h, crcs)
        lost = (1, k + 1)
        case.reconstruct(g._h, lost, False)
        case.reconstruct(g._h, lost, True)
        for lost, required in rows_patterns(k, m):
            case.reconstruct_rows(g._h, lost, required)
        got = kernels(g)
        for i, c in enumerate(counts):  # an empty part launched nothing in any of the calls
            assert got[i].startswith(fast_label(k, len(required)) + ",UA") if c else got[i] == "", (got, counts)


# ---------------------------------------------------------------- leg 2: the three host paths
@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["pipeline", "in_place", "mixed"])
def test_group_host_paths(gpu, variant):
    """RS(10,4), S = 2049, three members, seven blocks, padded strides: the encode with both CRCs,
    then the rows reconstruct.  "pipeline": pageable memory and small_call_bytes = 0 on every
    member, so every range goes through the copy engines and pitched, aligned staging (a label
    without ",UA").  "in_place": rsmi_host_alloc buffers, one kernel per range where the rows lie
    (",UA").  "mixed": pageable memory and small_call_bytes = 0 on member 1 only, so the members
    of one call take different paths (page-locked buffers are coded in place whatever
    small_call_bytes says, so only pageable memory lets the option split the members)."""
    k, m, S, M, nb = 10, 4, 2049, 3, 7
    ref = ref_of(k, m, S)
    counts = [rsmi.partition(nb, M, i)[1] for i in range(M)]
    assert counts == [3, 2, 2]
    (lost, required), = rows_patterns(k, m)
    rec = fast_label(k, len(required))
    arena = Arena()
    try:
        case = Case(ref, nb, pinned=variant == "in_place", arena=arena)
        with rsmi.DeviceGroup(k, m, member_devices(M)) as g:
            piped = {"pipeline": [0, 1, 2], "in_place": [], "mixed": [1]}[variant]
            for i in piped:
                set_member_option(g, i, "small_call_bytes", 0)
            want_enc = [fast_label(k, m) + ("" if i in piped else ",UA") for i in range(M)]
            want_rec = [rec + ("" if i in piped else ",UA") for i in range(M)]
            case.encode(g._h, ctx=(variant,))
            assert kernels(g) == want_enc, (variant, kernels(g))
            case.encode(g._h, (True, True), ctx=(variant,))
            case.reconstruct_rows(g._h, lost, required, ctx=(variant,))
            assert kernels(g) == want_rec, (variant, kernels(g))
            case.encode(g._h, (True, True), ctx=(variant, "again"))
    finally:
        arena.free()


# ---------------------------------------------------------------- leg 3: a failing member
@pytest.mark.gpu
def test_group_failing_member(gpu):
    """inject_host_fault = 1 on one member throws in that member's next encode before anything is
    launched.  Member 1 armed: the call is ERR_HOST, and the next call is OK with every byte right,
    so the workers and the contexts survive.  Member 2 armed and two blocks: member 2's part is
    empty and is not run, so the call is OK and the hook stays armed; with three blocks it fires."""
    k, m, S, M = 4, 2, 1000, 3
    ref = ref_of(k, m, S)
    OK, EH = rsmi.OK, rsmi.ErrHost
    case = Case(ref, 5)
    with rsmi.DeviceGroup(k, m, member_devices(M)) as g:
        case.encode(g._h, (True, True))
        set_member_option(g, 1, "inject_host_fault", 1)
        assert first_failure(5, [OK, EH, OK]) == EH
        assert case.call_encode(g._h, (True, True)) == EH
        case.encode(g._h, (True, True), ctx=("after member 1 failed",))
        case.reconstruct(g._h, (1, k + 1), False, ctx=("after member 1 failed",))

        set_member_option(g, 2, "inject_host_fault", 1)
        assert first_failure(2, [OK, OK, EH]) == OK and first_failure(3, [OK, OK, EH]) == EH
        case.encode(g._h, (True, True), nb=2, ctx=("member 2 armed, part empty",))
        assert case.call_encode(g._h, (True, True), nb=3) == EH
        case.encode(g._h, (True, True), nb=3, ctx=("after member 2 failed",))
        case.encode(g._h, ctx=("after member 2 failed",))


# ---------------------------------------------------------------- leg 4: callers
@pytest.mark.gpu
@pytest.mark.parametrize("k,m,S", SHAPES)
def test_two_threads_on_one_group_and_one_on_a_member(gpu, k, m, S):
    """Two threads share a three-member group, each with its own buffers, its own blocks and its
    own batch size (5 and 8), eight calls each, alternating the encode with both CRCs and a
    reconstruct; a third thread encodes on member 0's context directly for as long as they run.
    Every call of every thread is compared with the oracle."""
    L = rsmi.lib()
    ref = ref_of(k, m, S)
    lost = (1, k + 1)
    errors, done = [], threading.Event()
    direct_calls = []

    def guarded(fn):
        def run():
            try:
                fn()
            except BaseException as e:  # noqa: BLE001 - reported by the main thread
                errors.append(e)
        return run

    with rsmi.DeviceGroup(k, m, member_devices(3)) as g:
        def group_caller(nb, first):
            case = Case(ref, nb, first=first)

            def body():
                for i in range(8):
                    if i % 2 == 0:
                        case.encode(g._h, (True, True), ctx=("thread", nb, i))
                    else:
                        case.reconstruct(g._h, lost, i % 4 == 1, ctx=("thread", nb, i))
            return body

        def direct():
            case = Case(ref, 3, first=6)
            ctx0 = L.rsmi_group_context(g._h, 0)
            while len(direct_calls) < 4 or not done.is_set():
                case.encode(ctx0, group=False, ctx=("direct", len(direct_calls)))
                direct_calls.append(1)

        callers = [threading.Thread(target=guarded(group_caller(5, 0))),
                   threading.Thread(target=guarded(group_caller(8, 1)))]
        third = threading.Thread(target=guarded(direct))
        for t in callers + [third]:
            t.start()
        for t in callers:
            t.join()
        done.set()
        third.join()
    if errors:
        raise errors[0]
    assert len(direct_calls) >= 4


@pytest.mark.gpu
def test_wait_hook_is_not_taken_by_a_group_call(gpu):
    """The wait hook belongs to the calling thread and the group codes on its workers: a one-block
    group encode on page-locked memory (the call that would run the hook on a single context)
    leaves it pending, and rsmi_run_wait_hook then runs it once.  The ctypes callback as in
    test_abi.py."""
    L = rsmi.lib()
    k, m, S = 4, 2, 1000
    ran = []
    cb = ctypes.CFUNCTYPE(None, ctypes.c_void_p)(lambda arg: ran.append(arg))
    arena = Arena()
    try:
        case = Case(ref_of(k, m, S), 1, pinned=True, arena=arena)
        with rsmi.DeviceGroup(k, m, member_devices(2)) as g:
            assert L.rsmi_run_wait_hook() == 0
            L.rsmi_set_wait_hook(cb, 7)
            try:
                case.encode(g._h, (True, False))
                assert ran == []
                assert L.rsmi_run_wait_hook() == 1 and ran == [7]
                assert L.rsmi_run_wait_hook() == 0 and ran == [7]
            finally:
                L.rsmi_set_wait_hook(None, None)
    finally:
        arena.free()


# ---------------------------------------------------------------- leg 5: rsmi_group_host_alloc edges
def _check_member_pages(g, p, block_bytes, nblocks):
    """Where the members report different NUMA nodes: every whole page of each member's block range
    is on the member's node (get_mempolicy with MPOL_F_NODE | MPOL_F_ADDR, as test_device_group.py).
    Returns the members' nodes."""
    M = g.size()
    nodes = [g.member_numa_node(i) for i in range(M)]
    assert nodes == [rsmi.device_numa_node(d) for d in g.devices]
    if len(set(nodes)) < 2:
        return nodes
    libc = ctypes.CDLL(ctypes.util.find_library("c"), use_errno=True)
    page = mmap.PAGESIZE
    mode = ctypes.c_int(-1)
    for i, node in enumerate(nodes):
        st, cnt = rsmi.partition(nblocks, M, i)
        lo = -(-st * block_bytes // page) * page
        hi = (st + cnt) * block_bytes // page * page
        for off in range(lo, hi, page) if node >= 0 else ():
            rc = libc.syscall(239, ctypes.byref(mode), None, ctypes.c_ulong(0), ctypes.c_void_p(p + off),
                              ctypes.c_ulong(3))
            assert rc == 0 and mode.value == node, (i, off, rc, mode.value, node)
    return nodes


def _group_buffer(g, ptrs, block_bytes, nblocks):
    p = g.host_alloc(block_bytes, nblocks)
    ptrs.append(p)
    a = np.ctypeslib.as_array((ctypes.c_uint8 * (block_bytes * nblocks)).from_address(p))
    zeroed = not a.any()
    assert zeroed
    return p, a


@pytest.mark.gpu
@pytest.mark.parametrize("k,m,S,M,nb,split", [(4, 2, 1000, 3, 1, False), (4, 2, 25, 3, 3, True),
                                              (4, 2, 1000, 2, 5, False), (10, 4, 2049, 2, 5, False)],
                         ids=["one_block", "one_page", "mid_page_seam-rs4_2", "mid_page_seam-rs10_4"])
def test_group_host_alloc_edges(gpu, k, m, S, M, nb, split):
    """rsmi_group_host_alloc where its page arithmetic has edges: fewer blocks than members;
    block_bytes = 100 and three blocks, every member range inside the first page; two members
    whose seam (block 3 of 5 blocks of n*S bytes) falls in the middle of a page.  The buffer is
    non-null and zeroed, and coding it in place through the group gives the oracle's bytes: the
    encode in all of them (split: the data blocks in one allocation of 100-byte blocks and the
    parity in another; otherwise whole n*S blocks, the parity rows after the data rows), and a
    full reconstruct in place in the mid-page ones."""
    L = rsmi.lib()
    n = k + m
    ref = ref_of(k, m, S) if S != 25 else Ref(k, m, S, nb)
    page = mmap.PAGESIZE
    with rsmi.DeviceGroup(k, m, member_devices(M)) as g:
        ptrs = []
        try:
            if split:
                assert k * S == 100 and nb * k * S <= page
                pd, d = _group_buffer(g, ptrs, k * S, nb)
                pp, p = _group_buffer(g, ptrs, m * S, nb)
                d[:] = ref.data[:nb].reshape(-1)
                assert L.rsmi_group_encode_batch_host(g._h, pd, k * S, pp, m * S, S, nb) == rsmi.OK
                _assert_same(p.copy(), ref.parity[:nb].reshape(-1), ("split", "parity"))  # copies: see Arena
                _assert_same(d.copy(), ref.data[:nb].reshape(-1), ("split", "data"))
                _check_member_pages(g, pd, k * S, nb)
            else:
                bs = n * S
                ps, s = _group_buffer(g, ptrs, bs, nb)
                if nb > M:
                    assert (rsmi.partition(nb, M, 1)[0] * bs) % page != 0
                rows = s.reshape(nb, n, S)
                rows[:, :k] = ref.data[:nb]
                assert L.rsmi_group_encode_batch_host(g._h, ps, bs, ps + k * S, bs, S, nb) == rsmi.OK
                _assert_same(s.copy(), ref.rows[:nb].reshape(-1), ("in place", "encode"))
                if nb > M:
                    lost = (1, k + 1)
                    rows[:, list(lost)] = SENT
                    present = _mask(n, [i for i in range(n) if i not in lost])
                    assert L.rsmi_group_reconstruct_batch_host(g._h, ps, bs, S, nb, present, 0) == rsmi.OK
                    _assert_same(s.copy(), ref.rebuilt(lost)[:nb].reshape(-1), ("in place", "reconstruct"))
                _check_member_pages(g, ps, bs, nb)
        finally:
            d = p = s = rows = None  # no view outlives the memory (see Arena)
            for q in ptrs:
                g.host_free(q)
