"""The mutcask value checksum (CRC-32, crc32.hpp) on the paths test_crc32.py does not reach, and
the same shapes of gap in the CRC-16 rows pass.

The reference for legs 1 and 5 is built here from zlib alone: the zero-byte step A of the CRC
register as a 32 x 32 matrix over GF(2) (its columns read off zlib.crc32), and A^n by repeated
squaring on Python ints.  It shares no code with the library's tables or with oracle_lib, and a
CPU test anchors it to zlib on real data.  The CRC-16 twin is built the same way from
orc.crc16_ibm, assuming only that the zero-byte step is linear.

  leg 1 (CPU)  rsmi_crc32_entry / rsmi_crc16_entry at every power of two of data_len up to 2^40,
               and past 2^32 and 2^63
  leg 2 (GPU)  rsmi_encode_block_coalesced_crcs with a CRC-32 output: mixed requests, every
               memory mode, the table rule, a lone caller, the pipeline, several lanes
  leg 3 (GPU)  many short items per wave in both rows passes (waves_per_cu 1, >= 4 rows per CU)
  leg 4 (GPU)  one context across shard sizes, folds and layouts, queued without a host sync
  leg 5 (GPU)  rows past 2 GiB: each column-form segment power SC[i] = A^(8192 * 2^i), i < 19, alone
"""
import ctypes
import functools
import random
import threading
import zlib

import numpy as np
import pytest

import oracle_lib as orc
import rsmi

M32 = 0xFFFFFFFF
POISON = 0xA5A5A5A5


def raw32(data: bytes) -> int:
    """R32(D), the register after D from zero: zlib.crc32(D, v) = ~fold(~v, D)."""
    return ~zlib.crc32(data, M32) & M32


# ---------------------------------------------------------------------------------------------
# The reference: "append n zero bytes" as a GF(2) matrix power
# ---------------------------------------------------------------------------------------------

def _apply(cols, s):
    v, b = 0, 0
    while s:
        if s & 1:
            v ^= cols[b]
        s >>= 1
        b += 1
    return v


def _square(cols):
    return [_apply(cols, c) for c in cols]


def _fold32(s, data):
    """The CRC-32 register after `data` from state s, by zlib only."""
    return ~zlib.crc32(data, ~s & M32) & M32


@functools.lru_cache(maxsize=None)
def _pows32():
    """[A^(2^i) for i < 64], each as the images of the 32 basis vectors."""
    p = [[_fold32(1 << b, b"\0") for b in range(32)]]
    for _ in range(63):
        p.append(_square(p[-1]))
    return p


def shift_ref(s, n):
    """A^n(s): the CRC-32 register s after n more zero bytes."""
    assert 0 <= n < 1 << 64
    for i, cols in enumerate(_pows32()):
        if (n >> i) & 1:
            s = _apply(cols, s)
    return s


def _state16(data):
    """The CRC-16 register after `data` from 0xFFFF (crc16_ibm complements it on exit)."""
    return ~orc.crc16_ibm(data) & 0xFFFF


@functools.lru_cache(maxsize=None)
def _pows16():
    """[A16^(2^i) for i < 64] from the oracle's byte step: every D gives one pair
    (state(D), state(D || 0)) = (v, A16 v); 16 independent v determine the linear map."""
    rng = random.Random(16)
    basis = {}  # leading bit -> (v, A16 v)

    def reduce(v, w):
        for p in sorted(basis, reverse=True):
            if (v >> p) & 1:
                v ^= basis[p][0]
                w ^= basis[p][1]
        return v, w

    while len(basis) < 16:
        d = bytes(rng.randrange(256) for _ in range(2))
        v, w = reduce(_state16(d), _state16(d + b"\0"))
        if v:
            basis[v.bit_length() - 1] = (v, w)
    cols = []
    for b in range(16):
        v, w = reduce(1 << b, 0)
        assert v == 0
        cols.append(w)
    p = [cols]
    for _ in range(63):
        p.append(_square(p[-1]))
    return p


def shift16_ref(s, n):
    assert 0 <= n < 1 << 64
    for i, cols in enumerate(_pows16()):
        if (n >> i) & 1:
            s = _apply(cols, s)
    return s


def raw16(row: bytes) -> int:
    """R16(row), the register after the row from zero: Checksum(row) = ~(A^|row|(0xFFFF) ^ R16)."""
    return _state16(row) ^ shift16_ref(0xFFFF, len(row))


ANCHOR_N = [1, 15, 16, 1023, 8192, 70001]


def test_reference_anchored_to_zlib():
    r = random.Random(32)
    for n in ANCHOR_N:
        for plen in (0, 1, 9, 300):
            p = bytes(r.randrange(256) for _ in range(plen))
            assert shift_ref(raw32(p), n) == raw32(p + bytes(n)), (plen, n)
            # and from the complemented start, as rsmi_crc32_entry uses it
            assert ~shift_ref(~zlib.crc32(p) & M32, n) & M32 == zlib.crc32(p + bytes(n)), (plen, n)


def test_reference16_anchored_to_oracle():
    r = random.Random(17)
    for n in ANCHOR_N + [32766, 32767, 32768]:
        for plen in (0, 1, 9, 300):
            p = bytes(r.randrange(256) for _ in range(plen))
            assert shift16_ref(_state16(p), n) == _state16(p + bytes(n)), (plen, n)
    row = bytes(r.randrange(256) for _ in range(777))
    s = 0  # raw16 against a plain bit-serial register from zero
    for x in row:
        s ^= x
        for _ in range(8):
            s = (s >> 1) ^ 0xA001 if s & 1 else s >> 1
    assert raw16(row) == s


# ---------------------------------------------------------------------------------------------
# Leg 1: the host half at every length
# ---------------------------------------------------------------------------------------------

ENTRY_LENS = sorted({n for i in range(41) for n in ((1 << i) - 1, 1 << i, (1 << i) + 1)} |
                    {(1 << 32) - 1, 1 << 32, (1 << 32) + 7, (1 << 40) + 3, (1 << 63) + 11})


def test_binding_passes_64_bit_lengths():
    L = rsmi.lib()
    assert ctypes.sizeof(ctypes.c_size_t) == 8
    for f in (L.rsmi_crc32_entry, L.rsmi_crc16_entry):
        assert f.argtypes[1] is ctypes.c_size_t and f.argtypes[3] is ctypes.c_size_t
    # bits 32..63 of data_len reach the library: the results differ where the reference's do
    # (A has order 2^32 - 1, so 2^32 zero bytes act as one and 2^63 as 2^31)
    s = 0x12345678
    assert shift_ref(s, 1 << 32) == shift_ref(s, 1) != s
    assert shift_ref(s, 1 << 63) == shift_ref(s, 1 << 31) != s
    for n in (1 << 32, 1 << 63):
        assert rsmi.crc32_entry(b"", 0, n) != rsmi.crc32_entry(b"", 0, 0), hex(n)
        assert rsmi.crc16_entry(b"", 0, n) != rsmi.crc16_entry(b"", 0, 0), hex(n)


def test_crc32_entry_4gib_value():
    """The confirmed case: no head, raw 0x12345678, 2^32 data bytes."""
    want = ~(shift_ref(M32, 1 << 32) ^ 0x12345678) & M32
    assert want == 0xC036B9F5
    assert rsmi.crc32_entry(b"", 0x12345678, 1 << 32) == want


@pytest.mark.parametrize("head_len", [0, 16])
def test_crc32_entry_every_length(head_len):
    """ChecksumIEEE(head || D) from R32(D) and |D| = ~(A^|D|(register after head) ^ R32(D)), for
    |D| = 2^i - 1, 2^i, 2^i + 1 (i <= 40) and past 2^32, 2^40 and 2^63."""
    r = random.Random(1000 + head_len)
    head = bytes(r.randrange(256) for _ in range(head_len))
    s0 = ~zlib.crc32(head) & M32
    bad = []
    for n in ENTRY_LENS:
        raw = r.getrandbits(32)
        want = ~(shift_ref(s0, n) ^ raw) & M32
        got = rsmi.crc32_entry(head, raw, n)
        if got != want:
            bad.append((hex(n), hex(got), hex(want)))
    assert bad == []


@pytest.mark.parametrize("head_len", [0, 16])
def test_crc16_entry_every_length(head_len):
    """The same sweep for the datanode CRC-16 (the library reduces by the group order 32767)."""
    r = random.Random(2000 + head_len)
    head = bytes(r.randrange(256) for _ in range(head_len))
    s0 = _state16(head)
    bad = []
    for n in ENTRY_LENS:
        raw = r.getrandbits(16)
        want = ~(shift16_ref(s0, n) ^ raw) & 0xFFFF
        got = rsmi.crc16_entry(head, raw, n)
        if got != want:
            bad.append((hex(n), hex(got), hex(want)))
    assert bad == []


# ---------------------------------------------------------------------------------------------
# Leg 2: coalesced encode with R32
# ---------------------------------------------------------------------------------------------

BASELINE = ((2, 1), (4, 2), (10, 4), (16, 4))

COAL_SHAPES = [
    (10, 4, 262144, 12),  # S = 26215, unaligned windows
    (4, 2, 262144, 12),   # aligned rows
    (2, 1, 6, 8),         # S = 3: no fused form, separate passes, unaligned CRC-32 rows under 16 bytes
    (16, 4, 65543, 5),
    (5, 3, 70000, 7),     # no table kernels
    (20, 4, 5000, 5),     # k > 16: CRC-16 by the separate pass
    (4, 2, 4099, 70),     # more than kTableBlocks requests
]
COAL_MODES = ["pinned", "pinned_out", "pageable_small0", "pageable_small1g", "one_pageable"]


@functools.lru_cache(maxsize=None)
def _coal_ref(k, m, B, T, seed=0):
    """T random blocks and, per block, the oracle's n rows with both raw checksums' references."""
    rng = np.random.default_rng([k, m, B, T, seed])
    blocks, rows, c16, r32 = [], [], [], []
    for _ in range(T):
        b = bytes(rng.integers(0, 256, size=B, dtype=np.uint8))
        w = orc.split(k, m, b)
        w[k:] = orc.encode(k, m, w[:k])
        w.setflags(write=False)
        blocks.append(b)
        rows.append(w)
        c16.append([orc.crc16_ibm(x.tobytes()) for x in w])
        r32.append([raw32(x.tobytes()) for x in w])
    return blocks, rows, c16, r32


class _Bufs:
    """T shard buffers of n * S bytes, page-locked where pinned[t], else pageable."""

    def __init__(self, n, S, pinned):
        self.L = rsmi.lib()
        self.n, self.S = n, S
        self.hptrs, self.ptrs, self.views, self.keep = [], [], [], []
        for p in pinned:
            if p:
                a = self.L.rsmi_host_alloc(n * S)
                assert a
                self.hptrs.append(a)
                v = np.ctypeslib.as_array((ctypes.c_uint8 * (n * S)).from_address(a))
            else:
                v = np.zeros(n * S, dtype=np.uint8)
                a = v.ctypes.data
            self.ptrs.append(a)
            self.views.append(v)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.views = []
        for p in self.hptrs:
            self.L.rsmi_host_free(p)


def _wants_mixed(t):
    return (3, 2, 1, 0)[t % 4]  # bit 0: R16, bit 1: R32 -- both, R32 only, R16 only, neither


def _call_coalesced(c, bufs, B, blocks, wants, separate_block=False):
    """One rsmi_encode_block_coalesced_crcs call per block, each from its own thread.  Returns the
    status codes and the (n + 1)-word R16 / R32 arrays, poisoned before the call."""
    L, n = bufs.L, bufs.n
    T = len(blocks)
    srcs = []
    for t in range(T):
        bufs.views[t][:] = 0xA5  # stale bytes: padding and parity must be written
        if separate_block:
            s = bytearray(blocks[t])
            bufs.keep.append(s)
            srcs.append(ctypes.addressof((ctypes.c_char * B).from_buffer(s)))
        else:
            bufs.views[t][:B] = np.frombuffer(blocks[t], dtype=np.uint8)
            srcs.append(bufs.ptrs[t])
    o16 = [(ctypes.c_uint32 * (n + 1))(*([POISON] * (n + 1))) for _ in range(T)]
    o32 = [(ctypes.c_uint32 * (n + 1))(*([POISON] * (n + 1))) for _ in range(T)]
    rcs = [None] * T

    def enc(t):
        rcs[t] = L.rsmi_encode_block_coalesced_crcs(c._h, srcs[t], B, bufs.ptrs[t], o16[t] if wants[t] & 1 else None,
                                                    o32[t] if wants[t] & 2 else None)

    th = [threading.Thread(target=enc, args=(t,)) for t in range(T)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    bufs.keep.clear()
    return rcs, o16, o32


def _check_request(bufs, t, S, rows, c16, r32, want, o16, o32, tag=()):
    n = bufs.n
    assert np.array_equal(bufs.views[t].reshape(n, S), rows), tag + (t, "shards")
    if want & 1:
        for r in range(n):
            assert o16[r] < 0x10000 and rsmi.crc16_entry(b"", o16[r], S) == c16[r], tag + (t, r, "R16")
        assert o16[n] == POISON, tag + (t, "R16 past n")
    else:
        assert list(o16) == [POISON] * (n + 1), tag + (t, "R16 not asked for")
    if want & 2:
        for r in range(n):
            assert o32[r] == r32[r], tag + (t, r, "R32", hex(o32[r]), hex(r32[r]))
        assert o32[n] == POISON, tag + (t, "R32 past n")
    else:
        assert list(o32) == [POISON] * (n + 1), tag + (t, "R32 not asked for")


def _one_batch_codec(k, m, T):
    c = rsmi.Codec(k, m)
    c.set_option("coalesce_lanes", 1)
    c.set_option("coalesce_us", 100000)
    c.set_option("coalesce_max", T)
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("mode", COAL_MODES)
@pytest.mark.parametrize("k,m,B,T", COAL_SHAPES)
def test_coalesced_crcs_mixed_requests(k, m, B, T, mode):
    """One batch of T concurrent rsmi_encode_block_coalesced_crcs calls, request t asking for both
    checksums, R32 only, R16 only or neither (t % 4): DagNode.Put on a mutcask node.  Any R32
    request turns the table launch off, so a page-locked group runs a launch per request with
    its checksums at d16 / d32 + j * n and comes back through the read-back; a group with a
    pageable buffer stages through the host batch path.  Every row equals the oracle's Split +
    Encode, every checksum asked for equals the oracle's CRC-16 / zlib's CRC-32 of that row, and
    the outputs not asked for (and the word past the n-th) keep their poison."""
    n = k + m
    S = (B + k - 1) // k
    blocks, rows, c16, r32 = _coal_ref(k, m, B, T)
    pinned = [mode in ("pinned", "pinned_out") or (mode == "one_pageable" and t != T // 2) for t in range(T)]
    wants = [_wants_mixed(t) for t in range(T)]
    with _Bufs(n, S, pinned) as bufs, _one_batch_codec(k, m, T) as c:
        if mode.startswith("pageable_small"):
            c.set_option("small_call_bytes", 0 if mode == "pageable_small0" else 1 << 30)
        c.warm()
        b0 = c.stat("coalesced_batches")
        rcs, o16, o32 = _call_coalesced(c, bufs, B, blocks, wants, separate_block=(mode == "pinned_out"))
        assert rcs == [0] * T
        assert c.stat("coalesced_batches") - b0 == 1
        if all(pinned):
            assert ",TB" not in c.last_kernel(), c.last_kernel()  # R32 costs the table launch
        for t in range(T):
            _check_request(bufs, t, S, rows[t], c16[t], r32[t], wants[t], o16[t], o32[t])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["pinned", "pinned_out"])
@pytest.mark.parametrize("k,m,B,T", [s for s in COAL_SHAPES if (s[0], s[1]) in BASELINE and s[2] >= 16 * s[0]])
def test_coalesced_table_rule(k, m, B, T, mode):
    """The table rule on a page-locked group of a BASELINE shape: with no R32 request (R16 or
    nothing, by t % 2) the group is coded by table launches (",TB"); the same group with one R32
    request among them is not.  Results are checked both times."""
    n = k + m
    S = (B + k - 1) // k
    blocks, rows, c16, r32 = _coal_ref(k, m, B, T)
    with _Bufs(n, S, [True] * T) as bufs, _one_batch_codec(k, m, T) as c:
        c.warm()
        for one32 in (False, True, False):
            wants = [1 - t % 2 for t in range(T)]
            if one32:
                wants[T - 1] = 2
            b0 = c.stat("coalesced_batches")
            rcs, o16, o32 = _call_coalesced(c, bufs, B, blocks, wants, separate_block=(mode == "pinned_out"))
            assert rcs == [0] * T
            assert c.stat("coalesced_batches") - b0 == 1
            assert (",TB" in c.last_kernel()) == (not one32), (one32, c.last_kernel())
            for t in range(T):
                _check_request(bufs, t, S, rows[t], c16[t], r32[t], wants[t], o16[t], o32[t], (one32,))


@pytest.mark.gpu
@pytest.mark.parametrize("flag", [1, 0])
@pytest.mark.parametrize("want", [3, 2])
def test_coalesced_crcs_lone_caller(flag, want):
    """A lone caller (a batch of one) that wants R32, with the completion flag on and off: the
    flag belongs to the table launch, which R32 turns off, so neither setting may wait on it."""
    k, m, B = 10, 4, 262144
    n, S = k + m, (B + k - 1) // k
    blocks, rows, c16, r32 = _coal_ref(k, m, B, 1, seed=1)
    with _Bufs(n, S, [True]) as bufs, _one_batch_codec(k, m, 1) as c:
        c.set_option("coalesce_flag", flag)
        c.warm()
        for rep in range(2):
            rcs, o16, o32 = _call_coalesced(c, bufs, B, blocks, [want])
            assert rcs == [0]
            assert ",TB" not in c.last_kernel(), c.last_kernel()
            _check_request(bufs, 0, S, rows[0], c16[0], r32[0], want, o16[0], o32[0], (rep,))


@pytest.mark.gpu
def test_coalesced_crcs_pipeline_alternates():
    """coalesce_pipeline 1: six batches on the same buffers with fresh data each time, in turn
    "nobody wants R32" (the pipelined table launch, R16 landing in the pipeline's areas) and
    "everybody does" (synchronous, a launch per request).  Every batch is checked."""
    k, m, B, T = 10, 4, 262144, 6
    n, S = k + m, (B + k - 1) // k
    with _Bufs(n, S, [True] * T) as bufs, _one_batch_codec(k, m, T) as c:
        c.set_option("coalesce_pipeline", 1)
        c.warm()
        for i in range(6):
            blocks, rows, c16, r32 = _coal_ref(k, m, B, T, seed=10 + i)
            wants = [3 if t % 2 else 2 for t in range(T)] if i % 2 else [1] * T
            b0 = c.stat("coalesced_batches")
            rcs, o16, o32 = _call_coalesced(c, bufs, B, blocks, wants)
            assert rcs == [0] * T
            assert c.stat("coalesced_batches") - b0 == 1
            assert (",TB" in c.last_kernel()) == (i % 2 == 0), (i, c.last_kernel())
            for t in range(T):
                _check_request(bufs, t, S, rows[t], c16[t], r32[t], wants[t], o16[t], o32[t], (i,))


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [2, 4])
def test_coalesced_crcs_lanes(lanes):
    """16 concurrent callers over 2 and 4 coalescing lanes, three calls each with changing
    requests (both, R32, R16, neither).  Batching is not deterministic here: only the results and
    that some calls did share a batch are asserted."""
    k, m, B, T, per = 10, 4, 262144, 16, 3
    n, S = k + m, (B + k - 1) // k
    L = rsmi.lib()
    blocks, rows, c16, r32 = _coal_ref(k, m, B, T * per, seed=lanes)
    errors = []
    with _Bufs(n, S, [True] * T) as bufs, rsmi.Codec(k, m) as c:
        c.set_option("coalesce_lanes", lanes)
        c.set_option("coalesce_us", 3000)
        c.warm()
        c0, b0 = c.stat("coalesced_calls"), c.stat("coalesced_batches")

        def work(t):
            for j in range(per):
                i = t * per + j
                want = _wants_mixed(t + j)
                bufs.views[t][:] = 0xA5
                bufs.views[t][:B] = np.frombuffer(blocks[i], dtype=np.uint8)
                o16 = (ctypes.c_uint32 * (n + 1))(*([POISON] * (n + 1)))
                o32 = (ctypes.c_uint32 * (n + 1))(*([POISON] * (n + 1)))
                rc = L.rsmi_encode_block_coalesced_crcs(c._h, bufs.ptrs[t], B, bufs.ptrs[t], o16 if want & 1 else None,
                                                        o32 if want & 2 else None)
                if rc:
                    errors.append(("rc", i, rc))
                    return
                try:
                    _check_request(bufs, t, S, rows[i], c16[i], r32[i], want, o16, o32, (i,))
                except AssertionError as e:
                    errors.append(str(e)[:200])

        th = [threading.Thread(target=work, args=(t,)) for t in range(T)]
        for x in th:
            x.start()
        for x in th:
            x.join()
        assert errors == []
        assert c.stat("coalesced_calls") - c0 == T * per
        assert c.stat("coalesced_batches") - b0 < T * per


# ---------------------------------------------------------------------------------------------
# Leg 3: many items per wave, both rows passes
# ---------------------------------------------------------------------------------------------

WAVE_SIZES = [1, 1000, 4097, 5121, 8193, 12289, 69633, 73729]
WAVE_NROWS = 7
TILE = 1024        # a wave's tile: 64 lanes x 16 bytes
ITEM_TILES = 32    # 4 groups of 8 tiles


def _ceil(a, b):
    return (a + b - 1) // b


def _layout(S, layout):
    """(offset of the first row from a 16-byte-aligned base, row pitch)"""
    return (0, _ceil(S, 16) * 16 + 16) if layout == "aligned" else (5, S + 3)


def _wave_nblocks(num_cu):
    return _ceil(4 * num_cu + 3, WAVE_NROWS)


def _wave_plan(kind, fold, layout, S, nrows, nb, num_cu, wpc=1):
    """The launchers' own rule (launch_crc32 / launch_crc): tiles per row, items per row, the
    workgroup cap under waves_per_cu and the waves per workgroup.  Returns the number of waves
    and, per wave, the tile counts of the items it runs in order (wave w: items w, w + nw, ...)."""
    aligned = layout == "aligned"
    if kind == 32:
        tpb = _ceil(S + (0 if aligned else 15), TILE)
        nsup = _ceil(_ceil(tpb, 8), 4)
        wpg = 8 if fold else 4  # the matrix-core pass: workgroups of 8 waves
    else:
        tpb = _ceil(S + (15 if fold and not aligned else 0), TILE)
        nsup = _ceil(tpb, ITEM_TILES)
        wpg = 4
    nitems = nb * nrows * nsup
    cap = max(1, num_cu * wpc // wpg)
    nw = min(_ceil(nitems, wpg), cap) * wpg
    seqs = [[min(ITEM_TILES, tpb - ITEM_TILES * (it % nsup)) for it in range(w, nitems, nw)] for w in range(nw)]
    return nsup, seqs


def _assert_waves_run_many_items(kind, fold, layout, S, num_cu):
    nsup, seqs = _wave_plan(kind, fold, layout, S, WAVE_NROWS, _wave_nblocks(num_cu), num_cu)
    assert max(len(s) for s in seqs) >= 3, "no wave runs three items"
    if nsup > 1:
        both = [s for s in seqs if any(a < b for a, b in zip(s, s[1:])) and any(a > b for a, b in zip(s, s[1:]))]
        assert both, "no wave meets a short item then a long one and a long one then a short one"


WAVE_CASES = [(kind, fold, layout, S) for kind in (32, 16) for fold in (1, 0) for layout in ("aligned", "unaligned")
              for S in WAVE_SIZES]


@pytest.mark.parametrize("num_cu", [256, 304])
def test_wave_plan_runs_many_items_per_wave(num_cu):
    """The shapes of leg 3 do what they are chosen for, by the launchers' arithmetic alone: with
    waves_per_cu 1 some wave runs at least three items in sequence, and at the sizes of several
    items per row (32 + 32 + 5 or 9 tiles) some wave meets items of different tile counts in
    both orders."""
    for kind, fold, layout, S in WAVE_CASES:
        _assert_waves_run_many_items(kind, fold, layout, S, num_cu)
    # the tile counts the sizes stand for
    tiles = {S: _wave_plan(32, 0, "aligned", S, WAVE_NROWS, 4, 4)[1][0][:3] for S in WAVE_SIZES}
    assert [tiles[S][0] for S in WAVE_SIZES[:6]] == [1, 1, 5, 6, 9, 13]
    assert tiles[69633] == [32, 32, 5] and tiles[73729] == [32, 32, 9]


@pytest.fixture(scope="module")
def rows_pool():
    """One random byte pool on the host and the device, shared by legs 3 and 4."""
    import torch

    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    nb = _wave_nblocks(num_cu)
    need = max(_layout(S, lay)[0] + nb * WAVE_NROWS * _layout(S, lay)[1] for S in WAVE_SIZES
               for lay in ("aligned", "unaligned")) + 64
    host = torch.randint(0, 256, (need,), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
    dev = host.to("cuda")
    assert dev.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    yield num_cu, nb, host.numpy(), dev
    del dev
    torch.cuda.empty_cache()


_ROWS_REF = {}


def _rows_ref(kind, h, off, pitch, S, nrows, nb):
    """R32 / R16 of every row of the layout, computed once per (kind, layout, S)."""
    key = (kind, off, pitch, S, nrows, nb)
    if key not in _ROWS_REF:
        f = raw32 if kind == 32 else raw16
        ref = np.empty((nb, nrows), dtype=np.int64)
        for b in range(nb):
            for r in range(nrows):
                ref[b, r] = f(h[off + (b * nrows + r) * pitch:][:S].tobytes())
        ref.setflags(write=False)
        _ROWS_REF[key] = ref
    return _ROWS_REF[key]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,fold,layout,S", WAVE_CASES)
def test_rows_dev_many_items_per_wave(rows_pool, kind, fold, layout, S):
    """waves_per_cu 1 and at least four rows per CU: every wave runs several short items in
    sequence, carrying its accumulator, group value and half-group parity from one to the next
    and prefetching the next item's first unit while it folds the current one (the pipelined
    nibble passes), or restarting its per-item state (the matrix-core passes).  Every R32(row)
    equals zlib's and every R16(row) the oracle's; the slot past nrows stays untouched."""
    import torch

    num_cu, nb, h, dev = rows_pool
    _assert_waves_run_many_items(kind, fold, layout, S, num_cu)  # on the device at hand
    nrows = WAVE_NROWS
    off, pitch = _layout(S, layout)
    out = torch.full((nb, nrows + 1), 0xDEAD, dtype=torch.int32, device="cuda")
    with rsmi.Codec(4, 2) as c:
        c.set_option("waves_per_cu", 1)
        c.set_option("crc32_fold" if kind == 32 else "crc16_fold", fold)
        run = c.crc32_rows_dev if kind == 32 else c.crc16_rows_dev
        run(dev.data_ptr() + off, pitch, nrows * pitch, nrows, S, nb, out.data_ptr(), nrows + 1)
        torch.cuda.synchronize()
    got = out.cpu().numpy().astype(np.int64) & M32
    assert (got[:, nrows] == 0xDEAD).all()
    ref = _rows_ref(kind, h, off, pitch, S, nrows, nb)
    bad = np.argwhere(got[:, :nrows] != ref)
    assert bad.size == 0, (len(bad), [(int(b), int(r), hex(got[b, r]), hex(ref[b, r])) for b, r in bad[:8]])


# ---------------------------------------------------------------------------------------------
# Leg 4: one context, many shapes
# ---------------------------------------------------------------------------------------------

REUSE_SIZES = [8197, 5, 8197, 16389, 8192, 24576, 1, 65541, 5, 8197, 8197, 16381, 24581]


@pytest.mark.gpu
def test_one_context_across_shapes(rows_pool):
    """One Codec(10, 4) and one side stream, 26 rows passes queued back to back with no host sync
    until the end, CRC-32 and CRC-16 in turn.  The shard size walks through repeats, sizes equal
    modulo the 8 KiB segment and sizes on either side of it, so the context's cached per-launch
    shift (crc32_shift_S) is hit, missed and refilled; the fold option and the layout change
    between calls.  Each call has its own output, checked against zlib / the oracle."""
    import torch

    _, _, h, dev = rows_pool
    nb, nrows = 3, 4
    calls = []
    for i, S in enumerate(REUSE_SIZES * 2):
        calls.append((32 if i % 2 == 0 else 16, (i // 2) % 2, "aligned" if (i // 3) % 2 else "unaligned", S))
    crc32_sizes = [S for kind, _, _, S in calls if kind == 32]
    assert any(a == b for a, b in zip(crc32_sizes, crc32_sizes[1:]))  # a cache hit
    assert any(a != b and a % 8192 == b % 8192 for a, b in zip(crc32_sizes, crc32_sizes[1:]))
    assert len(calls) >= 24
    outs = [torch.full((nb, nrows + 1), 0xDEAD, dtype=torch.int32, device="cuda") for _ in calls]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with rsmi.Codec(10, 4) as c:
        for (kind, fold, layout, S), out in zip(calls, outs):
            off, pitch = _layout(S, layout)
            c.set_option("crc32_fold" if kind == 32 else "crc16_fold", fold)
            run = c.crc32_rows_dev if kind == 32 else c.crc16_rows_dev
            run(dev.data_ptr() + off, pitch, nrows * pitch, nrows, S, nb, out.data_ptr(), nrows + 1, side.cuda_stream)
        side.synchronize()
    for i, ((kind, fold, layout, S), out) in enumerate(zip(calls, outs)):
        off, pitch = _layout(S, layout)
        got = out.cpu().numpy().astype(np.int64) & M32
        assert (got[:, nrows] == 0xDEAD).all(), i
        ref = _rows_ref(kind, h, off, pitch, S, nrows, nb)
        assert np.array_equal(got[:, :nrows], ref), (i, kind, fold, layout, S)


# ---------------------------------------------------------------------------------------------
# Leg 5: rows long enough for every segment power
# ---------------------------------------------------------------------------------------------

SEG = 8192
Q18 = 1 << 18
BIG_S_MAX = SEG * (Q18 + 4) + 5  # 2 GiB + 32 KiB + 5


def _big_case(q8, item, groups, last=True):
    """A row of S = 8192 q8 + 5 zero bytes with 0x80 (0x40, ...) at offset 1234 of the given
    8 KiB groups of item `item` and 0x01 at the row's last byte.  Returns (S, writes, a): a is
    the number of whole segments the kernel shifts the item's value by, q8 - gl - 1 with gl the
    item's last group (crc32_item_out)."""
    S = SEG * q8 + 5
    writes = [((4 * item + g) * SEG + 1234, 0x80 >> j) for j, g in enumerate(groups)]
    if last:
        writes.append((S - 1, 0x01))
    gl = 4 * item + 3
    assert gl < q8 and S <= BIG_S_MAX
    return S, writes, q8 - gl - 1


def _big_cases():
    """SC[i] = A^(8192 * 2^i) is applied for every set bit i of a = q8 - gl - 1, where gl is the
    last group of a whole item (four groups), so gl = 3 mod 4 and a = q8 mod 4 (mod 4).  Case i
    picks the row length and the item for which a = 2^i exactly: q8 = 2^18 + 1 for i = 0,
    2^18 + 2 for i = 1 and 2^18 + 4 for i >= 2 (the shortest row in which a whole item's shift has
    bit 18 set).  A wrong SC[i] then fails case i and no other case i'."""
    cases = {}
    for i in range(19):
        q8 = Q18 + (1 if i == 0 else 2 if i == 1 else 4)
        S, writes, a = _big_case(q8, (q8 - 4 - (1 << i)) // 4, [i % 4])
        assert a == 1 << i
        cases["i%d" % i] = (S, writes)
    # every power below 2^18 at once: a = 2^18 - 1, the byte in group 1
    S, writes, a = _big_case(Q18 + 3, 0, [1])
    assert a == Q18 - 1
    cases["all_low"] = (S, writes)
    # bit 18 alone from each of the first item's four groups (the A^8192 steps inside an item)
    S, writes, a = _big_case(Q18 + 4, 0, [0, 1, 2, 3])
    assert a == Q18
    cases["item0"] = (S, writes)
    return cases


BIG_CASES = _big_cases()
BIG_RUNS = [(name, fold, 0) for name in BIG_CASES for fold in (1, 0)] + \
           [(name, fold, 5) for name in ("i18", "all_low", "item0", "i7") for fold in (1, 0)]


def test_big_cases_reach_every_segment_power():
    assert sorted(int(n[1:]) for n in BIG_CASES if n[0] == "i" and n[1:].isdigit()) == list(range(19))
    assert max(S for S, _ in BIG_CASES.values()) == BIG_S_MAX < 1 << 32
    assert BIG_CASES["i0"][0] == SEG * (Q18 + 1) + 5


BIG_ROWS = 32  # overlapping rows: see test_rows_dev_segment_powers


@pytest.fixture(scope="module")
def big_zeros():
    import torch

    buf = torch.zeros(BIG_S_MAX + 17 * BIG_ROWS + 64, dtype=torch.uint8, device="cuda")
    out = torch.zeros((BIG_ROWS, 2), dtype=torch.int32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    c = rsmi.Codec(4, 2)
    yield buf, out, c
    c.close()
    del buf
    torch.cuda.empty_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("name,fold,off", BIG_RUNS)
def test_rows_dev_segment_powers(big_zeros, name, fold, off):
    """Rows of zeros past 2 GiB with a few bytes set: a row's R32 is the XOR of
    A^(S - 1 - p)(R32([v])) over its bytes (p, v), by the zlib-built reference, so no host copy
    of a row is needed.  See _big_cases for what each case isolates.  The launch runs 32 rows
    (one per block) of one buffer that start 16 bytes apart (17 from off = 5: the unaligned pass, the
    memory-grid fold with every misalignment): the set bytes lie 16 r bytes earlier in row r, in
    the same item, so the values that go through the segment powers are v, A^-16 v, ...,
    A^-496 v, which span all 32 bits (A's minimal polynomial has degree 32) -- a wrong column
    of SC[i], not only a wrong matrix, fails the case."""
    import torch

    buf, out, c = big_zeros
    S, writes = BIG_CASES[name]
    pitch = 17 if off else 16
    # absolute positions: the case's bytes as row 0 sees them, and the last row's last byte
    writes = [(off + p, v) for p, v in writes] + [(off + (BIG_ROWS - 1) * pitch + S - 1, 0x02)]
    want = []
    for r in range(BIG_ROWS):
        w = 0
        for p, v in writes:
            q = p - off - r * pitch  # the byte's offset in row r
            if 0 <= q < S:
                w ^= shift_ref(raw32(bytes([v])), S - 1 - q)
        want.append(w)
    assert len(set(want)) == BIG_ROWS
    out.fill_(0xDEAD)
    for p, v in writes:
        buf[p] = v
    try:
        c.set_option("crc32_fold", fold)
        # one row per block, the blocks `pitch` bytes apart (rows of one block may not overlap)
        c.crc32_rows_dev(buf.data_ptr() + off, S if off else _ceil(S, 16) * 16, pitch, 1, S, BIG_ROWS, out.data_ptr(), 2)
        torch.cuda.synchronize()
        assert c.last_kernel() == ("rs_crc32_rows_kernel,MFMA" if fold else "rs_crc32_rows_kernel")
        got = out.cpu().numpy().astype(np.int64) & M32
    finally:
        for p, v in writes:
            buf[p] = 0
    assert (got[:, 1] == 0xDEAD).all()
    bad = [(r, hex(int(got[r, 0])), hex(want[r])) for r in range(BIG_ROWS) if got[r, 0] != want[r]]
    assert bad == [], (name, fold, off, bad[:4])
