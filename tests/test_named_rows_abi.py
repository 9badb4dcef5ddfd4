"""rsmi_crc_named_rows_dev and the mixed reconstruct's _crcs forms at the C-ABI boundary, on the CPU:
the symbols are exported and bound at ABI version 5, the header declares them parameter by
parameter, every argument check answers in its stated order before any device access (the pointers
handed in are never dereferenced: they point nowhere), and without a GPU the calls that need one
say so.  rsmi_reconstruct_mixed_batch_host_crcs with nothing to rebuild needs none."""
import ctypes
import os
import re

import numpy as np
import pytest

import rsmi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rsmi.h")
NEW = ("rsmi_crc_named_rows_dev", "rsmi_reconstruct_mixed_batch_dev_crcs", "rsmi_reconstruct_mixed_batch_host_crcs")
P = 0x1000           # a non-null address that is never dereferenced
OK, INVALID, NO_DATA, TOO_FEW, NO_DEVICE = rsmi.OK, rsmi.ErrInvalidArg, rsmi.ErrShardNoData, rsmi.ErrTooFewShards, \
    rsmi.ErrNoDevice

DECLS = {
    "rsmi_crc_named_rows_dev": [
        "rsmi_ctx*", "const uint8_t*", "size_t", "size_t", "const uint8_t*", "size_t", "size_t", "size_t", "size_t",
        "const int32_t*", "int", "uint32_t*", "uint32_t*", "void*"],
    "rsmi_reconstruct_mixed_batch_dev_crcs": [
        "rsmi_ctx*", "uint8_t*", "size_t", "size_t", "size_t", "size_t", "const uint8_t*", "const uint8_t*", "int",
        "int32_t*", "uint32_t*", "uint32_t*", "void*"],
    "rsmi_reconstruct_mixed_batch_host_crcs": [
        "rsmi_ctx*", "uint8_t*", "size_t", "size_t", "size_t", "const uint8_t*", "const uint8_t*", "int", "int32_t*",
        "uint32_t*", "uint32_t*"],
}


def declaration(name):
    """The parameter types of `name` as include/rsmi.h declares it (names dropped)."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, name
    out = []
    for p in m.group(1).split(","):
        p = " ".join(p.split())
        out.append(re.sub(r"\s*\b[A-Za-z_][A-Za-z0-9_]*$", "", p).replace(" *", "*"))
    return out


def test_symbols_exported_bound_and_version_5():
    L = ctypes.CDLL(rsmi.LIB_PATH)
    bound = rsmi.lib()
    for s in NEW:
        assert hasattr(L, s), s
        assert getattr(bound, s).restype is ctypes.c_int and getattr(bound, s).argtypes, s
    assert bound.rsmi_abi_version() == 5
    for meth in ("crc_named_rows_dev", "reconstruct_mixed_batch_dev_crcs", "reconstruct_mixed_batch_host_crcs_ptr"):
        assert callable(getattr(rsmi.Codec, meth)), meth


@pytest.mark.parametrize("name", NEW)
def test_header_declaration(name):
    assert declaration(name) == DECLS[name]
    assert len(getattr(rsmi.lib(), name).argtypes) == len(DECLS[name])


def test_mixed_crcs_share_the_mixed_calls_arguments():
    """The _crcs forms are the mixed calls with the two outputs put in before the stream (dev) or
    appended (host)."""
    dev, host = declaration("rsmi_reconstruct_mixed_batch_dev"), declaration("rsmi_reconstruct_mixed_batch_host")
    assert DECLS["rsmi_reconstruct_mixed_batch_dev_crcs"] == dev[:-1] + ["uint32_t*", "uint32_t*"] + dev[-1:]
    assert DECLS["rsmi_reconstruct_mixed_batch_host_crcs"] == host + ["uint32_t*", "uint32_t*"]


def named(L, h, data=P, drs=64, dbs=1024, parity=P, prs=64, pbs=1024, S=64, nb=1, rows=P, slots=1, o16=P, o32=P):
    return L.rsmi_crc_named_rows_dev(h, data, drs, dbs, parity, prs, pbs, S, nb, rows, slots, o16, o32, None)


def test_named_rows_argument_checks_in_order():
    L = rsmi.lib()
    with rsmi.Codec(4, 2) as c:
        h = c._h
        # rsmi_verify_batch_dev's checks, in its order: NULLs, S == 0, the shard strides
        assert named(L, None) == INVALID
        assert named(L, h, data=None, S=0) == INVALID
        assert named(L, h, parity=None, S=0) == INVALID
        assert named(L, h, S=0, drs=0, rows=None, slots=0, o16=None, o32=None) == NO_DATA
        assert named(L, h, drs=63, rows=None) == INVALID
        assert named(L, h, prs=63) == INVALID
        # then the call's own
        assert named(L, h, rows=None) == INVALID
        for slots in (0, -1, 7, 1 << 30):
            assert named(L, h, slots=slots) == INVALID, slots
        assert named(L, h, o16=None, o32=None) == INVALID
        assert named(L, h, o16=None, o32=None, nb=0) == INVALID
        # a row of 4 GiB or more: only the CRC-32 refuses it
        big = 1 << 32
        assert named(L, h, S=big, drs=big, prs=big, nb=0) == INVALID
        assert named(L, h, S=big, drs=big, prs=big, nb=0, o16=None) == INVALID
        assert named(L, h, S=big, drs=big, prs=big, nb=0, o32=None) == OK
        assert named(L, h, S=big - 1, drs=big, prs=big, nb=0) == OK
        # nblocks == 0 comes last, and needs no device
        for slots in (1, 2, 6):
            assert named(L, h, nb=0, slots=slots) == OK
            assert named(L, h, nb=0, slots=slots, o16=None) == OK
            assert named(L, h, nb=0, slots=slots, o32=None) == OK


def mixed_dev(L, h, shards=P, rs=64, bs=1024, S=64, nb=1, present=P, required=None, status=None, o16=P, o32=P):
    return L.rsmi_reconstruct_mixed_batch_dev_crcs(h, shards, rs, bs, S, nb, present, required, 0, status, o16, o32, None)


def mixed_host(L, h, shards=P, bs=1024, S=64, nb=1, present=P, required=None, status=None, o16=P, o32=P):
    return L.rsmi_reconstruct_mixed_batch_host_crcs(h, shards, bs, S, nb, present, required, 0, status, o16, o32)


def test_mixed_crcs_argument_checks_in_order():
    """The mixed calls' checks, order and statuses; both outputs NULL is one of the NULL checks."""
    L = rsmi.lib()
    k, m = 4, 2
    n = k + m
    with rsmi.Codec(k, m) as c:
        h = c._h
        for call in (mixed_dev, mixed_host):
            assert call(L, None) == INVALID
            assert call(L, h, shards=None, S=0) == INVALID
            assert call(L, h, present=None, S=0) == INVALID
            assert call(L, h, o16=None, o32=None, S=0) == INVALID
            assert call(L, h, S=0) == NO_DATA
            assert call(L, h, nb=0) == OK
            assert call(L, h, nb=0, o16=None) == OK
            assert call(L, h, nb=0, o32=None) == OK
        assert mixed_dev(L, h, rs=63, nb=0) == INVALID
        assert mixed_host(L, h, bs=n * 64 - 1, nb=0) == INVALID
        # the classing of the masks comes before any device access: too few rows without statuses
        few = np.array([[1, 1, 1, 0, 0, 0]], dtype=np.uint8)
        raw = np.full(n, 0x7EA5, dtype=np.uint32)
        assert mixed_dev(L, h, present=few.ctypes.data) == TOO_FEW
        assert mixed_host(L, h, present=few.ctypes.data, o16=raw.ctypes.data, o32=None) == TOO_FEW


def test_host_crcs_with_nothing_to_rebuild_needs_no_device():
    """Nothing wanted is missing (an intact block; a block whose missing rows are not required; a
    block with too few rows, with statuses): the outputs are zeroed, the statuses written, the rows
    untouched, and no device is asked for."""
    L = rsmi.lib()
    k, m, S, nb = 4, 2, 64, 3
    n = k + m
    present = np.ones((nb, n), dtype=np.uint8)
    present[1, [0, 5]] = 0
    present[2, :4] = 0
    required = np.ones((nb, n), dtype=np.uint8)
    required[1, [0, 5]] = 0
    required[2, :] = 0
    required[2, 0] = 1
    shards = np.arange(nb * n * S, dtype=np.uint32).astype(np.uint8)
    before = shards.copy()
    with rsmi.Codec(k, m) as c:
        for want16, want32 in ((True, True), (True, False), (False, True)):
            r16 = np.full(nb * n, 0x7EA5, dtype=np.uint32)
            r32 = np.full(nb * n, 0x7EA5, dtype=np.uint32)
            status = np.full(nb, -7, dtype=np.int32)
            rc = L.rsmi_reconstruct_mixed_batch_host_crcs(
                c._h, shards.ctypes.data, n * S, S, nb, present.ctypes.data, required.ctypes.data, 0,
                status.ctypes.data, r16.ctypes.data if want16 else None, r32.ctypes.data if want32 else None)
            assert rc == OK
            assert status.tolist() == [OK, OK, TOO_FEW]
            assert (r16 == (0 if want16 else 0x7EA5)).all() and (r32 == (0 if want32 else 0x7EA5)).all()
            assert np.array_equal(shards, before)
        got = c.reconstruct_mixed_batch_host_crcs_ptr(shards.ctypes.data, n * S, S, 2, present[:2], required[:2],
                                                      raw16_ptr=r16.ctypes.data)
        assert got == [OK, OK]


@pytest.mark.skipif(rsmi.device_count() != 0, reason="only meaningful on a host without a GPU")
def test_calls_fail_loudly_without_gpu():
    """No CPU path: with work to do every call reports RSMI_ERR_NO_DEVICE, and so does the
    device-resident mixed form with nothing to rebuild (it zeroes device memory on the stream)."""
    L = rsmi.lib()
    k, m, S = 4, 2, 64
    n = k + m
    intact = np.ones((1, n), dtype=np.uint8)
    lost = intact.copy()
    lost[0, 1] = 0
    shards = np.zeros(n * S, dtype=np.uint8)
    raw = np.full(n, 0x7EA5, dtype=np.uint32)
    with rsmi.Codec(k, m) as c:
        assert named(L, c._h) == NO_DEVICE
        assert mixed_dev(L, c._h, present=lost.ctypes.data) == NO_DEVICE
        assert mixed_dev(L, c._h, present=intact.ctypes.data) == NO_DEVICE
        assert mixed_host(L, c._h, shards=shards.ctypes.data, bs=n * S, present=lost.ctypes.data,
                          o16=raw.ctypes.data, o32=None) == NO_DEVICE
        with pytest.raises(rsmi.RsmiError) as e:
            c.crc_named_rows_dev(P, 64, 1024, P, 64, 1024, S, 1, P, 1, d_raw16=P)
        assert e.value.code == NO_DEVICE
