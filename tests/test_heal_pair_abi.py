"""rsmi_heal_pair at the C-ABI boundary, on the CPU: the four entry points are exported and bound,
argument errors come before any device access and write no result (the checks and their order are
those of test_locate_pair_abi.py), a host without a GPU reports RSMI_ERR_NO_DEVICE,
rsmi_heal_pair_matrix (host-only) gives, for every pair, a 2 x m matrix D with D [h_x h_y] = I_2
and at most two non-zero columns, and the instantiated heal pair kernels are those of the source."""
import ctypes
import os
import re

import numpy as np
import pytest

import rsmi
from test_locate_matrix import CSRC
from test_locate_pair import PAIR_KS, all_pairs, check_matrix, gf_tables

SYMS = ("rsmi_heal_pair_batch_dev", "rsmi_heal_pair_batch_host", "rsmi_heal_pair", "rsmi_heal_pair_matrix")


def test_symbols_exported_and_bound():
    raw = ctypes.CDLL(rsmi.LIB_PATH)
    L = rsmi.lib()
    for s in SYMS:
        assert hasattr(raw, s), s
        f = getattr(L, s)
        assert f.restype is ctypes.c_int and f.argtypes, s
    assert len(L.rsmi_heal_pair_batch_dev.argtypes) == 12
    assert len(L.rsmi_heal_pair_batch_host.argtypes) == 9
    assert len(L.rsmi_heal_pair.argtypes) == 4
    assert len(L.rsmi_heal_pair_matrix.argtypes) == 4
    for name in ("heal_pair", "heal_pair_batch_dev", "heal_pair_batch_host_ptr", "heal_pair_matrix"):
        assert callable(getattr(rsmi.Codec, name)), name
    assert callable(rsmi.Erasure.heal_pair)
    assert L.rsmi_abi_version() == 5  # additive: the version stays


def test_argument_errors_come_before_device_access():
    """The checks of rsmi_locate_pair_*, in their order: NULL -> INVALID_ARG (the flags pointer alone
    may be NULL), S == 0 -> SHARD_NO_DATA, a stride below S (or a block stride below the block's
    rows) -> INVALID_ARG, nblocks == 0 -> OK; none of them touches the device, writes a result or
    writes a shard byte."""
    L = rsmi.lib()
    buf = (ctypes.c_uint8 * 4096)(*([0x5A] * 4096))
    p = ctypes.addressof(buf)
    bad = (ctypes.c_uint32 * 16)()
    pb = ctypes.addressof(bad)
    out = (ctypes.c_int32 * 8)(*([7] * 8))
    po = ctypes.addressof(out)
    one = (ctypes.c_int * 2)(7, 7)
    mat = (ctypes.c_uint8 * 12)(*([9] * 12))
    pm = ctypes.addressof(mat)
    with rsmi.Codec(4, 2) as c:
        h = c._h
        dev, host, single = L.rsmi_heal_pair_batch_dev, L.rsmi_heal_pair_batch_host, L.rsmi_heal_pair
        assert dev(None, p, 64, 256, p, 64, 128, 64, 1, po, pb, None) == rsmi.ErrInvalidArg
        assert dev(h, None, 64, 256, p, 64, 128, 64, 1, po, pb, None) == rsmi.ErrInvalidArg
        assert dev(h, p, 64, 256, None, 64, 128, 64, 1, po, pb, None) == rsmi.ErrInvalidArg
        assert dev(h, p, 64, 256, p, 64, 128, 64, 1, None, pb, None) == rsmi.ErrInvalidArg
        assert dev(h, p, 64, 256, p, 64, 128, 64, 1, None, None, None) == rsmi.ErrInvalidArg
        assert dev(h, p, 64, 256, p, 64, 128, 0, 1, po, pb, None) == rsmi.ErrShardNoData
        assert dev(h, None, 64, 256, p, 64, 128, 0, 1, po, pb, None) == rsmi.ErrInvalidArg  # NULL before S
        assert dev(h, p, 63, 256, p, 64, 128, 64, 1, po, pb, None) == rsmi.ErrInvalidArg
        assert dev(h, p, 64, 256, p, 63, 128, 64, 1, po, None, None) == rsmi.ErrInvalidArg
        assert dev(h, p, 63, 256, p, 64, 128, 0, 1, po, pb, None) == rsmi.ErrShardNoData  # S before the strides
        assert dev(h, p, 64, 256, p, 64, 128, 64, 0, po, pb, None) == rsmi.OK
        assert dev(h, p, 64, 256, p, 64, 128, 64, 0, po, None, None) == rsmi.OK
        assert dev(h, p, 64, 256, p, 63, 128, 64, 0, po, pb, None) == rsmi.ErrInvalidArg
        assert host(None, p, 256, p, 128, 64, 1, po, pb) == rsmi.ErrInvalidArg
        assert host(h, None, 256, p, 128, 64, 1, po, pb) == rsmi.ErrInvalidArg
        assert host(h, p, 256, None, 128, 64, 1, po, pb) == rsmi.ErrInvalidArg
        assert host(h, p, 256, p, 128, 64, 1, None, pb) == rsmi.ErrInvalidArg
        assert host(h, p, 256, p, 128, 0, 1, po, pb) == rsmi.ErrShardNoData
        assert host(h, p, 255, p, 128, 64, 1, po, pb) == rsmi.ErrInvalidArg
        assert host(h, p, 256, p, 127, 64, 1, po, None) == rsmi.ErrInvalidArg
        assert host(h, p, 256, p, 128, 64, 0, po, pb) == rsmi.OK
        assert host(h, p, 256, p, 128, 64, 0, po, None) == rsmi.OK
        assert host(h, p, 255, p, 128, 64, 0, po, pb) == rsmi.ErrInvalidArg
        assert single(None, p, 64, one) == rsmi.ErrInvalidArg
        assert single(h, None, 64, one) == rsmi.ErrInvalidArg
        assert single(h, p, 64, None) == rsmi.ErrInvalidArg
        assert single(h, p, 0, one) == rsmi.ErrShardNoData
        with pytest.raises(TypeError):
            c.heal_pair(bytes(6 * 64), 64)  # the call rewrites its argument
        # the matrix: NULL, x == y, an index outside [0, n); m = 2 has one
        assert L.rsmi_heal_pair_matrix(None, 0, 1, pm) == rsmi.ErrInvalidArg
        assert L.rsmi_heal_pair_matrix(h, 0, 1, None) == rsmi.ErrInvalidArg
        for x, y in ((2, 2), (-1, 3), (3, -1), (0, 6), (6, 0), (6, 6)):
            assert L.rsmi_heal_pair_matrix(h, x, y, pm) == rsmi.ErrInvalidArg, (x, y)
        assert list(mat) == [9] * 12
        assert L.rsmi_heal_pair_matrix(h, 0, 5, pm) == rsmi.OK
        assert bytes(mat)[:4] == c.heal_pair_matrix(0, 5) and list(mat)[4:] == [9] * 8
    with rsmi.Codec(4, 1) as c:  # m = 1: no pair has a D
        for x, y in ((0, 1), (0, 4), (4, 0)):
            assert L.rsmi_heal_pair_matrix(c._h, x, y, pm) == rsmi.ErrInvalidArg, (x, y)
        assert list(mat)[4:] == [9] * 8
    assert list(one) == [7, 7] and not any(bad) and list(out) == [7] * 8
    assert bytes(buf) == bytes([0x5A] * 4096)


@pytest.mark.skipif(rsmi.device_count() != 0, reason="only meaningful on a host without a GPU")
def test_heal_pair_fails_loudly_without_gpu():
    """No CPU fallback: valid arguments on a host without a GPU give RSMI_ERR_NO_DEVICE, write no
    result and no shard byte; the matrix needs no device."""
    L = rsmi.lib()
    buf = (ctypes.c_uint8 * 4096)(*([0x5A] * 4096))
    p = ctypes.addressof(buf)
    bad = (ctypes.c_uint32 * 16)()
    pb = ctypes.addressof(bad)
    out = (ctypes.c_int32 * 8)(*([7] * 8))
    po = ctypes.addressof(out)
    one = (ctypes.c_int * 2)(7, 7)
    for k, m in ((4, 2), (4, 3)):
        with rsmi.Codec(k, m) as c:
            rs, n = 64, k + m
            assert L.rsmi_heal_pair_batch_dev(c._h, p, rs, n * rs, p, rs, n * rs, 64, 1, po, pb, None) == rsmi.ErrNoDevice
            assert L.rsmi_heal_pair_batch_dev(c._h, p, rs, n * rs, p, rs, n * rs, 64, 1, po, None, None) == rsmi.ErrNoDevice
            assert L.rsmi_heal_pair_batch_host(c._h, p, k * 64, p, m * 64, 64, 1, po, pb) == rsmi.ErrNoDevice
            assert L.rsmi_heal_pair(c._h, p, 64, one) == rsmi.ErrNoDevice
            with pytest.raises(rsmi.RsmiError) as e:
                c.heal_pair(bytearray(n * 64), 64)
            assert e.value.code == rsmi.ErrNoDevice
            assert len(c.heal_pair_matrix(0, 1)) == 2 * m
    assert list(one) == [7, 7] and not any(bad) and list(out) == [7] * 8
    assert bytes(buf) == bytes([0x5A] * 4096)


def test_erasure_heal_pair_raises_upstream_sentinels():
    """The checks of Erasure.heal, decided on the host before a codec is opened."""
    e = rsmi.NewErasure(4, 3, 64)
    good = [bytes(16)] * 7

    def code(shards):
        with pytest.raises(rsmi.RsmiError) as ex:
            e.heal_pair(shards)
        return ex.value.code

    assert code(good[:6]) == rsmi.ErrTooFewShards
    assert code(good + [bytes(16)]) == rsmi.ErrTooFewShards
    assert code([b""] * 7) == rsmi.ErrShardNoData
    assert code(good[:6] + [bytes(15)]) == rsmi.ErrShardSize
    assert code(good[:2] + [b""] + good[3:]) == rsmi.ErrShardSize
    assert e._codec is None


def encode_check_matrix(c):
    """H = [M | I_m] with M the parity rows of the library's own rsmi_encode_matrix."""
    k, m = c.k, c.m
    E = np.frombuffer(c.encode_matrix(), dtype=np.uint8).reshape(k + m, k)
    assert np.array_equal(E[:k], np.eye(k, dtype=np.uint8))
    return np.concatenate([E[k:], np.eye(m, dtype=np.uint8)], axis=1)


@pytest.mark.parametrize("k,m", [(10, 4), (6, 3), (16, 4), (4, 4), (20, 5)])
def test_matrix_inverts_exactly_the_pair(k, m):
    """For every pair, in both orders: D h_x = (1, 0), D h_y = (0, 1) with the oracle's multiply, and
    at most two non-zero columns, which are those the header names for the pair's kind.  H is built
    from rsmi_encode_matrix and equals the oracle's.  No device is touched."""
    MUL, _ = gf_tables()
    n = k + m
    with rsmi.Codec(k, m) as c:
        H = encode_check_matrix(c)
        assert np.array_equal(H, check_matrix(k, m))
        for x, y in all_pairs(n):
            D = np.frombuffer(c.heal_pair_matrix(x, y), dtype=np.uint8).reshape(2, m)
            DH = np.bitwise_xor.reduce(MUL[D[:, :, None], H[None, :, [x, y]]], axis=1)  # (2, 2)
            assert DH.tolist() == [[1, 0], [0, 1]], (x, y, DH.tolist())
            cols = np.flatnonzero(D.any(axis=0)).tolist()
            if x >= k:
                assert cols == [x - k, y - k] and D[:, cols].tolist() == [[1, 0], [0, 1]], (x, y)
            elif y >= k:
                assert cols == sorted([y - k, 1 if y == k else 0]), (x, y, cols)
            else:
                assert cols == [0, 1], (x, y, cols)
            swapped = np.frombuffer(c.heal_pair_matrix(y, x), dtype=np.uint8).reshape(2, m)
            assert np.array_equal(swapped, D[::-1]), (x, y)


def test_matrix_at_m2():
    """m = 2: no pair is ever named, but every pair has its D (H is 2 x n, any two columns a basis)."""
    MUL, _ = gf_tables()
    k, m = 4, 2
    with rsmi.Codec(k, m) as c:
        H = encode_check_matrix(c)
        for x, y in all_pairs(k + m):
            D = np.frombuffer(c.heal_pair_matrix(x, y), dtype=np.uint8).reshape(2, m)
            DH = np.bitwise_xor.reduce(MUL[D[:, :, None], H[None, :, [x, y]]], axis=1)
            assert DH.tolist() == [[1, 0], [0, 1]], (x, y)


def test_heal_pair_kernel_table_matches_source():
    """The instantiated (K, MT) set read from rs_heal_pair_kernels.hip equals the pair kernels' K with
    MT in {3, 4}: 40 kernels with both layouts, and both new sources are in the Makefile's lists."""
    with open(os.path.join(CSRC, "rs_heal_pair_kernels.hip")) as f:
        src = f.read()
    assert [int(x) for x in re.findall(r"\bfill_heal_pair_k<\s*(\d+)\s*>\s*\(", src)] == PAIR_KS
    assert re.findall(r"\bfill_heal_pair_km<K,\s*(\d+)>\(", src) == ["3", "4"]
    assert len(re.findall(r"&rs_heal_pair_kernel<", src)) == 2
    assert re.search(r"t\.fn\[K\]\[MT\] = reinterpret_cast<void\*>\(&rs_heal_pair_kernel<K, MT, false>\);", src)
    assert re.search(r"t\.ua\[K\]\[MT\] = reinterpret_cast<void\*>\(&rs_heal_pair_kernel<K, MT, true>\);", src)
    assert 2 * 2 * len(PAIR_KS) == 40
    with open(os.path.join(CSRC, "..", "Makefile")) as f:
        mk = f.read()
    assert "csrc/rs_heal_pair_kernels.hip" in mk and "csrc/rsmi_heal_pair.cpp" in mk
