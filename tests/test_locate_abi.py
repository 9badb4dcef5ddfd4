"""rsmi_locate at the C-ABI boundary, on the CPU: the four entry points are exported and bound,
argument errors come before any device access and write no result, a host without a GPU reports
RSMI_ERR_NO_DEVICE (there is no CPU fallback), Erasure.locate raises the upstream sentinels that
Erasure.verify raises, and rsmi_locate_matrix (host-only) is the ratio matrix
R[j][c] = M[k+j][c] / M[k][c] of the oracle's encode matrix."""
import ctypes

import numpy as np
import pytest

import oracle_lib as orc
import rsmi

SYMS = ("rsmi_locate_batch_dev", "rsmi_locate_batch_host", "rsmi_locate", "rsmi_locate_matrix")


def test_symbols_exported_and_bound():
    raw = ctypes.CDLL(rsmi.LIB_PATH)
    L = rsmi.lib()
    for s in SYMS:
        assert hasattr(raw, s), s
        f = getattr(L, s)
        assert f.restype is ctypes.c_int and f.argtypes, s
    assert len(L.rsmi_locate_batch_dev.argtypes) == 12
    assert len(L.rsmi_locate_batch_host.argtypes) == 9
    assert len(L.rsmi_locate.argtypes) == 4
    assert len(L.rsmi_locate_matrix.argtypes) == 2
    for name in ("locate", "locate_batch_dev", "locate_batch_host_ptr", "locate_matrix"):
        assert callable(getattr(rsmi.Codec, name)), name
    assert callable(rsmi.Erasure.locate)
    assert rsmi.LocateClean == -1 and rsmi.LocateUnknown == -2
    assert L.rsmi_abi_version() == 5  # additive: the version stays


def test_argument_errors_come_before_device_access():
    """NULL -> INVALID_ARG (the flags pointer alone may be NULL), S == 0 -> SHARD_NO_DATA, a stride
    below S (or a block stride below the block's rows) -> INVALID_ARG; none of them touches the
    device, so they read the same on a host with and without a GPU.  The pointers are never
    dereferenced by a failing call."""
    L = rsmi.lib()
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf)
    bad = (ctypes.c_uint32 * 16)()
    pb = ctypes.addressof(bad)
    cul = (ctypes.c_int32 * 8)(*([7] * 8))
    pc = ctypes.addressof(cul)
    one = ctypes.c_int(7)
    mat = (ctypes.c_uint8 * 8)()
    with rsmi.Codec(4, 2) as c:
        h = c._h
        # device-resident
        assert L.rsmi_locate_batch_dev(None, p, 64, 256, p, 64, 128, 64, 1, pc, pb, None) == rsmi.ErrInvalidArg
        assert L.rsmi_locate_batch_dev(h, None, 64, 256, p, 64, 128, 64, 1, pc, pb, None) == rsmi.ErrInvalidArg
        assert L.rsmi_locate_batch_dev(h, p, 64, 256, None, 64, 128, 64, 1, pc, pb, None) == rsmi.ErrInvalidArg
        assert L.rsmi_locate_batch_dev(h, p, 64, 256, p, 64, 128, 64, 1, None, pb, None) == rsmi.ErrInvalidArg
        assert L.rsmi_locate_batch_dev(h, p, 64, 256, p, 64, 128, 64, 1, None, None, None) == rsmi.ErrInvalidArg
        assert L.rsmi_locate_batch_dev(h, p, 64, 256, p, 64, 128, 0, 1, pc, pb, None) == rsmi.ErrShardNoData
        assert L.rsmi_locate_batch_dev(h, p, 63, 256, p, 64, 128, 64, 1, pc, pb, None) == rsmi.ErrInvalidArg
        assert L.rsmi_locate_batch_dev(h, p, 64, 256, p, 63, 128, 64, 1, pc, None, None) == rsmi.ErrInvalidArg
        assert L.rsmi_locate_batch_dev(h, p, 64, 256, p, 64, 128, 64, 0, pc, pb, None) == rsmi.OK
        assert L.rsmi_locate_batch_dev(h, p, 64, 256, p, 64, 128, 64, 0, pc, None, None) == rsmi.OK
        assert L.rsmi_locate_batch_dev(h, p, 64, 256, p, 63, 128, 64, 0, pc, pb, None) == rsmi.ErrInvalidArg
        # host batch
        assert L.rsmi_locate_batch_host(None, p, 256, p, 128, 64, 1, pc, pb) == rsmi.ErrInvalidArg
        assert L.rsmi_locate_batch_host(h, None, 256, p, 128, 64, 1, pc, pb) == rsmi.ErrInvalidArg
        assert L.rsmi_locate_batch_host(h, p, 256, None, 128, 64, 1, pc, pb) == rsmi.ErrInvalidArg
        assert L.rsmi_locate_batch_host(h, p, 256, p, 128, 64, 1, None, pb) == rsmi.ErrInvalidArg
        assert L.rsmi_locate_batch_host(h, p, 256, p, 128, 0, 1, pc, pb) == rsmi.ErrShardNoData
        assert L.rsmi_locate_batch_host(h, p, 255, p, 128, 64, 1, pc, pb) == rsmi.ErrInvalidArg
        assert L.rsmi_locate_batch_host(h, p, 256, p, 127, 64, 1, pc, None) == rsmi.ErrInvalidArg
        # nblocks == 0 validates and returns OK without a device
        assert L.rsmi_locate_batch_host(h, p, 256, p, 128, 64, 0, pc, pb) == rsmi.OK
        assert L.rsmi_locate_batch_host(h, p, 256, p, 128, 64, 0, pc, None) == rsmi.OK
        assert L.rsmi_locate_batch_host(h, p, 255, p, 128, 64, 0, pc, pb) == rsmi.ErrInvalidArg
        # one block
        assert L.rsmi_locate(None, p, 64, ctypes.byref(one)) == rsmi.ErrInvalidArg
        assert L.rsmi_locate(h, None, 64, ctypes.byref(one)) == rsmi.ErrInvalidArg
        assert L.rsmi_locate(h, p, 64, None) == rsmi.ErrInvalidArg
        assert L.rsmi_locate(h, p, 0, ctypes.byref(one)) == rsmi.ErrShardNoData
        # the matrix
        assert L.rsmi_locate_matrix(None, ctypes.addressof(mat)) == rsmi.ErrInvalidArg
        assert L.rsmi_locate_matrix(h, None) == rsmi.ErrInvalidArg
    assert one.value == 7 and not any(bad) and list(cul) == [7] * 8  # a failing call writes no result


@pytest.mark.skipif(rsmi.device_count() != 0, reason="only meaningful on a host without a GPU")
def test_locate_fails_loudly_without_gpu():
    """No CPU fallback: valid arguments on a host without a GPU give RSMI_ERR_NO_DEVICE and write
    no result; the matrix needs no device."""
    L = rsmi.lib()
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf)
    bad = (ctypes.c_uint32 * 16)()
    pb = ctypes.addressof(bad)
    cul = (ctypes.c_int32 * 8)(*([7] * 8))
    pc = ctypes.addressof(cul)
    one = ctypes.c_int(7)
    with rsmi.Codec(4, 2) as c:
        assert L.rsmi_locate_batch_dev(c._h, p, 64, 256, p, 64, 128, 64, 1, pc, pb, None) == rsmi.ErrNoDevice
        assert L.rsmi_locate_batch_dev(c._h, p, 64, 256, p, 64, 128, 64, 1, pc, None, None) == rsmi.ErrNoDevice
        assert L.rsmi_locate_batch_host(c._h, p, 256, p, 128, 64, 1, pc, pb) == rsmi.ErrNoDevice
        assert L.rsmi_locate(c._h, p, 64, ctypes.byref(one)) == rsmi.ErrNoDevice
        with pytest.raises(rsmi.RsmiError) as e:
            c.locate(bytearray(6 * 64), 64)
        assert e.value.code == rsmi.ErrNoDevice
        assert len(c.locate_matrix()) == 8
    assert one.value == 7 and not any(bad) and list(cul) == [7] * 8


def test_erasure_locate_raises_upstream_sentinels():
    """The checks of Erasure.verify (reedsolomon Verify: the list's length, then checkShards with
    nilok = false), decided on the host before a codec is opened."""
    e = rsmi.NewErasure(4, 2, 64)
    good = [bytes(16)] * 6

    def code(shards):
        with pytest.raises(rsmi.RsmiError) as ex:
            e.locate(shards)
        return ex.value.code

    assert code(good[:5]) == rsmi.ErrTooFewShards
    assert code([]) == rsmi.ErrTooFewShards
    assert code(good + [bytes(16)]) == rsmi.ErrTooFewShards
    assert code([b""] * 6) == rsmi.ErrShardNoData
    assert code(good[:5] + [bytes(15)]) == rsmi.ErrShardSize
    assert code([bytes(17)] + good[1:]) == rsmi.ErrShardSize
    assert code(good[:2] + [b""] + good[3:]) == rsmi.ErrShardSize  # a missing shard: nilok = false
    assert e._codec is None


@pytest.mark.parametrize("k,m", [(2, 2), (4, 2), (10, 4), (16, 4), (5, 5), (17, 3)])
def test_locate_matrix_is_the_ratio_matrix(k, m):
    """Row 0 is all ones, R[j][c] * M[k][c] == M[k+j][c] with the oracle's matrix and multiply, and
    the ratios of row 1 are pairwise distinct (what lets two syndromes tell the data shards apart).
    No device is touched."""
    M = orc.build_matrix(k, m)
    mul = orc.lib().rs_oracle_gal_mul
    with rsmi.Codec(k, m) as c:
        R = np.frombuffer(c.locate_matrix(), dtype=np.uint8).reshape(m, k)
        assert np.array_equal(np.frombuffer(c.encode_matrix(), dtype=np.uint8).reshape(k + m, k), M)
    assert (M[k:] != 0).all()
    assert (R[0] == 1).all()
    for j in range(m):
        for col in range(k):
            assert mul(int(R[j, col]), int(M[k, col])) == M[k + j, col], (j, col)
    assert len(set(R[1].tolist())) == k
