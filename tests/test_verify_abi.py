"""Encoder.Verify at the C-ABI boundary, on the CPU: the three entry points are exported and
bound, argument errors come before any device access, a host without a GPU reports
RSMI_ERR_NO_DEVICE (there is no CPU fallback), and Erasure.verify raises the upstream sentinels
of reedsolomon's Verify (len(shards) != totalShards, then checkShards with nilok = false)."""
import ctypes

import pytest

import rsmi

SYMS = ("rsmi_verify_batch_dev", "rsmi_verify_batch_host", "rsmi_verify")


def test_symbols_exported_and_bound():
    raw = ctypes.CDLL(rsmi.LIB_PATH)
    L = rsmi.lib()
    for s in SYMS:
        assert hasattr(raw, s), s
        f = getattr(L, s)
        assert f.restype is ctypes.c_int and f.argtypes, s
    assert len(L.rsmi_verify_batch_dev.argtypes) == 11
    assert len(L.rsmi_verify_batch_host.argtypes) == 8
    assert len(L.rsmi_verify.argtypes) == 4
    for name in ("verify", "verify_batch_dev", "verify_batch_host_ptr"):
        assert callable(getattr(rsmi.Codec, name)), name
    assert callable(rsmi.Erasure.verify)
    assert L.rsmi_abi_version() == 5  # additive: the version stays


def test_argument_errors_come_before_device_access():
    """NULL -> INVALID_ARG, S == 0 -> SHARD_NO_DATA, a stride below S (or a block stride below the
    block's rows) -> INVALID_ARG; none of them touches the device, so they read the same on a host
    with and without a GPU.  The pointers are never dereferenced by a failing call."""
    L = rsmi.lib()
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf)
    bad = (ctypes.c_uint32 * 16)()
    pb = ctypes.addressof(bad)
    ok = ctypes.c_int(7)
    with rsmi.Codec(4, 2) as c:
        h = c._h
        # device-resident
        assert L.rsmi_verify_batch_dev(None, p, 64, 256, p, 64, 128, 64, 1, pb, None) == rsmi.ErrInvalidArg
        assert L.rsmi_verify_batch_dev(h, None, 64, 256, p, 64, 128, 64, 1, pb, None) == rsmi.ErrInvalidArg
        assert L.rsmi_verify_batch_dev(h, p, 64, 256, None, 64, 128, 64, 1, pb, None) == rsmi.ErrInvalidArg
        assert L.rsmi_verify_batch_dev(h, p, 64, 256, p, 64, 128, 64, 1, None, None) == rsmi.ErrInvalidArg
        assert L.rsmi_verify_batch_dev(h, p, 64, 256, p, 64, 128, 0, 1, pb, None) == rsmi.ErrShardNoData
        assert L.rsmi_verify_batch_dev(h, p, 63, 256, p, 64, 128, 64, 1, pb, None) == rsmi.ErrInvalidArg
        assert L.rsmi_verify_batch_dev(h, p, 64, 256, p, 63, 128, 64, 1, pb, None) == rsmi.ErrInvalidArg
        assert L.rsmi_verify_batch_dev(h, p, 64, 256, p, 64, 128, 64, 0, pb, None) == rsmi.OK
        assert L.rsmi_verify_batch_dev(h, p, 64, 256, p, 63, 128, 64, 0, pb, None) == rsmi.ErrInvalidArg
        # host batch
        assert L.rsmi_verify_batch_host(None, p, 256, p, 128, 64, 1, pb) == rsmi.ErrInvalidArg
        assert L.rsmi_verify_batch_host(h, None, 256, p, 128, 64, 1, pb) == rsmi.ErrInvalidArg
        assert L.rsmi_verify_batch_host(h, p, 256, None, 128, 64, 1, pb) == rsmi.ErrInvalidArg
        assert L.rsmi_verify_batch_host(h, p, 256, p, 128, 64, 1, None) == rsmi.ErrInvalidArg
        assert L.rsmi_verify_batch_host(h, p, 256, p, 128, 0, 1, pb) == rsmi.ErrShardNoData
        assert L.rsmi_verify_batch_host(h, p, 255, p, 128, 64, 1, pb) == rsmi.ErrInvalidArg
        assert L.rsmi_verify_batch_host(h, p, 256, p, 127, 64, 1, pb) == rsmi.ErrInvalidArg
        # nblocks == 0 validates and returns OK without a device
        assert L.rsmi_verify_batch_host(h, p, 256, p, 128, 64, 0, pb) == rsmi.OK
        assert L.rsmi_verify_batch_host(h, p, 255, p, 128, 64, 0, pb) == rsmi.ErrInvalidArg
        # one block
        assert L.rsmi_verify(None, p, 64, ctypes.byref(ok)) == rsmi.ErrInvalidArg
        assert L.rsmi_verify(h, None, 64, ctypes.byref(ok)) == rsmi.ErrInvalidArg
        assert L.rsmi_verify(h, p, 64, None) == rsmi.ErrInvalidArg
        assert L.rsmi_verify(h, p, 0, ctypes.byref(ok)) == rsmi.ErrShardNoData
        assert ok.value == 7 and not any(bad)  # a failing call writes no result


@pytest.mark.skipif(rsmi.device_count() != 0, reason="only meaningful on a host without a GPU")
def test_verify_fails_loudly_without_gpu():
    """No CPU fallback: valid arguments on a host without a GPU give RSMI_ERR_NO_DEVICE."""
    L = rsmi.lib()
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf)
    bad = (ctypes.c_uint32 * 16)()
    pb = ctypes.addressof(bad)
    ok = ctypes.c_int(7)
    with rsmi.Codec(4, 2) as c:
        assert L.rsmi_verify_batch_dev(c._h, p, 64, 256, p, 64, 128, 64, 1, pb, None) == rsmi.ErrNoDevice
        assert L.rsmi_verify_batch_host(c._h, p, 256, p, 128, 64, 1, pb) == rsmi.ErrNoDevice
        assert L.rsmi_verify(c._h, p, 64, ctypes.byref(ok)) == rsmi.ErrNoDevice
        with pytest.raises(rsmi.RsmiError) as e:
            c.verify(bytearray(6 * 64), 64)
        assert e.value.code == rsmi.ErrNoDevice
    assert ok.value == 7


def test_erasure_verify_raises_upstream_sentinels():
    """reedsolomon Verify: a list of the wrong length is ErrTooFewShards; then checkShards with
    nilok = false: every shard empty is ErrShardNoData, a missing or unequal one ErrShardSize.
    All of it is decided on the host, before a codec is opened."""
    e = rsmi.NewErasure(4, 2, 64)
    good = [bytes(16)] * 6

    def code(shards):
        with pytest.raises(rsmi.RsmiError) as ex:
            e.verify(shards)
        return ex.value.code

    assert code(good[:5]) == rsmi.ErrTooFewShards
    assert code([]) == rsmi.ErrTooFewShards
    assert code(good + [bytes(16)]) == rsmi.ErrTooFewShards
    assert code([b""] * 6) == rsmi.ErrShardNoData
    assert code(good[:5] + [bytes(15)]) == rsmi.ErrShardSize
    assert code([bytes(17)] + good[1:]) == rsmi.ErrShardSize
    assert code(good[:2] + [b""] + good[3:]) == rsmi.ErrShardSize  # a missing shard: nilok = false
    assert e._codec is None
