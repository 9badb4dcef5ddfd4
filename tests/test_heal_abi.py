"""rsmi_heal at the C-ABI boundary, on the CPU: the three entry points are exported and bound, the
ABI version stays 5, argument errors come before any device access with the statuses rsmi_locate
gives for the same arguments and write nothing, a host without a GPU reports RSMI_ERR_NO_DEVICE
(there is no CPU fallback) and leaves the shards alone, and Erasure.heal raises the upstream
sentinels that Erasure.locate raises."""
import ctypes

import pytest

import rsmi

SYMS = ("rsmi_heal_batch_dev", "rsmi_heal_batch_host", "rsmi_heal")


def test_symbols_exported_and_bound():
    raw = ctypes.CDLL(rsmi.LIB_PATH)
    L = rsmi.lib()
    for s in SYMS:
        assert hasattr(raw, s), s
        f = getattr(L, s)
        assert f.restype is ctypes.c_int and f.argtypes, s
        # heal takes locate's arguments
        assert len(f.argtypes) == len(getattr(L, s.replace("heal", "locate")).argtypes), s
    assert len(L.rsmi_heal_batch_dev.argtypes) == 12
    assert len(L.rsmi_heal_batch_host.argtypes) == 9
    assert len(L.rsmi_heal.argtypes) == 4
    for name in ("heal", "heal_batch_dev", "heal_batch_host_ptr"):
        assert callable(getattr(rsmi.Codec, name)), name
    assert callable(rsmi.Erasure.heal)
    assert L.rsmi_abi_version() == 5  # additive: the version stays


def _dev_cases(p, pc, pb):
    """(arguments after the context, locate's documented status) of the device-resident call."""
    return [((None, 64, 256, p, 64, 128, 64, 1, pc, pb, None), rsmi.ErrInvalidArg),
            ((p, 64, 256, None, 64, 128, 64, 1, pc, pb, None), rsmi.ErrInvalidArg),
            ((p, 64, 256, p, 64, 128, 64, 1, None, pb, None), rsmi.ErrInvalidArg),
            ((p, 64, 256, p, 64, 128, 64, 1, None, None, None), rsmi.ErrInvalidArg),
            ((p, 64, 256, p, 64, 128, 0, 1, pc, pb, None), rsmi.ErrShardNoData),
            ((p, 63, 256, p, 64, 128, 64, 1, pc, pb, None), rsmi.ErrInvalidArg),
            ((p, 64, 256, p, 63, 128, 64, 1, pc, None, None), rsmi.ErrInvalidArg),
            ((p, 64, 256, p, 64, 128, 64, 0, pc, pb, None), rsmi.OK),
            ((p, 64, 256, p, 64, 128, 64, 0, pc, None, None), rsmi.OK),
            ((p, 64, 256, p, 63, 128, 64, 0, pc, pb, None), rsmi.ErrInvalidArg)]


def _host_cases(p, pc, pb):
    return [((None, 256, p, 128, 64, 1, pc, pb), rsmi.ErrInvalidArg),
            ((p, 256, None, 128, 64, 1, pc, pb), rsmi.ErrInvalidArg),
            ((p, 256, p, 128, 64, 1, None, pb), rsmi.ErrInvalidArg),
            ((p, 256, p, 128, 0, 1, pc, pb), rsmi.ErrShardNoData),
            ((p, 255, p, 128, 64, 1, pc, pb), rsmi.ErrInvalidArg),
            ((p, 256, p, 127, 64, 1, pc, None), rsmi.ErrInvalidArg),
            ((p, 256, p, 128, 64, 0, pc, pb), rsmi.OK),   # nblocks == 0 validates and needs no device
            ((p, 256, p, 128, 64, 0, pc, None), rsmi.OK),
            ((p, 255, p, 128, 64, 0, pc, pb), rsmi.ErrInvalidArg)]


def test_argument_errors_are_locates_and_come_before_device_access():
    """NULL -> INVALID_ARG (the flags pointer alone may be NULL), S == 0 -> SHARD_NO_DATA, a stride
    below S (or a block stride below the block's rows) -> INVALID_ARG, nblocks == 0 -> OK: the
    status is stated here and is also what rsmi_locate returns for the same arguments.  None of the
    calls touches the device or dereferences a pointer: the shards and the outputs stay as they
    were."""
    L = rsmi.lib()
    buf = (ctypes.c_uint8 * 4096)(*([0xA5] * 4096))
    p = ctypes.addressof(buf)
    bad = (ctypes.c_uint32 * 16)()
    pb = ctypes.addressof(bad)
    cul = (ctypes.c_int32 * 8)(*([7] * 8))
    pc = ctypes.addressof(cul)
    one = ctypes.c_int(7)
    with rsmi.Codec(4, 2) as c:
        h = c._h
        assert L.rsmi_heal_batch_dev(None, p, 64, 256, p, 64, 128, 64, 1, pc, pb, None) == rsmi.ErrInvalidArg
        for args, want in _dev_cases(p, pc, pb):
            assert L.rsmi_heal_batch_dev(h, *args) == want, args
            assert L.rsmi_locate_batch_dev(h, *args) == want, args
        assert L.rsmi_heal_batch_host(None, p, 256, p, 128, 64, 1, pc, pb) == rsmi.ErrInvalidArg
        for args, want in _host_cases(p, pc, pb):
            assert L.rsmi_heal_batch_host(h, *args) == want, args
            assert L.rsmi_locate_batch_host(h, *args) == want, args
        for args, want in (((None, p, 64, ctypes.byref(one)), rsmi.ErrInvalidArg),
                           ((h, None, 64, ctypes.byref(one)), rsmi.ErrInvalidArg),
                           ((h, p, 64, None), rsmi.ErrInvalidArg),
                           ((h, p, 0, ctypes.byref(one)), rsmi.ErrShardNoData)):
            assert L.rsmi_heal(*args) == want
            assert L.rsmi_locate(*args) == want
        with pytest.raises(TypeError):
            c.heal(bytes(6 * 64), 64)  # heal rewrites its argument: immutable bytes are refused
    assert one.value == 7 and not any(bad) and list(cul) == [7] * 8  # a failing call writes no result
    assert bytes(buf) == b"\xA5" * 4096


@pytest.mark.skipif(rsmi.device_count() != 0, reason="only meaningful on a host without a GPU")
def test_heal_fails_loudly_without_gpu():
    """No CPU fallback: valid arguments on a host without a GPU give RSMI_ERR_NO_DEVICE, write no
    result and leave the shards alone."""
    L = rsmi.lib()
    buf = (ctypes.c_uint8 * 4096)(*([0x3C] * 4096))
    p = ctypes.addressof(buf)
    bad = (ctypes.c_uint32 * 16)()
    pb = ctypes.addressof(bad)
    cul = (ctypes.c_int32 * 8)(*([7] * 8))
    pc = ctypes.addressof(cul)
    one = ctypes.c_int(7)
    with rsmi.Codec(4, 2) as c:
        assert L.rsmi_heal_batch_dev(c._h, p, 64, 256, p, 64, 128, 64, 1, pc, pb, None) == rsmi.ErrNoDevice
        assert L.rsmi_heal_batch_dev(c._h, p, 64, 256, p, 64, 128, 64, 1, pc, None, None) == rsmi.ErrNoDevice
        assert L.rsmi_heal_batch_host(c._h, p, 256, p, 128, 64, 1, pc, pb) == rsmi.ErrNoDevice
        assert L.rsmi_heal(c._h, p, 64, ctypes.byref(one)) == rsmi.ErrNoDevice
        one_block = bytearray(b"\x3C" * (6 * 64))
        with pytest.raises(rsmi.RsmiError) as e:
            c.heal(one_block, 64)
        assert e.value.code == rsmi.ErrNoDevice and one_block == b"\x3C" * (6 * 64)
    with pytest.raises(rsmi.RsmiError) as e:
        rsmi.NewErasure(4, 2, 64).heal([bytes(16)] * 6)
    assert e.value.code == rsmi.ErrNoDevice
    assert one.value == 7 and not any(bad) and list(cul) == [7] * 8
    assert bytes(buf) == b"\x3C" * 4096


def test_erasure_heal_raises_upstream_sentinels():
    """The checks of Erasure.locate, decided on the host before a codec is opened."""
    e = rsmi.NewErasure(4, 2, 64)
    good = [bytes(16)] * 6

    def code(shards):
        with pytest.raises(rsmi.RsmiError) as ex:
            e.heal(shards)
        return ex.value.code

    assert code(good[:5]) == rsmi.ErrTooFewShards
    assert code([]) == rsmi.ErrTooFewShards
    assert code(good + [bytes(16)]) == rsmi.ErrTooFewShards
    assert code([b""] * 6) == rsmi.ErrShardNoData
    assert code(good[:5] + [bytes(15)]) == rsmi.ErrShardSize
    assert code(good[:2] + [b""] + good[3:]) == rsmi.ErrShardSize  # a missing shard: nilok = false
    assert e._codec is None
