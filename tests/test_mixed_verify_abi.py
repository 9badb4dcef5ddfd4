"""rsmi_reconstruct_mixed_batch_dev_verify / _host_verify at the C-ABI boundary, on the CPU: the
symbols are exported and bound at ABI version 5, the header declares them parameter by parameter,
every argument check answers in its documented order before any device access (the pointers handed
in are never dereferenced: they point nowhere), the output is required, _host with nothing to
rebuild zeroes it without a device, and with something to rebuild and no GPU both calls say so and
write nothing.  The tile kernels of the new source are the 40 shapes x 2 layouts the GPU matrix
(test_mixed_verify_matrix.py) reaches."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import rsmi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rsmi.h")
CSRC = os.path.join(ROOT, "filedag-storage_amd", "csrc")
NEW = ("rsmi_reconstruct_mixed_batch_dev_verify", "rsmi_reconstruct_mixed_batch_host_verify")
P = 0x1000           # a non-null address that is never dereferenced
POISON = 0x7EA5
OK, INVALID, NO_DATA, TOO_FEW, NO_DEVICE = rsmi.OK, rsmi.ErrInvalidArg, rsmi.ErrShardNoData, rsmi.ErrTooFewShards, \
    rsmi.ErrNoDevice

DECLS = {
    "rsmi_reconstruct_mixed_batch_dev_verify": [
        "rsmi_ctx*", "uint8_t*", "size_t", "size_t", "size_t", "size_t", "const uint8_t*", "const uint8_t*", "int",
        "int32_t*", "uint32_t*", "void*"],
    "rsmi_reconstruct_mixed_batch_host_verify": [
        "rsmi_ctx*", "uint8_t*", "size_t", "size_t", "size_t", "const uint8_t*", "const uint8_t*", "int", "int32_t*",
        "uint32_t*"],
}
SHAPES_K = (1, 2, 3, 4, 5, 6, 8, 10, 12, 16)


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


def instantiated():
    """The (K, MT) the new source's fill_ calls instantiate, each on both layouts."""
    with open(os.path.join(CSRC, "rs_mixed_fused_kernels.hip")) as f:
        src = f.read()
    ks = [int(x) for x in re.findall(r"fill_mixed_fused_k<(\d+)>\(x\);", src)]
    mts = [int(x) for x in re.findall(r"fill_mixed_fused_km<K, (\d+)>\(t\);", src)]
    assert "rs_mixed_fused_kernel<K, MT, kFusedWavesPerSimd, false>" in src
    assert "rs_mixed_fused_kernel<K, MT, kFusedWavesPerSimd, true>" in src
    return [(k, mt) for k in ks for mt in mts]


def test_symbols_exported_bound_and_version_5():
    L = ctypes.CDLL(rsmi.LIB_PATH)
    bound = rsmi.lib()
    for s in NEW:
        assert hasattr(L, s), s
        assert getattr(bound, s).restype is ctypes.c_int and getattr(bound, s).argtypes, s
    assert bound.rsmi_abi_version() == 5
    with open(HEADER) as f:
        assert "#define RSMI_ABI_VERSION 5\n" in f.read()


def test_binding_signatures():
    """The binding's two methods, modelled on the _crcs pair: one output where those take two."""
    dev = list(inspect.signature(rsmi.Codec.reconstruct_mixed_batch_dev_verify).parameters)
    assert dev == ["self", "d_shards", "rs", "bs", "S", "nblocks", "present", "required", "data_only", "d_raw16_rows",
                   "stream", "status"]
    host = list(inspect.signature(rsmi.Codec.reconstruct_mixed_batch_host_verify_ptr).parameters)
    assert host == ["self", "ptr", "bs", "S", "nblocks", "present", "required", "data_only", "raw16_rows_ptr", "status"]
    crcs = list(inspect.signature(rsmi.Codec.reconstruct_mixed_batch_dev_crcs).parameters)
    assert [p for p in crcs if p not in ("d_raw16", "d_raw32")] == [p for p in dev if p != "d_raw16_rows"]


@pytest.mark.parametrize("name", NEW)
def test_header_declaration(name):
    assert declaration(name) == DECLS[name]
    assert len(getattr(rsmi.lib(), name).argtypes) == len(DECLS[name])


def test_verify_forms_share_the_mixed_calls_arguments():
    """The mixed calls with the one output put in before the stream (dev) or appended (host)."""
    dev, host = declaration("rsmi_reconstruct_mixed_batch_dev"), declaration("rsmi_reconstruct_mixed_batch_host")
    assert DECLS[NEW[0]] == dev[:-1] + ["uint32_t*"] + dev[-1:]
    assert DECLS[NEW[1]] == host + ["uint32_t*"]


def test_instantiated_shapes_and_makefile():
    assert instantiated() == [(k, mt) for k in SHAPES_K for mt in (1, 2, 3, 4)]
    with open(os.path.join(CSRC, "..", "Makefile")) as f:
        assert "csrc/rs_mixed_fused_kernels.hip" in f.read()
    # no INL form, no table form, and the combine kernel is the one the fused encode and the scrub run
    with open(os.path.join(CSRC, "rs_mixed_fused_kernels.hip")) as f:
        src = f.read()
    assert "BlockBases" not in src and "atomicInc" not in src
    with open(os.path.join(CSRC, "rsmi_mixed.cpp")) as f:
        assert "crc16_combine_mfma_kernel()" in f.read()


def dev_call(L, h, shards=P, rs=64, bs=1024, S=64, nb=1, present=P, required=None, status=None, out=P):
    return L.rsmi_reconstruct_mixed_batch_dev_verify(h, shards, rs, bs, S, nb, present, required, 0, status, out, None)


def host_call(L, h, shards=P, bs=1024, S=64, nb=1, present=P, required=None, status=None, out=P):
    return L.rsmi_reconstruct_mixed_batch_host_verify(h, shards, bs, S, nb, present, required, 0, status, out)


def test_argument_checks_in_order():
    """rsmi_reconstruct_mixed_batch_dev / _host's checks, order and statuses; the NULL output is one
    of the NULL checks, ahead of S == 0; nblocks == 0 comes last; then the classing of the masks."""
    L = rsmi.lib()
    k, m = 4, 2
    n = k + m
    with rsmi.Codec(k, m) as c:
        h = c._h
        for call in (dev_call, host_call):
            assert call(L, None) == INVALID
            assert call(L, h, shards=None, S=0) == INVALID
            assert call(L, h, present=None, S=0) == INVALID
            assert call(L, h, out=None, S=0) == INVALID
            assert call(L, h, out=None) == INVALID
            assert call(L, h, out=None, nb=0) == INVALID
            assert call(L, h, S=0) == NO_DATA
            assert call(L, h, S=0, nb=0) == NO_DATA
            assert call(L, h, nb=0) == OK
        assert dev_call(L, h, S=0, rs=0) == NO_DATA
        assert dev_call(L, h, rs=63, nb=0) == INVALID
        assert host_call(L, h, S=0, bs=0) == NO_DATA
        assert host_call(L, h, bs=n * 64 - 1, nb=0) == INVALID
        # too few rows without statuses: the whole batch, before any device access and any write
        few = np.array([[1, 1, 1, 1, 1, 1], [1, 1, 1, 0, 0, 0]], dtype=np.uint8)
        raw = np.full(2 * n, POISON, dtype=np.uint32)
        assert dev_call(L, h, nb=2, present=few.ctypes.data) == TOO_FEW
        assert host_call(L, h, nb=2, present=few.ctypes.data, out=raw.ctypes.data) == TOO_FEW
        assert (raw == POISON).all()


def test_host_with_nothing_to_rebuild_needs_no_device():
    """An intact block, a block whose missing rows are not required, a block with too few rows (with
    statuses): the output is zeroed, the statuses written, the rows untouched, no device asked for."""
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
        raw = np.full(nb * n + 2, POISON, dtype=np.uint32)
        status = np.full(nb, -7, dtype=np.int32)
        rc = L.rsmi_reconstruct_mixed_batch_host_verify(c._h, shards.ctypes.data, n * S, S, nb, present.ctypes.data,
                                                        required.ctypes.data, 0, status.ctypes.data, raw.ctypes.data)
        assert rc == OK
        assert status.tolist() == [OK, OK, TOO_FEW]
        assert (raw[:nb * n] == 0).all() and (raw[nb * n:] == POISON).all()
        assert np.array_equal(shards, before)
        raw[:] = POISON
        got = c.reconstruct_mixed_batch_host_verify_ptr(shards.ctypes.data, n * S, S, 2, present[:2], required[:2],
                                                        raw16_rows_ptr=raw.ctypes.data)
        assert got == [OK, OK] and (raw[:2 * n] == 0).all() and (raw[2 * n:] == POISON).all()


@pytest.mark.skipif(rsmi.device_count() != 0, reason="only meaningful on a host without a GPU")
def test_calls_fail_loudly_without_gpu():
    """No CPU path: with work to do both calls report RSMI_ERR_NO_DEVICE and write nothing, and so does
    the device-resident form with nothing to rebuild (it zeroes device memory on the stream)."""
    L = rsmi.lib()
    k, m, S = 4, 2, 64
    n = k + m
    intact = np.ones((1, n), dtype=np.uint8)
    lost = intact.copy()
    lost[0, 1] = 0
    shards = np.full(n * S, 0x33, dtype=np.uint8)
    raw = np.full(n, POISON, dtype=np.uint32)
    status = np.full(1, -7, dtype=np.int32)
    with rsmi.Codec(k, m) as c:
        assert dev_call(L, c._h, present=lost.ctypes.data) == NO_DEVICE
        assert dev_call(L, c._h, present=intact.ctypes.data) == NO_DEVICE
        assert host_call(L, c._h, shards=shards.ctypes.data, bs=n * S, present=lost.ctypes.data,
                         status=status.ctypes.data, out=raw.ctypes.data) == NO_DEVICE
        assert (raw == POISON).all() and (shards == 0x33).all() and status[0] == -7
        with pytest.raises(rsmi.RsmiError) as e:
            c.reconstruct_mixed_batch_dev_verify(P, 64, 1024, S, 1, lost, d_raw16_rows=P)
        assert e.value.code == NO_DEVICE
