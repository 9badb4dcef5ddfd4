"""rsmi_locate_pair at the C-ABI boundary, on the CPU: the four entry points are exported and
bound, argument errors come before any device access and write no result (the checks and their
order are those of test_locate_abi.py), a host without a GPU reports RSMI_ERR_NO_DEVICE,
rsmi_locate_pair_checks (host-only) gives, for every pair, m - 2 independent rows that annihilate
exactly the pair's two columns of H = [M | I], the numpy span test of test_locate_pair.py equals the
oracle form of the definition, and the instantiated pair kernels are those of the source."""
import ctypes
import os
import re

import numpy as np
import pytest

import oracle_lib as orc
import rsmi
from test_locate_matrix import CSRC, LOCATE_KS
from test_locate_pair import (PAIR_KS, all_pairs, check_matrix, gf_tables, in_span, pair_bit, want_pair_np,
                              want_pair_oracle)
from test_verify import stripes

SYMS = ("rsmi_locate_pair_batch_dev", "rsmi_locate_pair_batch_host", "rsmi_locate_pair", "rsmi_locate_pair_checks")


def test_symbols_exported_and_bound():
    raw = ctypes.CDLL(rsmi.LIB_PATH)
    L = rsmi.lib()
    for s in SYMS:
        assert hasattr(raw, s), s
        f = getattr(L, s)
        assert f.restype is ctypes.c_int and f.argtypes, s
    assert len(L.rsmi_locate_pair_batch_dev.argtypes) == 12
    assert len(L.rsmi_locate_pair_batch_host.argtypes) == 9
    assert len(L.rsmi_locate_pair.argtypes) == 4
    assert len(L.rsmi_locate_pair_checks.argtypes) == 4
    for name in ("locate_pair", "locate_pair_batch_dev", "locate_pair_batch_host_ptr", "locate_pair_checks"):
        assert callable(getattr(rsmi.Codec, name)), name
    assert callable(rsmi.Erasure.locate_pair)
    assert L.rsmi_abi_version() == 5  # additive: the version stays


def test_argument_errors_come_before_device_access():
    """The checks of rsmi_locate_*, in their order: NULL -> INVALID_ARG (the flags pointer alone may
    be NULL), S == 0 -> SHARD_NO_DATA, a stride below S (or a block stride below the block's rows)
    -> INVALID_ARG, nblocks == 0 -> OK; none of them touches the device or writes a result."""
    L = rsmi.lib()
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf)
    bad = (ctypes.c_uint32 * 16)()
    pb = ctypes.addressof(bad)
    out = (ctypes.c_int32 * 8)(*([7] * 8))
    po = ctypes.addressof(out)
    one = (ctypes.c_int * 2)(7, 7)
    chk = (ctypes.c_uint8 * 8)(*([9] * 8))
    pk = ctypes.addressof(chk)
    with rsmi.Codec(4, 2) as c:
        h = c._h
        dev, host, single = L.rsmi_locate_pair_batch_dev, L.rsmi_locate_pair_batch_host, L.rsmi_locate_pair
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
        # the check rows: NULL, x == y, an index outside [0, n); m <= 2 writes nothing
        assert L.rsmi_locate_pair_checks(None, 0, 1, pk) == rsmi.ErrInvalidArg
        assert L.rsmi_locate_pair_checks(h, 0, 1, None) == rsmi.ErrInvalidArg
        assert L.rsmi_locate_pair_checks(h, 0, 1, pk) == rsmi.OK
        assert c.locate_pair_checks(0, 5) == b""
    with rsmi.Codec(4, 3) as c:
        for x, y in ((2, 2), (-1, 3), (3, -1), (0, 7), (7, 0), (7, 7)):
            assert L.rsmi_locate_pair_checks(c._h, x, y, pk) == rsmi.ErrInvalidArg, (x, y)
        assert L.rsmi_locate_pair_checks(c._h, 6, 0, pk) == rsmi.OK and list(chk)[:3] != [9, 9, 9]
        assert c.locate_pair_checks(6, 0) == c.locate_pair_checks(0, 6) == bytes(chk)[:3]
    assert list(one) == [7, 7] and not any(bad) and list(out) == [7] * 8 and list(chk)[3:] == [9] * 5


@pytest.mark.skipif(rsmi.device_count() != 0, reason="only meaningful on a host without a GPU")
def test_locate_pair_fails_loudly_without_gpu():
    """No CPU fallback: valid arguments on a host without a GPU give RSMI_ERR_NO_DEVICE and write no
    result; the check rows need no device."""
    L = rsmi.lib()
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf)
    bad = (ctypes.c_uint32 * 16)()
    pb = ctypes.addressof(bad)
    out = (ctypes.c_int32 * 8)(*([7] * 8))
    po = ctypes.addressof(out)
    one = (ctypes.c_int * 2)(7, 7)
    for k, m in ((4, 2), (4, 3)):
        with rsmi.Codec(k, m) as c:
            rs, n = 64, k + m
            assert L.rsmi_locate_pair_batch_dev(c._h, p, rs, n * rs, p, rs, n * rs, 64, 1, po, pb, None) == rsmi.ErrNoDevice
            assert L.rsmi_locate_pair_batch_dev(c._h, p, rs, n * rs, p, rs, n * rs, 64, 1, po, None, None) == rsmi.ErrNoDevice
            assert L.rsmi_locate_pair_batch_host(c._h, p, k * 64, p, m * 64, 64, 1, po, pb) == rsmi.ErrNoDevice
            assert L.rsmi_locate_pair(c._h, p, 64, one) == rsmi.ErrNoDevice
            with pytest.raises(rsmi.RsmiError) as e:
                c.locate_pair(bytearray(n * 64), 64)
            assert e.value.code == rsmi.ErrNoDevice
            assert len(c.locate_pair_checks(0, 1)) == (m - 2) * m
    assert list(one) == [7, 7] and not any(bad) and list(out) == [7] * 8


def test_erasure_locate_pair_raises_upstream_sentinels():
    """The checks of Erasure.locate, decided on the host before a codec is opened."""
    e = rsmi.NewErasure(4, 3, 64)
    good = [bytes(16)] * 7

    def code(shards):
        with pytest.raises(rsmi.RsmiError) as ex:
            e.locate_pair(shards)
        return ex.value.code

    assert code(good[:6]) == rsmi.ErrTooFewShards
    assert code(good + [bytes(16)]) == rsmi.ErrTooFewShards
    assert code([b""] * 7) == rsmi.ErrShardNoData
    assert code(good[:6] + [bytes(15)]) == rsmi.ErrShardSize
    assert code(good[:2] + [b""] + good[3:]) == rsmi.ErrShardSize
    assert e._codec is None


def _rank(A):
    MUL, INV = gf_tables()
    A = A.astype(np.uint8).copy()
    r = 0
    for j in range(A.shape[1]):
        nz = np.flatnonzero(A[r:, j])
        if not len(nz):
            continue
        p = r + nz[0]
        A[[r, p]] = A[[p, r]]
        A[r] = MUL[INV[A[r, j]], A[r]]
        f = A[:, j].copy()
        f[r] = 0
        A ^= MUL[f[:, None], A[r][None, :]]
        r += 1
        if r == A.shape[0]:
            break
    return r


@pytest.mark.parametrize("k,m", [(10, 4), (16, 4), (6, 3), (4, 4), (20, 4)])
def test_pair_checks_annihilate_exactly_the_pair(k, m):
    """For every pair: rank m - 2, C h_x = C h_y = 0, and C h_z != 0 for every other shard z, with
    the oracle's matrix and multiply.  No device is touched."""
    MUL, _ = gf_tables()
    H = check_matrix(k, m)
    n = k + m
    with rsmi.Codec(k, m) as c:
        for x, y in all_pairs(n):
            C = np.frombuffer(c.locate_pair_checks(x, y), dtype=np.uint8).reshape(m - 2, m)
            assert _rank(C) == m - 2, (x, y)
            CH = np.bitwise_xor.reduce(MUL[C[:, :, None], H[None, :, :]], axis=1)  # (m - 2, n)
            zero = ~CH.any(axis=0)
            assert np.flatnonzero(zero).tolist() == [x, y], (x, y, np.flatnonzero(zero))


@pytest.mark.parametrize("k,m", [(4, 4), (6, 3), (10, 4)])
def test_span_form_equals_oracle_form(k, m):
    """The numpy span test that stands in for the oracle on wide codes gives the oracle form's
    verdict: clean, one, two and three damaged shards over one to five dirty byte columns, and the
    check rows agree with both (a pair explains iff its check rows annihilate every syndrome)."""
    MUL, _ = gf_tables()
    n, S = k + m, 64
    rng = np.random.default_rng(100 * k + m)
    full = stripes(k, m, S, 3)[0]
    seen = set()
    with rsmi.Codec(k, m) as c:
        for draw in range(14):
            sh = full.copy()
            nd = draw % 4
            cols = rng.choice(S, size=int(rng.integers(1, 6)), replace=False)
            for x in rng.choice(n, size=nd, replace=False):
                sh[x, cols] ^= rng.integers(1, 256, size=len(cols), dtype=np.uint8)
            a, b = want_pair_np(k, m, sh), want_pair_oracle(k, m, sh)
            assert a == b, (draw, a, b)
            seen.add("pair" if a[1] >= 0 else "single" if a[0] >= 0 else "clean" if a[0] == -1 else "unknown")
            syn = orc.encode(k, m, np.ascontiguousarray(sh[:k])) ^ sh[k:]
            for x, y in all_pairs(n)[::7]:
                C = np.frombuffer(c.locate_pair_checks(x, y), dtype=np.uint8).reshape(m - 2, m)
                by_rows = not np.bitwise_xor.reduce(MUL[C[:, :, None], syn[None, :, :]], axis=1).any()
                assert by_rows == in_span(check_matrix(k, m)[:, [x, y]], syn), (draw, x, y)
    assert {"clean", "single", "pair"} <= seen


def test_pair_kernel_table_matches_source():
    """The instantiated (K, MT) set read from rs_pair_kernels.hip equals the locate kernels' K with
    MT in {3, 4}: 40 kernels with both layouts.  The bit order is the lexicographic one."""
    with open(os.path.join(CSRC, "rs_pair_kernels.hip")) as f:
        src = f.read()
    assert [int(x) for x in re.findall(r"\bfill_pair_k<\s*(\d+)\s*>\s*\(", src)] == LOCATE_KS == PAIR_KS
    assert re.findall(r"\bfill_pair_km<K,\s*(\d+)>\(", src) == ["3", "4"]
    assert len(re.findall(r"&rs_locate_pair_kernel<", src)) == 2
    assert re.search(r"t\.fn\[K\]\[MT\] = reinterpret_cast<void\*>\(&rs_locate_pair_kernel<K, MT, false>\);", src)
    assert re.search(r"t\.ua\[K\]\[MT\] = reinterpret_cast<void\*>\(&rs_locate_pair_kernel<K, MT, true>\);", src)
    assert 2 * 2 * len(PAIR_KS) == 40
    assert [pair_bit(5, x, y) for x, y in all_pairs(5)] == list(range(10))
