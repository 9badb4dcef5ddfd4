"""rsmi_encode_ragged_* on a host without a GPU: the symbols, the argument checks in the uniform
call's order, the first bad block, and the device-free classing of the blocks against a numpy
restatement of launch_plan's layout test.  The GPU legs are in test_ragged_encode.py,
test_ragged_matrix.py and test_ragged_fuzz.py."""
import ctypes

import numpy as np
import pytest

import rsmi

RAGGED = {"rsmi_encode_ragged_batch_dev": 6, "rsmi_encode_ragged_batch_host": 5, "rsmi_encode_ragged_classify": 7}
RAGGED_KS = {1, 2, 3, 4, 5, 6, 8, 10, 12, 16}
BOGUS = 16   # a pointer that cannot be read


def blocks_of(rows):
    """(nblocks, 5) uint64: S, data_off, data_shard_stride, parity_off, parity_shard_stride."""
    return np.ascontiguousarray(np.array(rows, dtype=np.uint64).reshape(-1, 5))


def test_symbols_are_exported_and_bound():
    raw = ctypes.CDLL(rsmi.LIB_PATH)
    L = rsmi.lib()
    for name, nargs in RAGGED.items():
        assert hasattr(raw, name), name
        f = getattr(L, name)
        assert f.restype is ctypes.c_int and len(f.argtypes) == nargs, name
    assert L.rsmi_abi_version() == 5
    for meth in ("encode_ragged_batch_dev", "encode_ragged_batch_host_ptr", "encode_ragged_classify"):
        assert callable(getattr(rsmi.Codec, meth))
    assert callable(rsmi.Erasure.encode_data_many)
    assert ctypes.sizeof(rsmi.RaggedBlock) == 40
    assert [f[0] for f in rsmi.RaggedBlock._fields_] == ["S", "data_off", "data_shard_stride", "parity_off",
                                                         "parity_shard_stride"]
    assert (rsmi.RaggedAligned, rsmi.RaggedUA, rsmi.RaggedFallback) == (0, 1, 2)


def test_argument_errors_match_the_uniform_call():
    """rsmi_encode_batch_dev's statuses for the shared arguments, in its order, before anything is
    dereferenced: the bases cannot be read (address 16)."""
    L = rsmi.lib()
    k, m, S = 4, 2, 32
    with rsmi.Codec(k, m) as c:
        h = c._h

        def ragged(ctx, data, parity, S_, ds, ps):
            b = blocks_of([[S_, 0, ds, 0, ps]])
            return (L.rsmi_encode_ragged_batch_dev(ctx, data, parity, b.ctypes.data, 1, None),
                    L.rsmi_encode_ragged_batch_host(ctx, data, parity, b.ctypes.data, 1))

        def uniform(ctx, data, parity, S_, ds, ps):
            return L.rsmi_encode_batch_dev(ctx, data, ds, k * ds, parity, ps, m * ps, S_, 1, None)

        table = [((None, BOGUS, BOGUS, S, S, S), rsmi.ErrInvalidArg),
                 ((h, None, BOGUS, S, S, S), rsmi.ErrInvalidArg),
                 ((h, BOGUS, None, S, S, S), rsmi.ErrInvalidArg),
                 ((h, BOGUS, BOGUS, 0, S, S), rsmi.ErrShardNoData),
                 ((h, None, BOGUS, 0, S, S), rsmi.ErrInvalidArg),          # NULL before S == 0
                 ((h, BOGUS, BOGUS, S, S - 1, S), rsmi.ErrInvalidArg),
                 ((h, BOGUS, BOGUS, S, S, S - 1), rsmi.ErrInvalidArg),
                 ((h, BOGUS, BOGUS, 0, 0, 0), rsmi.ErrShardNoData)]        # S == 0 before the stride
        for args, want in table:
            assert ragged(*args) == (want, want), args
            assert uniform(*args) == want, args
        # NULL blocks, also with nblocks == 0; then nblocks == 0: OK without a device, nothing read
        for nb in (0, 1):
            assert L.rsmi_encode_ragged_batch_dev(h, BOGUS, BOGUS, None, nb, None) == rsmi.ErrInvalidArg
            assert L.rsmi_encode_ragged_batch_host(h, BOGUS, BOGUS, None, nb) == rsmi.ErrInvalidArg
            assert L.rsmi_encode_ragged_classify(h, BOGUS, BOGUS, None, nb, None, None) == rsmi.ErrInvalidArg
        assert L.rsmi_encode_ragged_batch_dev(h, BOGUS, BOGUS, BOGUS, 0, None) == rsmi.OK
        assert L.rsmi_encode_ragged_batch_host(h, BOGUS, BOGUS, BOGUS, 0) == rsmi.OK
        assert L.rsmi_encode_ragged_classify(h, None, None, BOGUS, 0, None, None) == rsmi.OK
        assert L.rsmi_encode_ragged_classify(None, None, None, BOGUS, 0, None, None) == rsmi.ErrInvalidArg
        assert c.encode_ragged_classify(0, 0, []) == ([], [])


def test_first_bad_block_decides():
    """The blocks are scanned in index order and the first bad one gives the status, whatever
    follows it; nothing is read or written (bases at address 16), classify leaves its outputs."""
    L = rsmi.lib()
    good, no_data, short_d, short_p = [64, 0, 64, 0, 64], [0, 0, 64, 0, 64], [64, 0, 63, 0, 64], [64, 0, 64, 0, 63]
    cases = [([good, no_data, short_d], rsmi.ErrShardNoData),
             ([good, short_d, no_data], rsmi.ErrInvalidArg),
             ([good, good, short_p, no_data], rsmi.ErrInvalidArg),
             ([no_data, short_p], rsmi.ErrShardNoData),
             ([[0, 0, 0, 0, 0], short_p], rsmi.ErrShardNoData)]
    with rsmi.Codec(10, 4) as c:
        for rows, want in cases:
            b = blocks_of(rows)
            nb = b.shape[0]
            assert L.rsmi_encode_ragged_batch_dev(c._h, BOGUS, BOGUS, b.ctypes.data, nb, None) == want, rows
            assert L.rsmi_encode_ragged_batch_host(c._h, BOGUS, BOGUS, b.ctypes.data, nb) == want, rows
            cls = np.full(nb, 0xEE, dtype=np.uint8)
            tiles = np.full(nb, 0xEEEE, dtype=np.uint64)
            assert L.rsmi_encode_ragged_classify(c._h, BOGUS, BOGUS, b.ctypes.data, nb, cls.ctypes.data,
                                                 tiles.ctypes.data) == want
            assert (cls == 0xEE).all() and (tiles == 0xEEEE).all()


# ---------------------------------------------------------------- the classing, restated
def restate(k, data_base, parity_base, blocks):
    """launch_plan's layout test on each block's two halves: (classes, tiles)."""
    cls, tiles = [], []
    for S, doff, ds, poff, ps in (tuple(int(x) for x in row) for row in blocks):
        S16 = (S + 15) // 16 * 16
        aligned = all(x % 16 == 0 for x in (data_base + doff, parity_base + poff, ds, ps)) and ds >= S16 and ps >= S16
        if k not in RAGGED_KS or S >= 1 << 31 or (not aligned and S < 16):
            cls.append(rsmi.RaggedFallback)
            tiles.append(0)
        else:
            cls.append(rsmi.RaggedAligned if aligned else rsmi.RaggedUA)
            tiles.append((S + 1023) // 1024)
    return cls, tiles


def test_classify_each_term_of_the_predicate():
    """A batch of aligned blocks in which each block breaks one term alone: the data base, the
    parity base, the data offset, the parity offset, either stride's multiple of 16, either
    stride's room for the last chunk; at S >= 16 the block turns UA, below it falls back."""
    for S in (1000, 24, 16, 15, 7):
        P = (S + 15) // 16 * 16
        good = [S, 4096, P + 16, 8192, P + 32]
        rows = [good,
                [S, 4096 + 8, P + 16, 8192, P + 32],      # the data offset
                [S, 4096, P + 16, 8192 + 4, P + 32],      # the parity offset
                [S, 4096, P + 24, 8192, P + 32],          # the data stride's multiple
                [S, 4096, P + 16, 8192, P + 33],          # the parity stride's multiple
                good]
        if S % 16:
            rows += [[S, 4096, S, 8192, P + 32], [S, 4096, P + 16, 8192, S]]   # strides below roundup(S, 16)
        b = blocks_of(rows)
        with rsmi.Codec(10, 4) as c:
            for dbase, pbase in ((1 << 20, 1 << 21), ((1 << 20) + 1, 1 << 21), (1 << 20, (1 << 21) + 15)):
                got = c.encode_ragged_classify(dbase, pbase, b)
                assert got == restate(10, dbase, pbase, b), (S, dbase, pbase)
            cls, tiles = c.encode_ragged_classify(1 << 20, 1 << 21, b)
            odd = rsmi.RaggedUA if S >= 16 else rsmi.RaggedFallback
            assert cls == [0] + [odd] * 4 + [0] + [odd] * (len(rows) - 6), S
            # an odd base breaks every block
            cls, _ = c.encode_ragged_classify((1 << 20) + 1, 1 << 21, b)
            assert cls == [odd] * len(rows)
            # a NULL base is aligned: only the alignment counts
            assert c.encode_ragged_classify(0, 0, b) == restate(10, 0, 0, b)


def test_classify_tiles_at_the_seams():
    sizes = [1, 1023, 1024, 1025, 4096, 4097, 26215, (1 << 31) - 1, 1 << 31]
    want = [1, 1, 1, 2, 4, 5, 26, 1 << 21, 0]
    for pitch in (lambda S: (S + 15) // 16 * 16, lambda S: S):
        b = blocks_of([[S, 0, pitch(S), 0, pitch(S)] for S in sizes])
        with rsmi.Codec(4, 2) as c:
            cls, tiles = c.encode_ragged_classify(4096, 8192, b)
            assert (cls, tiles) == restate(4, 4096, 8192, b)
            assert tiles[1:] == want[1:] and cls[-1] == rsmi.RaggedFallback   # S >= 2^31: launch_plan's byte kernel
            assert tiles[0] == (1 if cls[0] != rsmi.RaggedFallback else 0)


@pytest.mark.parametrize("k,m", [(7, 2), (20, 4), (9, 3)])
def test_classify_k_without_a_kernel_falls_back(k, m):
    b = blocks_of([[S, 0, 4096, 0, 4096] for S in (1, 16, 1024, 4000)])
    with rsmi.Codec(k, m) as c:
        assert c.encode_ragged_classify(0, 0, b) == ([rsmi.RaggedFallback] * 4, [0] * 4) == restate(k, 0, 0, b)


def test_classify_seeded_draw():
    rng = np.random.default_rng(0xA66ED)
    nb = 400
    S = rng.integers(1, 70000, size=nb)
    S[:8] = [1, 15, 16, 17, 1023, 1024, 1025, 4097]
    rows = []
    for s in S:
        s = int(s)
        al = rng.integers(0, 2)
        ds = (s + 15) // 16 * 16 + 16 * int(rng.integers(0, 3)) if al else s + int(rng.integers(0, 40))
        ps = (s + 15) // 16 * 16 + 16 * int(rng.integers(0, 3)) if rng.integers(0, 4) else s + int(rng.integers(0, 40))
        rows.append([s, int(rng.integers(0, 1 << 33)) * (16 if al else 1), ds, int(rng.integers(0, 1 << 20)) * 16, ps])
    rows[0], rows[2], rows[3] = [1, 3, 5, 0, 16], [16, 0, 16, 0, 16], [17, 0, 17, 0, 32]   # one of each class
    b = blocks_of(rows)
    for k, m in ((10, 4), (5, 5), (16, 4)):
        with rsmi.Codec(k, m) as c:
            got = c.encode_ragged_classify(1 << 30, 1 << 31, b)
            assert got == restate(k, 1 << 30, 1 << 31, b)
            assert set(got[0]) == {0, 1, 2}
            # the sequence form of the binding gives the same descriptors
            assert c.encode_ragged_classify(1 << 30, 1 << 31, [tuple(int(x) for x in r) for r in rows[:20]]) == \
                tuple(x[:20] for x in got)


@pytest.mark.skipif(rsmi.device_count() != 0, reason="only meaningful on a host without a GPU")
def test_calls_fail_loudly_without_gpu():
    """No CPU fallback: RSMI_ERR_NO_DEVICE, the parity rows untouched."""
    L = rsmi.lib()
    k, m, S = 4, 2, 40
    data = np.full(2 * k * 48, 0x11, dtype=np.uint8)
    parity = np.full(2 * m * 48, 0x22, dtype=np.uint8)
    b = blocks_of([[S, 0, 48, 0, 48], [17, k * 48, 17, m * 48, 17]])
    with rsmi.Codec(k, m) as c:
        assert L.rsmi_encode_ragged_batch_dev(c._h, data.ctypes.data, parity.ctypes.data, b.ctypes.data, 2,
                                              None) == rsmi.ErrNoDevice
        assert L.rsmi_encode_ragged_batch_host(c._h, data.ctypes.data, parity.ctypes.data, b.ctypes.data,
                                               2) == rsmi.ErrNoDevice
        with pytest.raises(rsmi.RsmiError) as e:
            c.encode_ragged_batch_host_ptr(data.ctypes.data, parity.ctypes.data, b)
        assert e.value.code == rsmi.ErrNoDevice
    assert (data == 0x11).all() and (parity == 0x22).all()
    e = rsmi.NewErasure(k, m, 64)
    assert e.encode_data_many([]) == [] and e.encode_data_many([b"", b""]) == [[None] * 6, [None] * 6]
    with pytest.raises(rsmi.RsmiError) as err:
        e.encode_data_many([b"", b"abc"])
    assert err.value.code == rsmi.ErrNoDevice
