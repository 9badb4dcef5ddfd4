"""rsmi_reconstruct_mixed_* on a host without a GPU: the symbols, the argument checks, the
device-free classing of the masks against a numpy restatement, and Erasure.decode_data_blocks_many's
sentinels.  The GPU legs are in test_mixed_reconstruct.py and test_mixed_matrix.py."""
import ctypes

import numpy as np
import pytest

import rsmi

POISON = 0x5EED
MIXED = {"rsmi_reconstruct_mixed_batch_dev": 11, "rsmi_reconstruct_mixed_batch_host": 9,
         "rsmi_reconstruct_mixed_classify": 9}


def test_symbols_are_exported_and_bound():
    raw = ctypes.CDLL(rsmi.LIB_PATH)
    L = rsmi.lib()
    for name, nargs in MIXED.items():
        assert hasattr(raw, name), name
        f = getattr(L, name)
        assert f.restype is ctypes.c_int and len(f.argtypes) == nargs, name
    assert L.rsmi_abi_version() == 5
    for meth in ("reconstruct_mixed_batch_dev", "reconstruct_mixed_batch_host_ptr", "reconstruct_mixed_classify"):
        assert callable(getattr(rsmi.Codec, meth))
    assert callable(rsmi.Erasure.decode_data_blocks_many)


# ---------------------------------------------------------------- argument errors
def test_argument_errors_match_the_uniform_calls():
    """The statuses of rsmi_reconstruct_batch_dev / _host for the shared arguments, checked in the
    same order, before anything is dereferenced: the bad calls get pointers that cannot be read
    (address 16), and status_out stays poisoned."""
    L = rsmi.lib()
    k, m, S, nb = 4, 2, 32, 3
    n = k + m
    buf = np.full(nb * n * S, 0x11, dtype=np.uint8)
    present = np.ones((nb, n), dtype=np.uint8)
    present[:, 1] = 0
    st = np.full(nb, POISON, dtype=np.int32)
    BOGUS = 16
    with rsmi.Codec(k, m) as c:
        h, p1 = c._h, present[0].ctypes.data

        def dev(ctx, sh, rs, S_, pres):
            return L.rsmi_reconstruct_mixed_batch_dev(ctx, sh, rs, n * S, S_, nb, pres, None, 1, st.ctypes.data, None)

        def host(ctx, sh, bs, S_, pres):
            return L.rsmi_reconstruct_mixed_batch_host(ctx, sh, bs, S_, nb, pres, None, 1, st.ctypes.data)

        def udev(ctx, sh, rs, S_, pres):
            return L.rsmi_reconstruct_batch_dev(ctx, sh, rs, n * S, S_, nb, pres, 1, None)

        def uhost(ctx, sh, bs, S_, pres):
            return L.rsmi_reconstruct_batch_host(ctx, sh, bs, S_, nb, pres, 1)

        # (mixed arguments, the uniform call's arguments, status)
        table_dev = [((None, BOGUS, S, S, BOGUS), (None, BOGUS, S, S, p1), rsmi.ErrInvalidArg),
                     ((h, None, S, S, BOGUS), (h, None, S, S, p1), rsmi.ErrInvalidArg),
                     ((h, BOGUS, S, S, None), (h, BOGUS, S, S, None), rsmi.ErrInvalidArg),
                     ((h, BOGUS, S, 0, BOGUS), (h, BOGUS, S, 0, p1), rsmi.ErrShardNoData),
                     ((h, None, S, 0, BOGUS), (h, None, S, 0, p1), rsmi.ErrInvalidArg),      # NULL before S == 0
                     ((h, BOGUS, S - 1, S, BOGUS), (h, BOGUS, S - 1, S, p1), rsmi.ErrInvalidArg),
                     ((h, BOGUS, S - 1, 0, BOGUS), (h, BOGUS, S - 1, 0, p1), rsmi.ErrShardNoData)]  # S == 0 before the stride
        for mixed_args, uni_args, want in table_dev:
            assert dev(*mixed_args) == want == udev(*uni_args), mixed_args
        table_host = [((None, BOGUS, n * S, S, BOGUS), (None, BOGUS, n * S, S, p1), rsmi.ErrInvalidArg),
                      ((h, None, n * S, S, BOGUS), (h, None, n * S, S, p1), rsmi.ErrInvalidArg),
                      ((h, BOGUS, n * S, S, None), (h, BOGUS, n * S, S, None), rsmi.ErrInvalidArg),
                      ((h, BOGUS, n * S, 0, BOGUS), (h, BOGUS, n * S, 0, p1), rsmi.ErrShardNoData),
                      ((h, BOGUS, n * S - 1, S, BOGUS), (h, BOGUS, n * S - 1, S, p1), rsmi.ErrInvalidArg),
                      ((h, BOGUS, 0, 0, BOGUS), (h, BOGUS, 0, 0, p1), rsmi.ErrShardNoData)]
        for mixed_args, uni_args, want in table_host:
            assert host(*mixed_args) == want == uhost(*uni_args), mixed_args
        assert (st == POISON).all() and (buf == 0x11).all()
        # nblocks == 0: OK without a device, nothing read
        assert L.rsmi_reconstruct_mixed_batch_dev(h, BOGUS, S, n * S, S, 0, BOGUS, None, 1, st.ctypes.data, None) == rsmi.OK
        assert L.rsmi_reconstruct_mixed_batch_host(h, BOGUS, n * S, S, 0, BOGUS, None, 1, st.ctypes.data) == rsmi.OK
        assert L.rsmi_reconstruct_mixed_classify(None, 0, None, None, 0, None, None, None, None) == rsmi.ErrInvalidArg
        assert L.rsmi_reconstruct_mixed_classify(h, 2, None, None, 0, None, None, None, None) == rsmi.ErrInvalidArg
        assert (st == POISON).all()


def test_too_few_and_nothing_to_do_need_no_device():
    """The classing comes before any device access: without status_out a block with too few rows
    fails the call as the uniform calls fail, and a batch with nothing to rebuild returns OK with
    its statuses, whether or not a GPU is there.  The shards pointer is never read."""
    L = rsmi.lib()
    k, m, S, nb = 4, 2, 32, 3
    n = k + m
    present = np.ones((nb, n), dtype=np.uint8)
    present[1, :3] = 0  # 3 present of 6, k = 4
    st = np.full(nb + 1, POISON, dtype=np.int32)
    BOGUS = 16
    with rsmi.Codec(k, m) as c:
        p = present.ctypes.data
        assert L.rsmi_reconstruct_mixed_batch_dev(c._h, BOGUS, S, n * S, S, nb, p, None, 1, None, None) == rsmi.ErrTooFewShards
        assert L.rsmi_reconstruct_mixed_batch_host(c._h, BOGUS, n * S, S, nb, p, None, 1, None) == rsmi.ErrTooFewShards
        # the too-few block is the only one with work: statuses, OK, no device
        assert L.rsmi_reconstruct_mixed_batch_dev(c._h, BOGUS, S, n * S, S, nb, p, None, 1, st.ctypes.data, None) == rsmi.OK
        assert st.tolist() == [0, rsmi.ErrTooFewShards, 0, POISON]
        st[:] = POISON
        assert L.rsmi_reconstruct_mixed_batch_host(c._h, BOGUS, n * S, S, nb, p, None, 1, st.ctypes.data) == rsmi.OK
        assert st.tolist() == [0, rsmi.ErrTooFewShards, 0, POISON]
        # parity lost only, data_only: nothing to rebuild; a required mask that names present rows only
        present[:] = 1
        present[:, k] = 0
        st[:] = POISON
        assert L.rsmi_reconstruct_mixed_batch_dev(c._h, BOGUS, S, n * S, S, nb, p, None, 1, st.ctypes.data, None) == rsmi.OK
        assert st.tolist() == [0, 0, 0, POISON]
        req = np.zeros((nb, n), dtype=np.uint8)
        req[:, 0] = 1
        assert L.rsmi_reconstruct_mixed_batch_host(c._h, BOGUS, n * S, S, nb, p, req.ctypes.data, 0, None) == rsmi.OK


@pytest.mark.skipif(rsmi.device_count() != 0, reason="only meaningful on a host without a GPU")
def test_calls_fail_loudly_without_gpu():
    """No CPU fallback: RSMI_ERR_NO_DEVICE, the buffer and status_out untouched."""
    L = rsmi.lib()
    k, m, S, nb = 4, 2, 32, 3
    n = k + m
    buf = np.full(nb * n * S, 0x11, dtype=np.uint8)
    present = np.ones((nb, n), dtype=np.uint8)
    present[0, 0] = present[2, 5] = 0
    st = np.full(nb, POISON, dtype=np.int32)
    with rsmi.Codec(k, m) as c:
        p = present.ctypes.data
        for status in (st.ctypes.data, None):
            assert L.rsmi_reconstruct_mixed_batch_dev(c._h, buf.ctypes.data, S, n * S, S, nb, p, None, 0, status,
                                                      None) == rsmi.ErrNoDevice
            assert L.rsmi_reconstruct_mixed_batch_host(c._h, buf.ctypes.data, n * S, S, nb, p, None, 0,
                                                       status) == rsmi.ErrNoDevice
        assert (st == POISON).all() and (buf == 0x11).all()
        with pytest.raises(rsmi.RsmiError) as e:
            c.reconstruct_mixed_batch_host_ptr(buf.ctypes.data, n * S, S, nb, present)
        assert e.value.code == rsmi.ErrNoDevice


# ---------------------------------------------------------------- the classing, restated
def restate(k, m, present, required, data_only):
    """include/rsmi.h rsmi_reconstruct_mixed_classify in numpy: (status, rows, pattern, npatterns)."""
    n = k + m
    P = np.asarray(present).reshape(-1, n) != 0
    if required is not None:
        W = ~P & (np.asarray(required).reshape(-1, n) != 0)
    else:
        W = ~P & ((np.arange(n) < k) | (not data_only))
    rows = W.sum(axis=1)
    few = (rows > 0) & (P.sum(axis=1) < k)
    seen = {}
    pattern = [seen.setdefault((P[b].tobytes(), W[b].tobytes()), len(seen)) for b in range(P.shape[0])]
    return (np.where(few, rsmi.ErrTooFewShards, 0).tolist(), np.where(few, 0, rows).tolist(), pattern, len(seen))


def classify(c, present, required, data_only):
    nb = present.shape[0]
    st, rows, pat, npat = c.reconstruct_mixed_classify(nb, present, required, data_only)
    return st, rows, pat, npat


def test_classify_rs42_every_mask():
    k, m = 4, 2
    n = k + m
    present = np.array([[(v >> i) & 1 for i in range(n)] for v in range(64)], dtype=np.uint8)
    present[present != 0] = np.arange(1, 1 + int((present != 0).sum())).astype(np.uint8) | 1  # any non-zero byte is "present"
    rng = np.random.default_rng(42)
    required = rng.integers(0, 2, size=(64, n), dtype=np.uint8) * 3
    with rsmi.Codec(k, m) as c:
        for data_only in (False, True):
            got = classify(c, present, None, data_only)
            assert got == restate(k, m, present, None, data_only), data_only
            assert got[3] == 64
        got = classify(c, present, required, True)
        assert got == restate(k, m, present, required, True)
        # the same masks twice: the numbering is by first appearance, the count stays
        twice = np.concatenate([present[::-1], present])
        got = classify(c, twice, None, False)
        assert got == restate(k, m, twice, None, False)
        assert got[2][:64] == list(range(64)) and got[2][64:] == list(range(63, -1, -1)) and got[3] == 64


def test_classify_rs104_seeded_draw():
    k, m, nb = 10, 4, 500
    n = k + m
    rng = np.random.default_rng(104)
    lost = rng.integers(0, 7, size=nb)
    lost[0], lost[1], lost[2] = 0, 5, 6  # all present, fewer than k present
    present = np.ones((nb, n), dtype=np.uint8)
    for b in range(nb):
        present[b, rng.choice(n, size=lost[b], replace=False)] = 0
    required = rng.integers(0, 2, size=(nb, n), dtype=np.uint8)
    with rsmi.Codec(k, m) as c:
        for req, data_only in ((None, False), (None, True), (required, False)):
            got = classify(c, present, req, data_only)
            want = restate(k, m, present, req, data_only)
            assert got == want, data_only
        st, rows, _, _ = classify(c, present, None, False)
        assert st[0] == 0 and rows[0] == 0 and st[1] == st[2] == rsmi.ErrTooFewShards and rows[1] == rows[2] == 0
        assert set(rows) == {0, 1, 2, 3, 4}


def test_classify_rs55_and_empty():
    with rsmi.Codec(5, 5) as c:
        present = np.array([[0] * 5 + [1] * 5, [1] * 10, [0, 1] * 5, [0] * 6 + [1] * 4], dtype=np.uint8)
        got = classify(c, present, None, False)
        assert got == restate(5, 5, present, None, False)
        assert got[1] == [5, 0, 5, 0] and got[0] == [0, 0, 0, rsmi.ErrTooFewShards]
        assert c.reconstruct_mixed_classify(0, None, None, False) == ([], [], [], 0)
        assert c.reconstruct_mixed_classify(0, np.zeros((0, 10), dtype=np.uint8)) == ([], [], [], 0)


# ---------------------------------------------------------------- Erasure.decode_data_blocks_many
def test_decode_data_blocks_many_sentinels():
    """decode_data_blocks' checks per block, the first failing block's sentinel in order, raised
    before any device call (this runs without a GPU) and with no list changed."""
    e = rsmi.NewErasure(4, 2, 64)
    S = e.shard_size()
    good = [bytes([i]) * S for i in range(6)]
    lossy = [None] + good[1:]

    def raises(blocks, code):
        before = [list(b) for b in blocks]
        with pytest.raises(rsmi.RsmiError) as err:
            e.decode_data_blocks_many(blocks)
        assert err.value.code == code
        assert blocks == before

    e.decode_data_blocks_many([])
    e.decode_data_blocks_many([list(good), list(good)])          # nothing missing: no device needed
    e.decode_data_blocks_many([good[:4] + [None, None]])         # parity lost only
    raises([list(good), lossy[:5]], rsmi.ErrTooFewShards)         # a shard list of the wrong length
    raises([[None, good[1], good[2][:-1], good[3], good[4], good[5]]], rsmi.ErrShardSize)
    raises([[None] * 6], rsmi.ErrShardNoData)
    raises([list(good), [None, None, None] + good[3:]], rsmi.ErrTooFewShards)  # 3 of 6 present
    # the first failing block in order decides
    raises([[None, None, None] + good[3:], [None, good[1], good[2][:-1], good[3], good[4], good[5]]],
           rsmi.ErrTooFewShards)
    raises([[None, good[1], good[2][:-1], good[3], good[4], good[5]], [None, None, None] + good[3:]],
           rsmi.ErrShardSize)
    # blocks that need decoding share one shard size
    short = [None] + [x[:-1] for x in good[1:]]
    raises([list(lossy), short], rsmi.ErrShardSize)
    if rsmi.device_count() == 0:
        raises([list(lossy), list(good)], rsmi.ErrNoDevice)
