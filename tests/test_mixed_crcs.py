"""rsmi_reconstruct_mixed_batch_dev_crcs / _host_crcs on the GPU, exactly.

The rebuilt bytes are the definition's (test_mixed_reconstruct.definition: the oracle's reconstruct
of every block under its own masks) and equal rsmi_reconstruct_mixed_batch_dev's on a copy of the
buffer.  The raws: where the call wrote row r of block b,
  rsmi.crc16_entry(b"", raw16[b, r], S) == oracle crc16_ibm(row)
  rsmi.crc32_entry(b"", raw32[b, r], S) == zlib.crc32(row)
(rows of at most 2 KiB also against the raw references), and 0 everywhere else: present rows,
unwanted rows, intact blocks, blocks with too few rows.  The device outputs lie between guard words
and start as garbage.  No tolerances.

  1  every RS(4,2) pattern in one call; RS(10,4) one- and two-lost with per-block required masks;
     only raw16, only raw32, both
  2  the fallback beside fast classes, RS(5,5); a K without a class kernel; short unaligned rows
  3  equality with rsmi_reconstruct_rows_batch_host_crcs on uniform masks
  4  stream order: the mask arrays overwritten at once
  5  the scratch regrows and starts over, by repeated calls on one stream
  6  host paths: page-locked in place, the small call, the pipeline past one chunk
"""
import ctypes
import zlib

import numpy as np
import pytest

import oracle_lib as orc
from test_crc16 import raw_crc
from test_crc32_paths import raw16, raw32
from test_mixed_reconstruct import (MISSING, TOO_FEW, definition, host_chunk_blocks, layout, present_of, rs42_losses,
                                    same_bytes, stored, u8, wanted)
from test_verify import GAP, stripes

GUARD = 8
POISON, GUARD_WORD = 0x7EA5, 0x6A6A
SIZES = [17, 1025, 4097, 32769]
OUTS = [(True, True), (True, False), (False, True)]


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    rsmi = pytest.importorskip("rsmi")
    if not torch.cuda.is_available() or rsmi.device_count() == 0:
        pytest.skip("no GPU")
    return torch, rsmi


def written(W, status):
    """The rows the call writes: wanted rows of blocks with status OK."""
    return W & (np.asarray(status) == 0)[:, None]


def assert_raws(rsmi, image, wr, r16, r32, ctx):
    """r16 / r32 (nb, n) uint32 or None: the checksums of image's rows where wr, 0 elsewhere."""
    nb, n, S = image.shape
    for bits, got in ((16, r16), (32, r32)):
        if got is None:
            continue
        assert got.shape == (nb, n)
        stray = np.argwhere((got != 0) & ~wr)
        assert stray.size == 0, (ctx, bits, "a raw where nothing was rebuilt", stray[:4].tolist())
        for b, r in np.argwhere(wr):
            row = image[b, r].tobytes()
            raw = int(got[b, r])
            if bits == 16:
                assert raw >> 16 == 0
                assert rsmi.crc16_entry(b"", raw, S) == orc.crc16_ibm(row), (ctx, 16, b, r)
                if S <= 2048:
                    assert raw == raw_crc(row) == raw16(row), (ctx, 16, b, r)
            else:
                assert rsmi.crc32_entry(b"", raw, S) == zlib.crc32(row), (ctx, 32, b, r)
                if S <= 2048:
                    assert raw == raw32(row), (ctx, 32, b, r)


class DevRaws:
    def __init__(self, torch, words, want16, want32):
        self.t = [torch.full((2 * GUARD + words,), POISON, dtype=torch.int32, device="cuda") if w else None
                  for w in (want16, want32)]
        for t in self.t:
            if t is not None:
                t[:GUARD] = GUARD_WORD
                t[-GUARD:] = GUARD_WORD

    def ptr(self, i):
        return self.t[i].data_ptr() + 4 * GUARD if self.t[i] is not None else 0

    def read(self, shape):
        out = []
        for t in self.t:
            if t is None:
                out.append(None)
                continue
            a = t.cpu().numpy()
            assert (a[:GUARD] == GUARD_WORD).all() and (a[-GUARD:] == GUARD_WORD).all(), "a guard word was written"
            out.append(a[GUARD:-GUARD].astype(np.uint32).reshape(shape))
        return out


def check_dev(torch, rsmi, c, lay, sh, present, required, data_only, outs=(True, True), stream=None):
    """One rsmi_reconstruct_mixed_batch_dev_crcs over sh laid out by lay: statuses, the whole buffer
    against the definition and against rsmi_reconstruct_mixed_batch_dev on a copy, the raws."""
    k, m, n, nb = lay.k, lay.m, lay.n, lay.nb
    W = wanted(k, present, required, data_only)
    want_status, image = definition(k, m, sh, present, W)
    host = lay.fill(sh)
    d0, d1 = torch.from_numpy(host.copy()).cuda(), torch.from_numpy(host.copy()).cuda()
    raws = DevRaws(torch, nb * n, *outs)
    st = stream if stream is not None else torch.cuda.current_stream()
    P, R = u8(present), None if required is None else u8(required)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        old = c.reconstruct_mixed_batch_dev(d0.data_ptr() + lay.off, lay.rs, lay.bs, lay.S, nb, P, R, data_only,
                                            st.cuda_stream)
        got = c.reconstruct_mixed_batch_dev_crcs(d1.data_ptr() + lay.off, lay.rs, lay.bs, lay.S, nb, P, R, data_only,
                                                 raws.ptr(0), raws.ptr(1), st.cuda_stream)
    st.synchronize()
    ctx = (k, m, lay.S, lay.aligned, data_only, outs)
    assert got == old == want_status, (ctx, got, want_status)
    expect = host.copy()
    lay.rows(expect)[:] = image
    same_bytes(d1.cpu().numpy(), expect, ctx)
    same_bytes(d1.cpu().numpy(), d0.cpu().numpy(), ctx)
    r16, r32 = raws.read((nb, n))
    assert_raws(rsmi, image, written(W, want_status), r16, r32, ctx)
    return image, r16, r32


# ---------------------------------------------------------------- 1: every pattern
@pytest.mark.gpu
@pytest.mark.parametrize("data_only", [False, True], ids=["all", "data_only"])
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "ua"])
def test_rs42_every_pattern_in_one_call(gpu, aligned, data_only):
    """6 one-lost and 15 two-lost patterns, an intact block and a block with 3 rows lost."""
    torch, rsmi = gpu
    k, m = 4, 2
    losses = rs42_losses()
    present = present_of(6, losses)
    with rsmi.Codec(k, m) as c:
        for i, S in enumerate(SIZES):
            lay = layout(rsmi, k, m, S, len(losses), aligned)
            sh = stored(stripes(k, m, S, len(losses)), present)
            check_dev(torch, rsmi, c, lay, sh, present, None, data_only, OUTS[i % 3])
            assert c.last_kernel().startswith("rs_crc"), c.last_kernel()


def rs104_losses_12(nb, seed):
    """Seeded one- and two-lost patterns over data and parity."""
    rng = np.random.default_rng(seed)
    return [tuple(sorted(rng.choice(14, size=1 + (rng.integers(0, 3) == 0), replace=False).tolist())) for _ in range(nb)]


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "ua"])
def test_rs104_one_and_two_lost_with_required(gpu, aligned):
    """Per-block required masks: subsets of the missing rows (some empty), present rows named too; a
    too-few block with statuses.  Both folds."""
    torch, rsmi = gpu
    k, m, nb = 10, 4, 24
    losses = rs104_losses_12(nb - 1, 31) + [(0, 1, 2, 3, 4)]
    present = present_of(14, losses)
    rng = np.random.default_rng(32)
    required = rng.integers(0, 4, size=(nb, 14)) != 0
    required[5] = False
    required[nb - 1, 0] = True
    with rsmi.Codec(k, m) as c:
        for i, S in enumerate(SIZES):
            lay = layout(rsmi, k, m, S, nb, aligned)
            sh = stored(stripes(k, m, S, nb), present)
            for fold in (1, 0):
                c.set_option("crc16_fold", fold)
                c.set_option("crc32_fold", fold)
                check_dev(torch, rsmi, c, lay, sh, present, None, False, OUTS[(i + fold) % 3])
                image, r16, r32 = check_dev(torch, rsmi, c, lay, sh, present, required, False)
                assert not r16[nb - 1].any() and not r32[nb - 1].any() and not r16[5].any()


# ---------------------------------------------------------------- 2: the fallback
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "ua"])
def test_fallback_beside_fast_blocks(gpu, aligned):
    """RS(5,5): 5 rows lost is a two-tile plan and takes launch_plan, 1 or 2 lost is a class; RS(7,3):
    no class kernel at all.  The pass is independent of what rebuilt the row."""
    torch, rsmi = gpu
    S = 1030
    k, m = 5, 5
    losses = [(0,), (0, 1, 2, 3, 4), (7,), (0, 2, 4, 6, 8), (0, 2, 4, 6, 8), (3,), (1, 2, 3, 8, 9), (2, 6), ()]
    present = present_of(10, losses)
    sh = stored(stripes(k, m, S, len(losses)), present)
    with rsmi.Codec(k, m) as c:
        check_dev(torch, rsmi, c, layout(rsmi, k, m, S, len(losses), aligned), sh, present, None, False)
    k, m = 7, 3
    losses = [(0,), (0,), (1, 9), (2,), (0, 1, k), (0, 1, k), (), (k - 1, k)]
    present = present_of(10, losses)
    sh = stored(stripes(k, m, S, len(losses)), present)
    with rsmi.Codec(k, m) as c:
        check_dev(torch, rsmi, c, layout(rsmi, k, m, S, len(losses), aligned), sh, present, None, False)
        check_dev(torch, rsmi, c, layout(rsmi, k, m, S, len(losses), aligned), sh, present, None, True)


@pytest.mark.gpu
def test_fallback_unaligned_short_rows(gpu):
    """Unaligned rows shorter than 16 bytes: the byte-granular rebuild, then the UA named pass."""
    torch, rsmi = gpu
    k, m, S = 4, 2, 8
    losses = rs42_losses()
    present = present_of(6, losses)
    sh = stored(stripes(k, m, S, len(losses)), present)
    with rsmi.Codec(k, m) as c:
        check_dev(torch, rsmi, c, layout(rsmi, k, m, S, len(losses), False), sh, present, None, False)
        assert c.last_kernel().endswith(",UA")


# ---------------------------------------------------------------- 3: the uniform call
@pytest.mark.gpu
@pytest.mark.parametrize("k,m,lost,req", [(10, 4, (3,), None), (10, 4, (0, 5, 11, 13), (5, 13)), (4, 2, (1, 4), None)])
def test_equals_the_uniform_host_crcs(gpu, k, m, lost, req):
    """One pattern for all blocks: rows, raw16 and raw32 equal rsmi_reconstruct_rows_batch_host_crcs'."""
    torch, rsmi = gpu
    n, S, nb = k + m, 3000, 9
    present = present_of(n, [lost] * nb)
    required = np.zeros((nb, n), dtype=bool)
    required[:, list(req if req is not None else lost)] = True
    sh = stored(stripes(k, m, S, nb), present)
    with rsmi.Codec(k, m) as c:
        a, b = sh.copy().reshape(-1), sh.copy().reshape(-1)
        a16, a32, b16, b32 = (np.full(nb * n, POISON, dtype=np.uint32) for _ in range(4))
        c.reconstruct_rows_batch_host_crcs_ptr(a.ctypes.data, n * S, S, nb, present[0].tolist(), required[0].tolist(),
                                               a16.ctypes.data, a32.ctypes.data)
        got = c.reconstruct_mixed_batch_host_crcs_ptr(b.ctypes.data, n * S, S, nb, u8(present), u8(required), False,
                                                      b16.ctypes.data, b32.ctypes.data)
        assert got == [0] * nb
        assert np.array_equal(a, b) and not np.array_equal(a, sh.reshape(-1))
        assert np.array_equal(a16, b16) and np.array_equal(a32, b32) and a16.any() and a32.any()


# ---------------------------------------------------------------- 4: stream order
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "ua"])
def test_stream_order_masks_overwritten(gpu, aligned):
    """Behind a gate on a side stream: the call returns while the stream is still held, its mask
    arrays are overwritten at once, and the outputs are cloned and overwritten right behind it."""
    torch, rsmi = gpu
    from test_stream_order import Gate
    gate = Gate(torch)
    k, m, S, nb = 10, 4, 4097, 12
    n = k + m
    present = present_of(14, rs104_losses_12(nb, 41))
    W = wanted(k, present, None, False)
    sh = stored(stripes(k, m, S, nb), present)
    want_status, image = definition(k, m, sh, present, W)
    lay = layout(rsmi, k, m, S, nb, aligned)
    host = lay.fill(sh)
    pinned = torch.from_numpy(host).pin_memory()
    st = torch.cuda.Stream()
    with rsmi.Codec(k, m) as c:
        for gated in (False, True):  # the first pass builds the plans, the tables and the scratch
            d = torch.full((host.size,), 0xEE, dtype=torch.uint8, device="cuda")
            r16 = torch.full((nb * n,), 0x0BAD, dtype=torch.int32, device="cuda")
            r32 = torch.full((nb * n,), 0x0BAD, dtype=torch.int32, device="cuda")
            masks = u8(present).copy()
            torch.cuda.synchronize()
            e1, e2 = torch.cuda.Event(), torch.cuda.Event()
            with torch.cuda.stream(st):
                if gated:
                    gate()
                e1.record()
                d.copy_(pinned, non_blocking=True)
                got = c.reconstruct_mixed_batch_dev_crcs(d.data_ptr() + lay.off, lay.rs, lay.bs, S, nb,
                                                         masks.ctypes.data, None, False, r16.data_ptr(), r32.data_ptr(),
                                                         st.cuda_stream)
                masks[:] = 0xA5
                k16, k32 = r16.clone(), r32.clone()
                r16.fill_(-1)
                r32.fill_(-1)
                e2.record()
            if gated:
                assert not e1.query(), "the call waited for the stream"
            e2.synchronize()
            assert got == want_status
            expect = host.copy()
            lay.rows(expect)[:] = image
            same_bytes(d.cpu().numpy(), expect, ("stream order", gated))
            assert_raws(rsmi, image, written(W, want_status), k16.cpu().numpy().astype(np.uint32).reshape(nb, n),
                        k32.cpu().numpy().astype(np.uint32).reshape(nb, n), ("stream order", gated))
            assert (r16.cpu().numpy() == -1).all() and (r32.cpu().numpy() == -1).all(), "a launch ran late"


# ---------------------------------------------------------------- 5: the scratch
@pytest.mark.gpu
def test_scratch_regrow_and_wrap(gpu):
    """One context, one stream: a small call, then one whose lists and rows array outgrow the
    scratch's first size (1 MiB), the same again (it no longer fits behind the first: the scratch
    starts over), then the small one again.  RS(10,4), S = 16; the large batch repeats a 48-block
    period, so its image and raws are the period's, tiled."""
    torch, rsmi = gpu
    from test_mixed_reconstruct import rs104_losses
    k, m, S = 10, 4, 16
    n = k + m
    period = rs104_losses(48, 60)
    reps = 1500
    big = reps * len(period)
    P = present_of(14, period)
    base = stored(stripes(k, m, S, len(period)), P)
    # 8 bytes per block with rows to rebuild and 4 slots of 4 bytes per block
    fast_blocks = reps * sum(1 for lost in period if 0 < len(lost) <= m)
    words = fast_blocks * 8 + big * 4 * 4
    assert (1 << 20) < words and 2 * words > max(words, 3 << 19)  # it regrows; a second one does not fit behind it
    with rsmi.Codec(k, m) as c:
        lay = layout(rsmi, k, m, S, len(period), True)
        image, p16, p32 = check_dev(torch, rsmi, c, lay, base, P, None, False)
        lay_big = layout(rsmi, k, m, S, big, True)
        host = lay_big.fill(np.concatenate([base] * reps))
        expect = host.copy()
        lay_big.rows(expect)[:] = np.concatenate([image] * reps)
        masks = u8(np.concatenate([P] * reps))
        for _ in range(2):
            d = torch.from_numpy(host).cuda()
            raws = DevRaws(torch, big * n, True, True)
            c.reconstruct_mixed_batch_dev_crcs(d.data_ptr(), lay_big.rs, lay_big.bs, S, big, masks, None, False,
                                               raws.ptr(0), raws.ptr(1), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            same_bytes(d.cpu().numpy(), expect, "the large batch")
            r16, r32 = raws.read((reps, len(period), n))
            assert (r16 == p16[None]).all() and (r32 == p32[None]).all()
            del d, raws
        check_dev(torch, rsmi, c, lay, base, P, None, False)


# ---------------------------------------------------------------- 6: host paths
def host_case(rsmi, c, buf_of, k, m, S, sh, present, required, data_only, outs=(True, True), bs=None):
    """rsmi_reconstruct_mixed_batch_host_crcs over sh at pitch S, block stride bs, in the buffer
    buf_of(nbytes) returns: statuses, the whole buffer, the raws (host memory, poisoned first)."""
    n, nb = k + m, sh.shape[0]
    bs = bs or n * S
    buf = buf_of(nb * bs + 7)
    buf[:] = GAP
    rows = np.lib.stride_tricks.as_strided(buf, shape=(nb, n, S), strides=(bs, S, 1))
    rows[:] = sh
    W = wanted(k, present, required, data_only)
    want_status, image = definition(k, m, sh, present, W)
    expect = buf.copy()
    np.lib.stride_tricks.as_strided(expect, shape=(nb, n, S), strides=(bs, S, 1))[:] = image
    r16 = np.full(nb * n + 2, POISON, dtype=np.uint32)
    r32 = np.full(nb * n + 2, POISON, dtype=np.uint32)
    got = c.reconstruct_mixed_batch_host_crcs_ptr(buf.ctypes.data, bs, S, nb, u8(present),
                                                  None if required is None else u8(required), data_only,
                                                  r16.ctypes.data if outs[0] else None,
                                                  r32.ctypes.data if outs[1] else None)
    assert got == want_status
    same_bytes(buf, expect, (k, m, S, nb, bs))
    assert (r16[nb * n:] == POISON).all() and (r32[nb * n:] == POISON).all()
    assert outs[0] or (r16 == POISON).all()
    assert outs[1] or (r32 == POISON).all()
    assert_raws(rsmi, image, written(W, want_status), r16[:nb * n].reshape(nb, n) if outs[0] else None,
                r32[:nb * n].reshape(nb, n) if outs[1] else None, (k, m, S, nb, bs, outs))


@pytest.mark.gpu
def test_host_page_locked_and_small(gpu):
    """Page-locked shards are rebuilt and summed where they lie; a small pageable call goes through
    the page-locked staging; with the small-call limit off the same call takes the upload path."""
    torch, rsmi = gpu
    k, m = 10, 4
    L = rsmi.lib()
    held = []

    def pinned(nbytes):
        p = L.rsmi_host_alloc(nbytes)
        assert p
        held.append(p)
        return np.ctypeslib.as_array((ctypes.c_uint8 * nbytes).from_address(p))

    def pageable(nbytes):
        return np.empty(nbytes, dtype=np.uint8)

    try:
        with rsmi.Codec(k, m) as c:
            nb = 24
            for i, S in enumerate((1030, 4097, 16)):
                losses = rs104_losses_12(nb - 2, S) + [(0, 1, 2, 3, 4), ()]
                present = present_of(14, losses)
                sh = stored(stripes(k, m, S, nb), present)
                req = np.random.default_rng(S).integers(0, 2, size=(nb, 14)).astype(bool)
                for buf_of in (pinned, pageable):
                    host_case(rsmi, c, buf_of, k, m, S, sh, present, None, False, OUTS[i])
                    host_case(rsmi, c, buf_of, k, m, S, sh, present, req, False, bs=14 * S + 5)
                    host_case(rsmi, c, buf_of, k, m, S, sh[:1], present[:1], None, True)
            c.set_option("small_call_bytes", 0)
            for S in (1030, 1040):
                sh = stored(stripes(k, m, S, nb), present)
                host_case(rsmi, c, pageable, k, m, S, sh, present, None, False)
                host_case(rsmi, c, pageable, k, m, S, sh, present, None, False, OUTS[1], bs=14 * S + 3)
    finally:
        for p in held:
            L.rsmi_host_free(p)


@pytest.mark.gpu
def test_host_upload_past_one_chunk(gpu):
    """Pageable shards, four chunks with a short last one over the three staging slots (slot 0
    serves chunks 0 and 3): the raws of every chunk land at its offset.  Every block has its own
    pattern, a too-few block sits in the last chunk.  The stripes repeat every 64 blocks, so every
    rebuilt row and every raw is compared with the stripe it belongs to."""
    torch, rsmi = gpu
    k, m, S = 4, 2, 2049
    n = k + m
    ch = host_chunk_blocks(n, S)
    nb = 3 * ch + 5
    assert -(-nb // ch) == 4 and nb * n * S > 2 << 20
    pats = [lost for lost in rs42_losses() if len(lost) <= m]
    present = present_of(n, [pats[(b * 7 + b // ch) % 22] for b in range(nb)])
    present[nb - 2] = [True, False, False, False, True, True]  # too few, in the last chunk
    base = stripes(k, m, S, 64)
    b16 = np.array([[orc.crc16_ibm(base[b, r].tobytes()) for r in range(n)] for b in range(64)], dtype=np.uint32)
    b32 = np.array([[zlib.crc32(base[b, r].tobytes()) for r in range(n)] for b in range(64)], dtype=np.uint32)
    sh = base[np.arange(nb) % 64].copy()
    sh[~present] = MISSING
    W = wanted(k, present, None, False)
    W[nb - 2] = False
    before = sh.copy()
    r16 = np.full(nb * n, POISON, dtype=np.uint32)
    r32 = np.full(nb * n, POISON, dtype=np.uint32)
    with rsmi.Codec(k, m) as c:
        got = c.reconstruct_mixed_batch_host_crcs_ptr(sh.reshape(-1).ctypes.data, n * S, S, nb, u8(present), None, False,
                                                      r16.ctypes.data, r32.ctypes.data)
    assert got == [0] * (nb - 2) + [TOO_FEW, 0]
    assert np.array_equal(sh[~W], before[~W]), "a row that was not to be rebuilt changed"
    tiled = base[np.arange(nb) % 64]
    assert np.array_equal(sh[W], tiled[W])
    r16, r32 = r16.reshape(nb, n), r32.reshape(nb, n)
    assert not r16[~W].any() and not r32[~W].any()
    # finishing is a bijection of raw at fixed S: finish every distinct raw once
    f16 = {int(x): rsmi.crc16_entry(b"", int(x), S) for x in np.unique(r16[W])}
    f32 = {int(x): rsmi.crc32_entry(b"", int(x), S) for x in np.unique(r32[W])}
    want16, want32 = b16[np.arange(nb) % 64], b32[np.arange(nb) % 64]
    for b, r in np.argwhere(W):
        assert f16[int(r16[b, r])] == want16[b, r] and f32[int(r32[b, r])] == want32[b, r], (b, r)
