"""rsmi_reconstruct_mixed_batch_dev_verify / _host_verify on the GPU, exactly.

The rebuilt bytes are the definition's (test_mixed_reconstruct.definition: the oracle's reconstruct
of every block under its own masks); the whole buffer, padding and gaps included, equals the
definition's image and rsmi_reconstruct_mixed_batch_dev's result on a copy.  The raws: in a block
with status OK and something to rebuild, for every row the call touched -- the first k present rows,
which it read, and the wanted missing rows, which it wrote --
  rsmi.crc16_entry(b"", raw[b, r], S) == oracle crc16_ibm(row as it lies after the call)
(rows of at most 2 KiB also raw == test_crc16.raw_crc(row)), and 0 everywhere else: present rows
beyond the first k, missing rows nobody wanted, intact blocks, blocks with too few rows.  The device
output lies between guard words and starts as garbage.  No tolerances.

  1  sizes: one chunk .. the headline row's seven units, both sides of the CRC's order; the padding trap
  2  every RS(4,2) pattern in one call, with and without statuses; RS(10,4) all one- and two-lost
     patterns with per-block required masks, parity-only rebuilds included
  3  accumulator pairing; a survivor damaged after encoding; a junk-filled unused present row
  4  the UA last window at byte phases 1, 7, 15
  5  the fallback beside fast classes, a K without a kernel, short unaligned rows
  6  segment cuts through option launch_units_max, split_launches; waves_per_cu = 1
  7  equality with _dev_crcs, rsmi_crc_named_rows_dev and rsmi_reconstruct_batch_host_verify
  8  stream order behind a gate; the scratch regrows on two streams
  9  a block past 4 GiB
 10  host paths: page-locked in place, small pageable, one block, past one chunk, strided blocks
"""
import ctypes
import itertools

import numpy as np
import pytest

import oracle_lib as orc
from test_crc16 import raw_crc
from test_mixed_reconstruct import (MISSING, TOO_FEW, definition, host_chunk_blocks, junk_unused_survivor, layout,
                                    present_of, rs42_losses, same_bytes, stored, u8, wanted)
from test_stream_order import Gate
from test_verify import GAP, Lay, stripes

GUARD = 8
POISON, GUARD_WORD = 0x7EA5, 0x6A6A
SIZES = [16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 5125, 26215, 32767, 32768, 40000]


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    rsmi = pytest.importorskip("rsmi")
    if not torch.cuda.is_available() or rsmi.device_count() == 0:
        pytest.skip("no GPU")
    return torch, rsmi


def fused_label(K, MT, aligned):
    return "rs_mixed_fused_kernel<K=%d,MT=%d>%s" % (K, MT, "" if aligned else ",UA")


def touched(k, present, W, status):
    """The rows the call reads or writes: in blocks with status OK and something to rebuild, the
    first k present rows and the wanted missing rows.  (nb, n) bool."""
    present = np.asarray(present, dtype=bool)
    T = np.zeros_like(present)
    for b in range(present.shape[0]):
        if status[b] == 0 and W[b].any():
            T[b, np.flatnonzero(present[b])[:k]] = True
            T[b] |= W[b]
    return T


def assert_raws(rsmi, image, T, got, ctx):
    """got (nb, n) uint32: R of image's rows where T, 0 elsewhere."""
    nb, n, S = image.shape
    assert got.shape == (nb, n)
    stray = np.argwhere((got != 0) & ~T)
    assert stray.size == 0, (ctx, "a raw of a row the call did not touch", stray[:4].tolist())
    for b, r in np.argwhere(T):
        row = image[b, r].tobytes()
        raw = int(got[b, r])
        assert raw >> 16 == 0
        assert rsmi.crc16_entry(b"", raw, S) == orc.crc16_ibm(row), (ctx, b, r)
        if S <= 2048:
            assert raw == raw_crc(row), (ctx, b, r)


class DevRaw:
    """nblocks * n words of device memory between guard words, starting as garbage."""

    def __init__(self, torch, words):
        self.t = torch.full((2 * GUARD + words,), POISON, dtype=torch.int32, device="cuda")
        self.t[:GUARD] = GUARD_WORD
        self.t[-GUARD:] = GUARD_WORD

    def ptr(self):
        return self.t.data_ptr() + 4 * GUARD

    def read(self, shape):
        a = self.t.cpu().numpy()
        assert (a[:GUARD] == GUARD_WORD).all() and (a[-GUARD:] == GUARD_WORD).all(), "a guard word was written"
        return a[GUARD:-GUARD].astype(np.uint32).reshape(shape)


def check_dev(torch, rsmi, c, lay, sh, present, required, data_only, label=None, status=True, host=None):
    """One rsmi_reconstruct_mixed_batch_dev_verify over sh laid out by lay: statuses, the whole buffer
    against the definition and against rsmi_reconstruct_mixed_batch_dev on a copy, the raws."""
    k, m, n, nb = lay.k, lay.m, lay.n, lay.nb
    W = wanted(k, present, required, data_only)
    want_status, image = definition(k, m, sh, present, W)
    if host is None:
        host = lay.fill(sh)
    d0, d1 = torch.from_numpy(host.copy()).cuda(), torch.from_numpy(host.copy()).cuda()
    raw = DevRaw(torch, nb * n)
    st = torch.cuda.current_stream().cuda_stream
    P, R = u8(present), None if required is None else u8(required)
    old = c.reconstruct_mixed_batch_dev(d0.data_ptr() + lay.off, lay.rs, lay.bs, lay.S, nb, P, R, data_only, st, status)
    got = c.reconstruct_mixed_batch_dev_verify(d1.data_ptr() + lay.off, lay.rs, lay.bs, lay.S, nb, P, R, data_only,
                                               raw.ptr(), st, status)
    torch.cuda.synchronize()
    ctx = (k, m, lay.S, lay.aligned, data_only)
    if status:
        assert got == old == want_status, (ctx, got, want_status)
    if label is not None:
        assert c.last_kernel() == label, (ctx, c.last_kernel(), label)
    expect = host.copy()
    lay.rows(expect)[:] = image
    same_bytes(d1.cpu().numpy(), expect, ctx)
    same_bytes(d1.cpu().numpy(), d0.cpu().numpy(), ctx)
    r = raw.read((nb, n))
    assert_raws(rsmi, image, touched(k, present, W, want_status), r, ctx)
    return image, r


# ---------------------------------------------------------------- 1: sizes, the padding trap
def small_losses(k, m):
    """Six blocks: one, two and m rows lost over data and parity, parity only, an intact block."""
    n = k + m
    return [(0,), (1, n - 1), tuple(range(k - 1, k - 1 + m)), (n - 1,), (), (k - 1, k)][:6]


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "ua"])
@pytest.mark.parametrize("k,m", [(10, 4), (4, 2)])
def test_sizes(gpu, k, m, aligned):
    """One chunk, a partial last chunk, exactly one tile, one full unit, a second unit of one tile,
    the headline row's seven units, both sides of the CRC's order (32767 bytes)."""
    torch, rsmi = gpu
    losses = small_losses(k, m)
    present = present_of(k + m, losses)
    with rsmi.Codec(k, m) as c:
        for S in SIZES:
            lay = layout(rsmi, k, m, S, len(losses), aligned)
            sh = stored(stripes(k, m, S, len(losses)), present)
            check_dev(torch, rsmi, c, lay, sh, present, None, False, fused_label(k, m, aligned))


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "ua"])
def test_padding_trap(gpu, aligned):
    """Junk in the padding, in the gaps and in the bytes at and past S changes no raw and no rebuilt
    byte, and stays what it was."""
    torch, rsmi = gpu
    k, m = 10, 4
    losses = small_losses(k, m)
    present = present_of(k + m, losses)
    rng = np.random.default_rng(77)
    with rsmi.Codec(k, m) as c:
        for S in (17, 1025, 4097):
            lay = layout(rsmi, k, m, S, len(losses), aligned)
            sh = stored(stripes(k, m, S, len(losses)), present)
            _, clean = check_dev(torch, rsmi, c, lay, sh, present, None, False)
            host = rng.integers(0, 256, size=lay.size, dtype=np.uint8)
            lay.rows(host)[:] = sh
            _, junk = check_dev(torch, rsmi, c, lay, sh, present, None, False, host=host)
            assert np.array_equal(clean, junk)


# ---------------------------------------------------------------- 2: every pattern
@pytest.mark.gpu
@pytest.mark.parametrize("data_only", [False, True], ids=["all", "data_only"])
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "ua"])
def test_rs42_every_pattern_in_one_call(gpu, aligned, data_only):
    """6 one-lost and 15 two-lost patterns, an intact block and a block with 3 rows lost; without
    status_out the too-few block fails the whole call before anything is launched or written."""
    torch, rsmi = gpu
    k, m = 4, 2
    losses = rs42_losses()
    present = present_of(6, losses)
    with rsmi.Codec(k, m) as c:
        for S in (17, 1025, 4097, 32769):
            lay = layout(rsmi, k, m, S, len(losses), aligned)
            sh = stored(stripes(k, m, S, len(losses)), present)
            junk_unused_survivor(k, sh, present)
            check_dev(torch, rsmi, c, lay, sh, present, None, data_only, fused_label(4, 2, aligned))
        host = lay.fill(sh)
        d = torch.from_numpy(host.copy()).cuda()
        raw = DevRaw(torch, len(losses) * 6)
        with pytest.raises(rsmi.RsmiError) as e:
            c.reconstruct_mixed_batch_dev_verify(d.data_ptr() + lay.off, lay.rs, lay.bs, S, len(losses), u8(present),
                                                 None, data_only, raw.ptr(), 0, status=False)
        torch.cuda.synchronize()
        assert e.value.code == TOO_FEW
        same_bytes(d.cpu().numpy(), host, "too few without statuses")
        assert (raw.read((len(losses), 6)) == POISON).all()
        # without the too-few block the call needs no statuses
        keep = [b for b, lost in enumerate(losses) if len(lost) <= m]
        lay2 = layout(rsmi, k, m, S, len(keep), aligned)
        check_dev(torch, rsmi, c, lay2, sh[keep], present[keep], None, data_only, status=False)


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "ua"])
def test_rs104_every_one_and_two_lost_pattern(gpu, aligned):
    """All 14 one-lost and 91 two-lost patterns, interleaved so neighbours differ in class; then with
    per-block required masks (subsets of the missing rows, some empty, present rows named too), and
    with only parity required, where every survivor is a data row."""
    torch, rsmi = gpu
    k, m, S = 10, 4, 1030
    one = [(i,) for i in range(14)]
    two = list(itertools.combinations(range(14), 2))
    losses = []
    for i, t in enumerate(two):
        losses.append(t)
        if i % 6 == 0 and i // 6 < 14:
            losses.append(one[i // 6])
    losses += one[len(losses) - 91:]
    assert len(losses) == 105 and len(set(losses)) == 105
    nb = len(losses)
    present = present_of(14, losses)
    sh = stored(stripes(k, m, S, nb), present)
    junk_unused_survivor(k, sh, present)
    lay = layout(rsmi, k, m, S, nb, aligned)
    rng = np.random.default_rng(5)
    required = rng.integers(0, 3, size=(nb, 14)) != 0
    required[7] = False
    parity_only = np.zeros((nb, 14), dtype=bool)
    parity_only[:, k:] = True
    with rsmi.Codec(k, m) as c:
        check_dev(torch, rsmi, c, lay, sh, present, None, False, fused_label(10, 2, aligned))
        _, r = check_dev(torch, rsmi, c, lay, sh, present, required, False)
        assert not r[7].any()
        _, r = check_dev(torch, rsmi, c, lay, sh, present, parity_only, False)
        only_parity_lost = [b for b, lost in enumerate(losses) if all(x >= k for x in lost)]
        assert len(only_parity_lost) == 4 + 6 and all(r[b, :k].all() for b in only_parity_lost)


# ---------------------------------------------------------------- 3: pairing, damage, unused rows
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "ua"])
@pytest.mark.parametrize("k,m", [(10, 4), (4, 2), (5, 3)])
def test_accumulator_pairing(gpu, k, m, aligned):
    """Block r: of the rows the call reads only row r is non-zero.  A rebuilt row is a GF(2^8)-linear
    image of the survivors in which no coefficient is zero (the code is MDS), so it cannot be non-zero
    alone: R is then non-zero exactly at r and at the rebuilt rows, and zero at every other survivor.
    A swap of the even and odd shard of an accumulator, or of the survivor and output slots, moves
    the non-zero words.  Row r < k: one other data row is lost; r >= k: data rows 0 .. r - k are, so
    parity row r is among the first k present."""
    torch, rsmi = gpu
    n, S = k + m, 1040
    losses = [((r + 1) % k,) if r < k else tuple(range(r - k + 1)) for r in range(n)]
    present = present_of(n, losses)
    rng = np.random.default_rng(11)
    sh = np.zeros((n, n, S), dtype=np.uint8)
    for r in range(n):
        assert r in np.flatnonzero(present[r])[:k]
        sh[r, r] = rng.integers(1, 256, size=S, dtype=np.uint8)
    sh[~present] = MISSING
    lay = layout(rsmi, k, m, S, n, aligned)
    with rsmi.Codec(k, m) as c:
        image, raw = check_dev(torch, rsmi, c, lay, sh, present, None, False)
    for r in range(n):
        nz = set(np.flatnonzero(raw[r]).tolist())
        assert nz == {r} | set(losses[r]), (r, sorted(nz))
        assert all(image[r, x].any() for x in losses[r])


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "ua"])
def test_damaged_survivor(gpu, aligned):
    """A survivor damaged after encoding: the rebuilt rows are wrong, and both they and the survivor's
    R are the oracle's values for the bytes as they lie: R is of the stored bytes."""
    torch, rsmi = gpu
    k, m, S, nb = 10, 4, 4097, 6
    losses = [(0,), (3, 12), (9,), (1, 2, 3), (13,), (0, 11)]
    present = present_of(14, losses)
    full = stripes(k, m, S, nb)
    sh = stored(full, present)
    hit = [(0, 1, 0), (1, 0, S - 1), (2, 10, 1024), (3, 4, 4096), (5, 5, 2000)]
    for b, r, at in hit:
        assert r in np.flatnonzero(present[b])[:k]
        sh[b, r, at] ^= 0x40
    lay = layout(rsmi, k, m, S, nb, aligned)
    with rsmi.Codec(k, m) as c:
        image, raw = check_dev(torch, rsmi, c, lay, sh, present, None, False)
        _, clean = check_dev(torch, rsmi, c, lay, stored(full, present), present, None, False)
    for b, r, at in hit:
        assert raw[b, r] != clean[b, r]
        for x in losses[b]:
            assert not np.array_equal(image[b, x], full[b, x]) and raw[b, x] != clean[b, x]
    assert np.array_equal(raw[4], clean[4])


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "ua"])
def test_unused_present_row_is_not_read(gpu, aligned):
    """A present row beyond the first k holds junk: it is not a survivor, its word is 0, and neither
    the rebuilt rows nor the other raws depend on it."""
    torch, rsmi = gpu
    k, m, S, nb = 10, 4, 1025, 14
    losses = [(i,) for i in range(14)]
    present = present_of(14, losses)
    sh = stored(stripes(k, m, S, nb), present)
    _, want = None, None
    with rsmi.Codec(k, m) as c:
        lay = layout(rsmi, k, m, S, nb, aligned)
        _, want = check_dev(torch, rsmi, c, lay, sh, present, None, False)
        junk = sh.copy()
        junk_unused_survivor(k, junk, present)
        assert not np.array_equal(junk, sh)
        _, got = check_dev(torch, rsmi, c, lay, junk, present, None, False)
    assert np.array_equal(got, want)
    for b in range(nb):
        unused = np.flatnonzero(present[b])[k:]
        assert unused.size == 3 and not got[b, unused].any()


# ---------------------------------------------------------------- 4: the UA last window
@pytest.mark.gpu
@pytest.mark.parametrize("phase", [1, 7, 15])
def test_ua_last_window(gpu, phase):
    """Rows at byte phases 1, 7 and 15, pitches that are no multiple of 16.  The only non-zero bytes
    of one survivor, and so of the rebuilt rows, lie in the row's last 16 bytes, which the last
    window holds at a shifted position and (S > 16) shares with the window before it; and a
    survivor damaged in those bytes."""
    torch, rsmi = gpu
    k, m = 4, 2
    n = k + m
    losses = [(0,), (1, 5), (4,), (2, 3)]
    nb = len(losses)
    present = present_of(n, losses)
    rng = np.random.default_rng(phase)
    with rsmi.Codec(k, m) as c:
        for S in (16, 17, 31, 1025, 4099):
            for rs in (S, S + 3):
                lay = Lay(rsmi, k, m, S, nb, False, rs=rs)
                lay.off = phase
                assert rs % 16 != 0 or S == 16
                # a: clean stripes with one survivor damaged inside the last window
                sh = stored(stripes(k, m, S, nb), present)
                for b in range(nb):
                    r = int(np.flatnonzero(present[b])[b % k])
                    sh[b, r, S - 1 - (b * 5) % min(16, S)] ^= 0x81
                check_dev(torch, rsmi, c, lay, sh, present, None, False, fused_label(4, 2, False))
                # b: everything zero but one survivor's last bytes
                z = np.zeros((nb, n, S), dtype=np.uint8)
                for b in range(nb):
                    r = int(np.flatnonzero(present[b])[(b + 1) % k])
                    z[b, r, S - 1 - b:] = rng.integers(1, 256, size=1 + b, dtype=np.uint8)
                z[~present] = MISSING
                image, raw = check_dev(torch, rsmi, c, lay, z, present, None, False)
                for b in range(nb):
                    assert all(raw[b, x] != 0 and image[b, x, S - 1 - b:].any() and not image[b, x, :S - 1 - b].any()
                               for x in losses[b])


# ---------------------------------------------------------------- 5: the fallback
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "ua"])
def test_fallback_beside_fast_blocks(gpu, aligned):
    """RS(5,5): 5 rows lost is a two-tile plan and takes launch_plan and the named rows pass over
    its 5 survivors and 5 rebuilt rows, 1 or 2 lost is a fused class, in one call; RS(7,2): no K = 7
    kernel at all."""
    torch, rsmi = gpu
    S = 1030
    k, m = 5, 5
    losses = [(0,), (0, 1, 2, 3, 4), (7,), (0, 2, 4, 6, 8), (0, 2, 4, 6, 8), (3,), (1, 2, 3, 8, 9), (2, 6), (),
              (0, 1, 2, 3, 4, 5)]
    present = present_of(10, losses)
    sh = stored(stripes(k, m, S, len(losses)), present)
    with rsmi.Codec(k, m) as c:
        _, raw = check_dev(torch, rsmi, c, layout(rsmi, k, m, S, len(losses), aligned), sh, present, None, False)
        assert c.last_kernel().startswith("rs_crc16_named"), c.last_kernel()
        assert raw[1].all() and raw[0].sum() and not raw[8].any() and not raw[9].any()
    k, m = 7, 2
    losses = [(0,), (0,), (1, 8), (2,), (0, 1, k), (), (k - 1, k), (8,)]
    present = present_of(9, losses)
    sh = stored(stripes(k, m, S, len(losses)), present)
    with rsmi.Codec(k, m) as c:
        for data_only in (False, True):
            check_dev(torch, rsmi, c, layout(rsmi, k, m, S, len(losses), aligned), sh, present, None, data_only)
            assert c.last_kernel().startswith("rs_crc16_named"), c.last_kernel()


@pytest.mark.gpu
def test_fallback_unaligned_short_rows(gpu):
    """Unaligned rows shorter than 16 bytes: the byte-granular rebuild, then the UA named rows pass."""
    torch, rsmi = gpu
    k, m = 4, 2
    losses = rs42_losses()
    present = present_of(6, losses)
    with rsmi.Codec(k, m) as c:
        for S in (1, 8, 15):
            sh = stored(stripes(k, m, S, len(losses)), present)
            check_dev(torch, rsmi, c, layout(rsmi, k, m, S, len(losses), False), sh, present, None, False)
            assert c.last_kernel() == "rs_crc16_named_mfma_kernel,UA"


# ---------------------------------------------------------------- 6: segment cuts
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "ua"])
def test_segment_cuts_and_split_launches(gpu, aligned):
    """launch_units_max of a few units: a segment is max(1, cap // tpb) blocks, and every segment
    launches one tile kernel per class that has a block in it; the records and the (entry, slot) words
    of a later segment and of a later class start over in the scratch.  S = 4097: 5 tiles, 2 units a
    block.  The classes alternate, so a class's list is cut inside a run of its entries."""
    torch, rsmi = gpu
    k, m, S, nb = 10, 4, 4097, 23
    tpb = 5
    losses = [tuple(sorted(np.random.default_rng(100 + b).choice(14, size=b % 3 + 1, replace=False).tolist()))
              for b in range(nb)]
    losses[9] = ()
    present = present_of(14, losses)
    sh = stored(stripes(k, m, S, nb), present)
    lay = layout(rsmi, k, m, S, nb, aligned)
    with rsmi.Codec(k, m) as c:
        _, want = check_dev(torch, rsmi, c, lay, sh, present, None, False)
        for cap in (3, 5, 12, 37, 64):
            seg = max(1, cap // tpb)
            count = sum(len({len(lost) for lost in losses[s:s + seg] if lost}) for s in range(0, nb, seg))
            c.set_option("launch_units_max", cap)
            try:
                # the plain mixed call takes as many tile launches, so the pair counts twice
                at = c.stat("split_launches")
                _, got = check_dev(torch, rsmi, c, lay, sh, present, None, False)
                assert c.stat("split_launches") - at == 2 * count, (cap, count)
            finally:
                c.set_option("launch_units_max", 0)
            assert np.array_equal(got, want), cap


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "ua"])
def test_waves_per_cu_1(gpu, aligned):
    """waves_per_cu = 1 caps the grids of the tile kernels that stride; the fused kernel keeps a
    workgroup per unit, and the fallback classes beside it walk strided."""
    torch, rsmi = gpu
    k, m, S = 5, 5, 5125
    losses = [(0,), (0, 1, 2, 3, 4), (7, 8), (3,), (1, 2, 3, 8, 9), (2, 6, 9), (), (0, 4, 5, 9)] * 3
    present = present_of(10, losses)
    sh = stored(stripes(k, m, S, len(losses)), present)
    with rsmi.Codec(k, m) as c:
        c.set_option("waves_per_cu", 1)
        check_dev(torch, rsmi, c, layout(rsmi, k, m, S, len(losses), aligned), sh, present, None, False)


# ---------------------------------------------------------------- 7: equality with the other calls
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "ua"])
def test_equals_dev_crcs_and_named_rows(gpu, aligned):
    """The rebuilt rows' raws equal _dev_crcs' raw16 on a copy; the survivors' equal
    rsmi_crc_named_rows_dev's over each block's first k present rows."""
    torch, rsmi = gpu
    k, m, S, nb = 10, 4, 5125, 16
    n = k + m
    rng = np.random.default_rng(3)
    losses = [tuple(sorted(rng.choice(14, size=b % 4 + 1, replace=False).tolist())) for b in range(nb)]
    present = present_of(14, losses)
    sh = stored(stripes(k, m, S, nb), present)
    lay = layout(rsmi, k, m, S, nb, aligned)
    W = wanted(k, present, None, False)
    with rsmi.Codec(k, m) as c:
        _, raw = check_dev(torch, rsmi, c, lay, sh, present, None, False)
        d = torch.from_numpy(lay.fill(sh)).cuda()
        r16 = torch.full((nb * n,), POISON, dtype=torch.int32, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        base = d.data_ptr() + lay.off
        c.reconstruct_mixed_batch_dev_crcs(base, lay.rs, lay.bs, S, nb, u8(present), None, False, r16.data_ptr(), 0, st)
        rows = np.array([np.flatnonzero(present[b])[:k] for b in range(nb)], dtype=np.int32)
        d_rows = torch.from_numpy(rows.reshape(-1)).cuda()
        named = torch.full((nb * k,), POISON, dtype=torch.int32, device="cuda")
        c.crc_named_rows_dev(base, lay.rs, lay.bs, base + k * lay.rs, lay.rs, lay.bs, S, nb, d_rows.data_ptr(), k,
                             named.data_ptr(), 0, st)
        torch.cuda.synchronize()
        r16 = r16.cpu().numpy().astype(np.uint32).reshape(nb, n)
        named = named.cpu().numpy().astype(np.uint32).reshape(nb, k)
    assert np.array_equal(raw[W], r16[W]) and r16[W].all()
    for b in range(nb):
        assert np.array_equal(raw[b, rows[b]], named[b]), b


@pytest.mark.gpu
@pytest.mark.parametrize("k,m,lost", [(10, 4, (3,)), (10, 4, (0, 5, 11, 13)), (4, 2, (1, 4))])
def test_equals_the_uniform_host_verify(gpu, k, m, lost):
    """One pattern for all blocks: the rows equal rsmi_reconstruct_batch_host_verify's and the k
    survivors' raws its raw16_in, survivor by survivor."""
    torch, rsmi = gpu
    n, S, nb = k + m, 3000, 9
    present = present_of(n, [lost] * nb)
    sh = stored(stripes(k, m, S, nb), present)
    L = rsmi.lib()
    with rsmi.Codec(k, m) as c:
        a, b = sh.copy().reshape(-1), sh.copy().reshape(-1)
        raw_in = np.full(nb * k, POISON, dtype=np.uint32)
        p = (ctypes.c_uint8 * n)(*[int(x) for x in present[0]])
        rc = L.rsmi_reconstruct_batch_host_verify(c._h, a.ctypes.data, n * S, S, nb, p, 0, raw_in.ctypes.data)
        assert rc == 0
        raw = np.full(nb * n, POISON, dtype=np.uint32)
        got = c.reconstruct_mixed_batch_host_verify_ptr(b.ctypes.data, n * S, S, nb, u8(present), None, False,
                                                        raw.ctypes.data)
        assert got == [0] * nb
    assert np.array_equal(a, b) and not np.array_equal(a, sh.reshape(-1))
    used = np.flatnonzero(present[0])[:k]
    assert np.array_equal(raw.reshape(nb, n)[:, used], raw_in.reshape(nb, k)) and raw_in.all()


# ---------------------------------------------------------------- 8: stream order, the scratch
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "ua"])
def test_stream_order_masks_overwritten(gpu, aligned):
    """Behind a gate on a side stream: the call returns while the stream is still held, its mask
    arrays are overwritten at once, and the output is cloned and overwritten right behind it."""
    torch, rsmi = gpu
    gate = Gate(torch)
    k, m, S, nb = 10, 4, 4097, 12
    n = k + m
    rng = np.random.default_rng(41)
    losses = [tuple(sorted(rng.choice(14, size=1 + b % 2, replace=False).tolist())) for b in range(nb)]
    present = present_of(14, losses)
    W = wanted(k, present, None, False)
    sh = stored(stripes(k, m, S, nb), present)
    want_status, image = definition(k, m, sh, present, W)
    T = touched(k, present, W, want_status)
    lay = layout(rsmi, k, m, S, nb, aligned)
    host = lay.fill(sh)
    pinned = torch.from_numpy(host).pin_memory()
    st = torch.cuda.Stream()
    with rsmi.Codec(k, m) as c:
        for gated in (False, True):  # the first pass builds the plans, the tables and the scratch
            d = torch.full((host.size,), 0xEE, dtype=torch.uint8, device="cuda")
            raw = torch.full((nb * n,), 0x0BAD, dtype=torch.int32, device="cuda")
            masks = u8(present).copy()
            torch.cuda.synchronize()
            e1, e2 = torch.cuda.Event(), torch.cuda.Event()
            with torch.cuda.stream(st):
                if gated:
                    gate()
                e1.record()
                d.copy_(pinned, non_blocking=True)
                got = c.reconstruct_mixed_batch_dev_verify(d.data_ptr() + lay.off, lay.rs, lay.bs, S, nb,
                                                           masks.ctypes.data, None, False, raw.data_ptr(), st.cuda_stream)
                masks[:] = 0xA5
                kept = raw.clone()
                raw.fill_(-1)
                e2.record()
            if gated:
                assert not e1.query(), "the call waited for the stream"
            e2.synchronize()
            assert got == want_status
            expect = host.copy()
            lay.rows(expect)[:] = image
            same_bytes(d.cpu().numpy(), expect, ("stream order", gated))
            assert_raws(rsmi, image, T, kept.cpu().numpy().astype(np.uint32).reshape(nb, n), ("stream order", gated))
            assert (raw.cpu().numpy() == -1).all(), "a launch ran late"


@pytest.mark.gpu
def test_scratch_regrows_on_two_streams(gpu):
    """One context, two streams: a small call, a larger one whose records outgrow the stream's
    scratch, a larger one still, then the small one again, alternating the streams; every call's
    bytes and raws are the period's."""
    torch, rsmi = gpu
    k, m, S = 10, 4, 1025
    n = k + m
    rng = np.random.default_rng(8)
    period = [tuple(sorted(rng.choice(14, size=b % 4 + 1, replace=False).tolist())) for b in range(8)]
    P = present_of(14, period)
    base = stored(stripes(k, m, S, len(period)), P)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    with rsmi.Codec(k, m) as c:
        lay = layout(rsmi, k, m, S, len(period), True)
        image, praw = check_dev(torch, rsmi, c, lay, base, P, None, False)
        for i, reps in enumerate((1, 8, 1, 40, 8, 1)):
            st = streams[i % 2]
            nb = reps * len(period)
            lay_big = layout(rsmi, k, m, S, nb, True)
            host = lay_big.fill(np.concatenate([base] * reps))
            expect = host.copy()
            lay_big.rows(expect)[:] = np.concatenate([image] * reps)
            d = torch.from_numpy(host).cuda()
            raw = DevRaw(torch, nb * n)
            torch.cuda.synchronize()
            c.reconstruct_mixed_batch_dev_verify(d.data_ptr(), lay_big.rs, lay_big.bs, S, nb, u8(np.concatenate([P] * reps)),
                                                 None, False, raw.ptr(), st.cuda_stream)
            st.synchronize()
            same_bytes(d.cpu().numpy(), expect, ("regrow", i))
            assert (raw.read((reps, len(period), n)) == praw[None]).all(), i


# ---------------------------------------------------------------- 9: offsets past 4 GiB
@pytest.mark.gpu
def test_offsets_past_4gib(gpu):
    """Two blocks a block stride of 4 GiB + 4096 apart, each with its own pattern, aligned and
    shifted by one byte.  A row or block offset truncated to 32 bits would land in the near block."""
    torch, rsmi = gpu
    if torch.cuda.mem_get_info()[0] < 8 << 30:
        pytest.skip("needs 8 GiB of free device memory")
    k, m, S, nb = 4, 2, 1040, 2
    n = k + m
    bs = 2 ** 32 + 4096
    full = stripes(k, m, S, nb)
    losses = [(1,), (0, 5)]
    present = present_of(6, losses)
    sh = stored(full, present)
    W = wanted(k, present, None, False)
    T = touched(k, present, W, [0, 0])
    try:
        with rsmi.Codec(k, m) as c:
            d = torch.empty(2 ** 32 + 2 ** 20, dtype=torch.uint8, device="cuda")
            assert 1 + bs + n * S <= d.numel()
            for off in (0, 1):
                for b in range(nb):
                    for i in range(n):
                        o = off + b * bs + i * S
                        d[o:o + S].copy_(torch.from_numpy(sh[b, i]))
                raw = DevRaw(torch, nb * n)
                got = c.reconstruct_mixed_batch_dev_verify(d.data_ptr() + off, S, bs, S, nb, u8(present), None, False,
                                                           raw.ptr(), torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                assert got == [0, 0] and c.last_kernel() == fused_label(4, 2, off == 0)
                for b in range(nb):
                    for i in range(n):
                        o = off + b * bs + i * S
                        assert np.array_equal(d[o:o + S].cpu().numpy(), full[b, i]), (off, b, i)
                assert_raws(rsmi, np.array(full), T, raw.read((nb, n)), ("past 4 GiB", off))
            del d
    finally:
        torch.cuda.empty_cache()


# ---------------------------------------------------------------- 10: host paths
def host_case(rsmi, c, buf_of, k, m, S, sh, present, required, data_only, bs=None):
    """rsmi_reconstruct_mixed_batch_host_verify over sh at pitch S, block stride bs, in the buffer
    buf_of(nbytes) returns: statuses, the whole buffer (only wanted rows change), the raws."""
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
    raw = np.full(nb * n + 2, POISON, dtype=np.uint32)
    got = c.reconstruct_mixed_batch_host_verify_ptr(buf.ctypes.data, bs, S, nb, u8(present),
                                                    None if required is None else u8(required), data_only,
                                                    raw.ctypes.data)
    assert got == want_status
    same_bytes(buf, expect, (k, m, S, nb, bs))
    assert (raw[nb * n:] == POISON).all()
    assert_raws(rsmi, image, touched(k, present, W, want_status), raw[:nb * n].reshape(nb, n), (k, m, S, nb, bs))


@pytest.mark.gpu
def test_host_page_locked_and_small(gpu):
    """Page-locked shards are rebuilt and summed where they lie; a small pageable call goes through
    the page-locked staging; the one-block call; with the small-call limit off the same call takes the
    upload path.  Strided blocks with required masks on each."""
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
            for S in (1030, 4097, 16):
                rng = np.random.default_rng(S)
                losses = [tuple(sorted(rng.choice(14, size=1 + b % 3, replace=False).tolist())) for b in range(nb - 2)]
                losses += [(0, 1, 2, 3, 4), ()]
                present = present_of(14, losses)
                sh = stored(stripes(k, m, S, nb), present)
                junk_unused_survivor(k, sh, present)
                req = rng.integers(0, 2, size=(nb, 14)).astype(bool)
                for buf_of in (pinned, pageable):
                    host_case(rsmi, c, buf_of, k, m, S, sh, present, None, False)
                    host_case(rsmi, c, buf_of, k, m, S, sh, present, req, False, bs=14 * S + 5)
                    host_case(rsmi, c, buf_of, k, m, S, sh[:1], present[:1], None, True)
            c.set_option("small_call_bytes", 0)
            for S in (1030, 1040):
                sh = stored(stripes(k, m, S, nb), present)
                host_case(rsmi, c, pageable, k, m, S, sh, present, None, False)
                host_case(rsmi, c, pageable, k, m, S, sh, present, req, False, bs=14 * S + 3)
    finally:
        for p in held:
            L.rsmi_host_free(p)


@pytest.mark.gpu
def test_host_upload_past_one_chunk(gpu):
    """Pageable shards, four chunks with a short last one over the three staging slots (slot 0
    serves chunks 0 and 3): the raws of every chunk land at its offset.  Every block has its own
    pattern, a too-few block sits in the last chunk.  The stripes repeat every 64 blocks, so every
    rebuilt row and every raw is compared with the stripe it belongs to; only wanted rows change."""
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
    sh = base[np.arange(nb) % 64].copy()
    sh[~present] = MISSING
    W = wanted(k, present, None, False)
    W[nb - 2] = False
    status = [0] * (nb - 2) + [TOO_FEW, 0]
    T = touched(k, present, W, status)
    before = sh.copy()
    raw = np.full(nb * n, POISON, dtype=np.uint32)
    with rsmi.Codec(k, m) as c:
        got = c.reconstruct_mixed_batch_host_verify_ptr(sh.reshape(-1).ctypes.data, n * S, S, nb, u8(present), None,
                                                        False, raw.ctypes.data)
    assert got == status
    assert np.array_equal(sh[~W], before[~W]), "a row that was not to be rebuilt changed"
    tiled = base[np.arange(nb) % 64]
    assert np.array_equal(sh[W], tiled[W])
    raw = raw.reshape(nb, n)
    assert not raw[~T].any()
    # finishing is a bijection of raw at fixed S: finish every distinct raw once
    fin = {int(x): rsmi.crc16_entry(b"", int(x), S) for x in np.unique(raw[T])}
    want16 = b16[np.arange(nb) % 64]
    for b, r in np.argwhere(T):
        assert fin[int(raw[b, r])] == want16[b, r], (b, r)
