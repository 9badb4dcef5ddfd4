"""rsmi_reconstruct_mixed_batch_* on the GPU against the definition, computed with the CPU oracle.

Every block is compared with oracle_lib.reconstruct under that block's own masks, and the whole
buffer is compared byte for byte with the definition's image: the sentinels of test_verify.Lay in
padding and gaps, the MISSING bytes of missing rows nobody asked for, untouched blocks.  There are
no tolerances.  One tile is 1 KiB of a row; S in {16, 1000, 1030, 3000, 5121} gives 1, 1, 2, 3, 6
tiles per block, and neighbouring blocks differ in pattern and in class, so a workgroup's four
waves hold tiles of different blocks, patterns and (through the class lists) positions.

  1  RS(4,2): all 21 loss patterns, an intact block and a 3-lost block in one call
  2  RS(10,4): 64 blocks, 1-4 rows lost, classes interleaved; per-block required masks
  3  status_out == NULL with a too-few block; all blocks intact
  4  waves_per_cu = 1: the strided walk restages its tables
  5  the fallback beside fast blocks: RS(5,5), RS(7,3), RS(20,4), unaligned S = 8
  6  scratch regrow and start-over on one stream, then three streams
  7  stream order: two calls back to back behind a gate, the mask arrays overwritten at once
  8  equality with rsmi_reconstruct_rows_batch_dev; offsets past 4 GiB
  9  host entry: page-locked in place, small pageable, four chunks over the three slots
 10  no side effects on the other calls of the context; Erasure.decode_data_blocks_many
 11  the segment seam of launch_mixed: 2^22 + 5 blocks, fast classes and fallback runs across it
 12  past 32 caller streams: the scratch of every stream is freed on the way, twice
 13  host entry: three chunks with gaps between the blocks and per-block required masks
"""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import oracle_lib as orc
from test_kernel_matrix import fast_label, generic_label
from test_stream_order import Gate
from test_verify import GAP, Lay, stripes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIXED_CPP = os.path.join(ROOT, "filedag-storage_amd", "csrc", "rsmi_mixed.cpp")
MISSING = 0x5C     # what a missing row holds before the call
POISON = 0x5EED
TOO_FEW = 2
SIZES = [16, 1000, 1030, 3000, 5121]
SEAM = 1 << 22         # blocks per segment of launch_mixed (leg 0 pins it)
PAST_STREAMS = 40      # mixed_scratch() evicts once it keeps 32 streams (leg 0 pins it)


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    rsmi = pytest.importorskip("rsmi")
    if not torch.cuda.is_available() or rsmi.device_count() == 0:
        pytest.skip("no GPU")
    assert rsmi.ErrTooFewShards == TOO_FEW
    return torch, rsmi


def mixed_label(K, MT, aligned):
    return "rs_mixed_kernel<K=%d,MT=%d>%s" % (K, MT, "" if aligned else ",UA")


def layout(rsmi, k, m, S, nb, aligned):
    """test_verify.Lay; the unaligned form starts one byte past an aligned base, rows at pitch S."""
    lay = Lay(rsmi, k, m, S, nb, aligned)
    if not aligned:
        lay.off = 1
    return lay


def present_of(n, losses):
    """(nb, n) bool from a list of lost-row tuples."""
    p = np.ones((len(losses), n), dtype=bool)
    for b, lost in enumerate(losses):
        p[b, list(lost)] = False
    return p


def wanted(k, present, required, data_only):
    """The rows the call writes, per block, before the too-few rule: (nb, n) bool."""
    n = present.shape[1]
    if required is not None:
        return ~present & required
    return ~present & ((np.arange(n) < k) | (not data_only))


def stored(full, present):
    """The shards as the caller holds them: missing rows hold MISSING."""
    sh = np.array(full)
    sh[~present] = MISSING
    return sh


def definition(k, m, sh, present, W):
    """(statuses, image): the oracle's reconstruction of every block under its own masks."""
    out = sh.copy()
    status = []
    for b in range(sh.shape[0]):
        if not W[b].any():
            status.append(0)
        elif present[b].sum() < k:
            status.append(TOO_FEW)
        else:
            rc, rec = orc.reconstruct(k, m, sh[b], present[b].tolist(), False)
            assert rc == 0
            out[b, W[b]] = rec[W[b]]
            status.append(0)
    return status, out


def same_bytes(got, want, ctx):
    if not np.array_equal(got, want):
        at = np.flatnonzero(got != want)
        raise AssertionError("%r: %d bytes differ, first at offset %d: got %#x, want %#x" %
                             (ctx, at.size, at[0], got[at[0]], want[at[0]]))


def u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


def check(torch, c, lay, sh, present, required, data_only, label, status=True):
    """One rsmi_reconstruct_mixed_batch_dev over sh (nb, n, S) laid out by lay: the statuses, the
    whole buffer and the label against the definition.  Returns the image."""
    k, m = lay.k, lay.m
    W = wanted(k, present, required, data_only)
    want_status, image = definition(k, m, sh, present, W)
    host = lay.fill(sh)
    d = torch.from_numpy(host.copy()).cuda()
    assert d.data_ptr() % 256 == 0
    got = c.reconstruct_mixed_batch_dev(d.data_ptr() + lay.off, lay.rs, lay.bs, lay.S, lay.nb, u8(present),
                                        None if required is None else u8(required), data_only,
                                        torch.cuda.current_stream().cuda_stream, status)
    torch.cuda.synchronize()
    ctx = (k, m, lay.S, lay.aligned, data_only)
    if status:
        assert got == want_status, (ctx, got, want_status)
    if label is not None:
        assert c.last_kernel() == label, (ctx, c.last_kernel(), label)
    expect = host.copy()
    lay.rows(expect)[:] = image
    same_bytes(d.cpu().numpy(), expect, ctx)
    return image


def junk_unused_survivor(k, sh, present):
    """The first-k-present rule: a present row behind the first k present ones is not a survivor,
    so what it holds must not matter.  Such a row gets junk where a block has one (the oracle
    reads the same shards, and ignores it the same way)."""
    for b in range(sh.shape[0]):
        rows = np.flatnonzero(present[b])
        if rows.size > k:
            sh[b, rows[-1]] ^= 0x3C


# ---------------------------------------------------------------- 0: the chunk rule matches the source
def host_chunk_blocks(n, S):
    """Blocks per chunk of the mixed host pipeline: whole blocks at pitch S.  Restated here on
    purpose; the CPU leg pins it to the source."""
    return max(1, (64 << 20) // (n * S))


def test_chunk_rule_matches_source():
    with open(MIXED_CPP) as f:
        src = f.read()
    assert src.count("(size_t(64) << 20)") == 1
    assert "const size_t n = size_t(c->n), blk = n * S;" in src
    assert "const size_t chunk = std::max<size_t>(1, (size_t(64) << 20) / blk);" in src
    assert src.count("const int ns = nblocks > chunk ? 3 : 1;") == 1
    assert src.count("Staging& st = c->staging[i % ns];") == 1
    assert re.findall(r"map\.size\(\)\s*>=\s*(\d+)", src) == ["32"]
    assert "size_t(1) << 20" in src  # the scratch's first size, which leg 6 outgrows
    kept = int(re.findall(r"map\.size\(\)\s*>=\s*(\d+)", src)[0])
    assert PAST_STREAMS == 40 > kept  # leg 12 stays beyond the eviction threshold
    # leg 11: a segment of launch_mixed is at most 2^22 blocks
    assert src.count("uint64_t(1) << 22") == 1 and SEAM == 1 << 22
    assert ("const uint64_t seg = std::min<uint64_t>(std::max<uint64_t>(1, uint64_t(c->opt_launch_units_max) / tpb), "
            "uint64_t(1) << 22);") in " ".join(src.split())
    assert src.count("const uint64_t seg =") == 1 and "<< 31" not in src
    # leg 11 runs one tile per block, where the option's default (2^24 - 1 tiles) is the larger arm
    with open(os.path.join(os.path.dirname(MIXED_CPP), "rsmi_impl.hpp")) as f:
        assert "constexpr uint64_t kLaunchUnitsDefault = (uint64_t(1) << 24) - 1;" in f.read()
    assert "uint8_t* sbase = base + (s0 - b0) * bs;" in src
    assert "list[cls[p]].push_back(MixedEntry{uint32_t(b), p});" in src


# ---------------------------------------------------------------- 1: RS(4,2), every pattern in one call
def rs42_losses():
    """6 one-lost and 15 two-lost patterns alternating (so neighbours differ in class as well),
    an intact block and a block with 3 rows lost."""
    one = [(i,) for i in range(6)]
    two = list(itertools.combinations(range(6), 2))
    out = []
    for i in range(15):
        out.append(two[i])
        if i < 6:
            out.append(one[i])
        if i == 7:
            out.append(())
        if i == 11:
            out.append((0, 2, 5))
    assert len(out) == 23
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("data_only", [False, True], ids=["all", "data_only"])
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "ua"])
def test_rs42_every_pattern_in_one_call(gpu, aligned, data_only):
    torch, rsmi = gpu
    k, m = 4, 2
    losses = rs42_losses()
    present = present_of(6, losses)
    with rsmi.Codec(k, m) as c:
        for S in SIZES:
            lay = layout(rsmi, k, m, S, len(losses), aligned)
            sh = stored(stripes(k, m, S, len(losses)), present)
            junk_unused_survivor(k, sh, present)
            check(torch, c, lay, sh, present, None, data_only, mixed_label(4, 2, aligned))


# ---------------------------------------------------------------- 2: RS(10,4), classes interleaved
def rs104_losses(nb, seed):
    """Block b loses b % 4 + 1 rows drawn over data and parity: the classes alternate block by block."""
    rng = np.random.default_rng(seed)
    return [tuple(sorted(rng.choice(14, size=b % 4 + 1, replace=False).tolist())) for b in range(nb)]


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "ua"])
def test_rs104_interleaved_classes(gpu, aligned):
    torch, rsmi = gpu
    k, m, S, nb = 10, 4, 3000, 64
    losses = rs104_losses(nb, 20)
    present = present_of(14, losses)
    assert len(set(losses)) > 40
    sh = stored(stripes(k, m, S, nb), present)
    junk_unused_survivor(k, sh, present)
    lay = layout(rsmi, k, m, S, nb, aligned)
    with rsmi.Codec(k, m) as c:
        check(torch, c, lay, sh, present, None, False, mixed_label(10, 4, aligned))
        # data_only: a block that lost parity only has nothing to rebuild, the others change class
        W = wanted(k, present, None, True)
        check(torch, c, lay, sh, present, None, True, mixed_label(10, int(W.sum(axis=1).max()), aligned))
        # per-block required masks: a subset of the missing rows (some empty), present rows named too
        rng = np.random.default_rng(21)
        required = rng.integers(0, 2, size=(nb, 14)).astype(bool)
        required[5] = False
        W = wanted(k, present, required, False)
        assert set(W.sum(axis=1).tolist()) >= {0, 1, 2, 3}
        check(torch, c, lay, sh, present, required, False, mixed_label(10, int(W.sum(axis=1).max()), aligned))


# ---------------------------------------------------------------- 3: too few without statuses; nothing to do
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "ua"])
def test_too_few_without_statuses_and_intact_batch(gpu, aligned):
    torch, rsmi = gpu
    k, m, S, nb = 4, 2, 1030, 5
    lay = layout(rsmi, k, m, S, nb, aligned)
    full = stripes(k, m, S, nb)
    stream = torch.cuda.current_stream().cuda_stream
    with rsmi.Codec(k, m) as c:
        present = present_of(6, [(0,), (1, 4), (0, 1, 2), (5,), ()])
        sh = stored(full, present)
        host = lay.fill(sh)
        d = torch.from_numpy(host.copy()).cuda()
        with pytest.raises(rsmi.RsmiError) as e:
            c.reconstruct_mixed_batch_dev(d.data_ptr() + lay.off, lay.rs, lay.bs, S, nb, u8(present), None, False,
                                          stream, status=False)
        assert e.value.code == TOO_FEW
        torch.cuda.synchronize()
        same_bytes(d.cpu().numpy(), host, "nothing is written")
        assert c.last_kernel() == ""
        # with statuses the same batch goes through
        check(torch, c, lay, sh, present, None, False, mixed_label(4, 2, aligned))
        # all intact: OK, no launch; the marker launch's label stays
        host = lay.fill(np.array(full))
        d = torch.from_numpy(host.copy()).cuda()
        base = d.data_ptr() + lay.off
        c.encode_batch_dev(base, lay.rs, lay.bs, base + k * lay.rs, lay.rs, lay.bs, S, nb, stream)
        marker = c.last_kernel()
        assert marker.startswith("rs_fast_kernel<K=4,MT=2")
        for status in (True, False):
            got = c.reconstruct_mixed_batch_dev(base, lay.rs, lay.bs, S, nb, np.ones((nb, 6), dtype=np.uint8), None,
                                                False, stream, status)
            assert got == ([0] * nb if status else None)
        torch.cuda.synchronize()
        assert c.last_kernel() == marker
        same_bytes(d.cpu().numpy(), host, "an intact batch")


# ---------------------------------------------------------------- 4: the strided walk
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "ua"])
@pytest.mark.parametrize("nb", [40, 1280])
def test_waves_per_cu_1(gpu, nb, aligned):
    """waves_per_cu = 1 caps a launch at one wave per CU.  40 blocks of 2 tiles; and 1280 blocks,
    640 tiles per class, more than a 256-CU device has such waves: a wave goes on to tiles of
    other blocks with other patterns and restages its tables.  The 1280 blocks repeat 40 stripes,
    each time under another pattern."""
    torch, rsmi = gpu
    k, m, S = 10, 4, 1030
    losses = rs104_losses(nb, 40 + nb)
    present = present_of(14, losses)
    base = stripes(k, m, S, 40)
    sh = stored(np.concatenate([base] * (nb // 40)), present)
    lay = layout(rsmi, k, m, S, nb, aligned)
    with rsmi.Codec(k, m) as c:
        c.set_option("waves_per_cu", 1)
        check(torch, c, lay, sh, present, None, False, mixed_label(10, 4, aligned))


# ---------------------------------------------------------------- 5: the fallback beside fast blocks
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "ua"])
def test_fallback_beside_fast_blocks(gpu, aligned):
    torch, rsmi = gpu
    S = 1030
    # RS(5,5): 5 rows lost is a two-tile plan (4 + 1 rows) and takes launch_plan; 1 lost is a class
    k, m = 5, 5
    losses = [(0,), (0, 1, 2, 3, 4), (7,), (0, 2, 4, 6, 8), (0, 2, 4, 6, 8), (3,), (1, 2, 3, 8, 9), (2, 6)]
    present = present_of(10, losses)
    sh = stored(stripes(k, m, S, len(losses)), present)
    lay = layout(rsmi, k, m, S, len(losses), aligned)
    with rsmi.Codec(k, m) as c:
        # the fallback's runs come behind the classes: the last launch is the last run's second tile
        check(torch, c, lay, sh, present, None, False, fast_label(5, 1, ua=not aligned))
    # K without an rs_mixed_kernel: every block takes launch_plan, one launch per run of equal masks
    for k, m in ((7, 3), (20, 4)):
        n = k + m
        losses = [(0,), (0,), (1, n - 1), (2,), (0, 1, k), (0, 1, k), (), (k - 1, k)]
        present = present_of(n, losses)
        sh = stored(stripes(k, m, S, len(losses)), present)
        lay = layout(rsmi, k, m, S, len(losses), aligned)
        with rsmi.Codec(k, m) as c:
            check(torch, c, lay, sh, present, None, False, generic_label(k, 2))
            check(torch, c, lay, sh, present, None, True, generic_label(k, 1))


@pytest.mark.gpu
def test_fallback_unaligned_short_rows(gpu):
    """Unaligned rows shorter than 16 bytes are neither aligned nor UA: the byte-granular kernel."""
    torch, rsmi = gpu
    k, m, S = 4, 2, 8
    losses = rs42_losses()
    present = present_of(6, losses)
    sh = stored(stripes(k, m, S, len(losses)), present)
    with rsmi.Codec(k, m) as c:
        check(torch, c, layout(rsmi, k, m, S, len(losses), False), sh, present, None, False, generic_label(4, 2))
        # the same rows aligned have a class
        check(torch, c, layout(rsmi, k, m, S, len(losses), True), sh, present, None, False, mixed_label(4, 2, True))


# ---------------------------------------------------------------- 6: the scratch grows and starts over
@pytest.mark.gpu
def test_scratch_regrow_and_streams(gpu):
    """One context: a small call, then one whose lists outgrow the scratch's first size (1 MiB:
    more than 131072 blocks) on the same stream, the same again (it no longer fits behind the
    first: the scratch starts over), a small one, then calls on three more streams.  RS(10,4),
    S = 16, classes 1..4 in every call; the large batch repeats a 48-block period, so its image is
    the period's, tiled."""
    torch, rsmi = gpu
    k, m, S = 10, 4, 16
    period = rs104_losses(48, 60)
    reps = 3000
    big = reps * len(period)
    P = present_of(14, period)
    base = stored(stripes(k, m, S, len(period)), P)
    want_status = definition(k, m, base, P, wanted(k, P, None, False))[0]
    # the list words of the large call alone (8 bytes per block with rows to rebuild) outgrow the
    # first size, and a second such call does not fit behind the first: it starts over
    fast_blocks = reps * sum(1 for lost in period if 0 < len(lost) <= m)
    assert (1 << 20) < fast_blocks * 8 < (3 << 19) < 2 * fast_blocks * 8
    with rsmi.Codec(k, m) as c:
        lay = layout(rsmi, k, m, S, len(period), True)
        image = check(torch, c, lay, base, P, None, False, mixed_label(10, 4, True))
        lay_big = layout(rsmi, k, m, S, big, True)
        host = lay_big.fill(np.concatenate([base] * reps))
        expect = host.copy()
        lay_big.rows(expect)[:] = np.concatenate([image] * reps)
        masks = u8(np.concatenate([P] * reps))
        for _ in range(2):
            d = torch.from_numpy(host).cuda()
            got = c.reconstruct_mixed_batch_dev(d.data_ptr(), lay_big.rs, lay_big.bs, S, big, masks, None, False,
                                                torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert got == want_status * reps
            same_bytes(d.cpu().numpy(), expect, "the large batch")
            del d
        check(torch, c, lay, base, P, None, False, mixed_label(10, 4, True))
        for _ in range(3):
            with torch.cuda.stream(torch.cuda.Stream()):
                for aligned in (True, False):
                    check(torch, c, layout(rsmi, k, m, 1030, len(period), aligned),
                          stored(stripes(k, m, 1030, len(period)), P), P, None, False, mixed_label(10, 4, aligned))


# ---------------------------------------------------------------- 7: stream order
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "ua"])
def test_stream_order_back_to_back(gpu, aligned):
    """Behind a gate on a side stream: two mixed calls with different masks on two buffers, each
    call's mask arrays overwritten with garbage as soon as it returns, then an encode on that
    stream that reads the first buffer's rebuilt data rows.  No host sync before the end."""
    torch, rsmi = gpu
    gate = Gate(torch)
    k, m, S, nb = 10, 4, 1030, 24
    full = stripes(k, m, S, nb)
    lay = layout(rsmi, k, m, S, nb, aligned)
    PA = present_of(14, rs104_losses(nb, 70))
    PB = present_of(14, rs104_losses(nb, 71)[::-1])
    RB = np.random.default_rng(72).integers(0, 2, size=(nb, 14)).astype(bool)
    shA, shB = stored(full, PA), stored(full, PB)
    stA, imgA = definition(k, m, shA, PA, wanted(k, PA, None, False))
    stB, imgB = definition(k, m, shB, PB, wanted(k, PB, RB, False))
    hostA, hostB = lay.fill(shA), lay.fill(shB)
    with rsmi.Codec(k, m) as c:
        dA, dB = torch.from_numpy(hostA.copy()).cuda(), torch.from_numpy(hostB.copy()).cuda()
        par = torch.full((nb * m * S,), 0xEE, dtype=torch.uint8, device="cuda")
        # the plans of both calls exist before the gate closes (building one copies synchronously)
        warm = torch.from_numpy(hostA.copy()).cuda()
        for P_, R_ in ((PA, None), (PB, RB)):
            c.reconstruct_mixed_batch_dev(warm.data_ptr() + lay.off, lay.rs, lay.bs, S, nb, u8(P_),
                                          None if R_ is None else u8(R_), False, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        masks = [u8(PA), u8(PB), u8(RB)]
        with torch.cuda.stream(side):
            gate()
            h = side.cuda_stream
            gotA = c.reconstruct_mixed_batch_dev(dA.data_ptr() + lay.off, lay.rs, lay.bs, S, nb, masks[0].ctypes.data,
                                                 None, False, h)
            masks[0][:] = 0xA5
            gotB = c.reconstruct_mixed_batch_dev(dB.data_ptr() + lay.off, lay.rs, lay.bs, S, nb, masks[1].ctypes.data,
                                                 masks[2].ctypes.data, False, h)
            masks[1][:] = 0
            masks[2][:] = 0xFF
            base = dA.data_ptr() + lay.off
            c.encode_batch_dev(base, lay.rs, lay.bs, par.data_ptr(), S, m * S, S, nb, h)
            assert not side.query(), "the gate opened before the calls were queued: nothing was ordered"
        torch.cuda.synchronize()
    assert gotA == stA and gotB == stB
    for d, host, img, tag in ((dA, hostA, imgA, "first"), (dB, hostB, imgB, "second")):
        expect = host.copy()
        lay.rows(expect)[:] = img
        same_bytes(d.cpu().numpy(), expect, tag)
    # data rows rebuilt by the first call are the originals, so the encode gives the stored parity
    assert (np.flatnonzero(~PA[:, :k].all(axis=1)).size > 0)
    want_par = np.stack([orc.encode(k, m, np.ascontiguousarray(imgA[b, :k])) for b in range(nb)])
    same_bytes(par.cpu().numpy(), want_par.reshape(-1), "the encode behind the calls")


# ---------------------------------------------------------------- 8: the uniform call; far offsets
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "ua"])
@pytest.mark.parametrize("k,m,lost,req", [(10, 4, (3,), None), (10, 4, (0, 5, 11, 13), (5, 13)), (4, 2, (1, 4), None),
                                          (16, 4, (0, 15, 17), None)])
def test_equals_the_uniform_call(gpu, k, m, lost, req, aligned):
    """One pattern for all blocks: the buffer equals rsmi_reconstruct_rows_batch_dev's byte for
    byte, padding and gaps included."""
    torch, rsmi = gpu
    n, S, nb = k + m, 3000, 9
    present = present_of(n, [lost] * nb)
    required = np.zeros((nb, n), dtype=bool)
    required[:, list(req if req is not None else lost)] = True
    lay = layout(rsmi, k, m, S, nb, aligned)
    host = lay.fill(stored(stripes(k, m, S, nb), present))
    stream = torch.cuda.current_stream().cuda_stream
    with rsmi.Codec(k, m) as c:
        d1, d2 = torch.from_numpy(host.copy()).cuda(), torch.from_numpy(host.copy()).cuda()
        c.reconstruct_rows_batch_dev(d1.data_ptr() + lay.off, lay.rs, lay.bs, S, nb, present[0].tolist(),
                                     required[0].tolist(), stream)
        assert c.reconstruct_mixed_batch_dev(d2.data_ptr() + lay.off, lay.rs, lay.bs, S, nb, u8(present), u8(required),
                                             False, stream) == [0] * nb
        torch.cuda.synchronize()
        assert c.last_kernel() == mixed_label(k, int(required[0].sum()), aligned)
        same_bytes(d2.cpu().numpy(), d1.cpu().numpy(), (k, m, lost, aligned))
        assert not np.array_equal(d1.cpu().numpy(), host)


@pytest.mark.gpu
def test_offsets_past_4gib(gpu):
    """Two blocks a block stride of 4 GiB + 4096 apart, each with its own pattern, aligned and
    shifted by one byte.  A row or block offset truncated to 32 bits would land in the near block."""
    torch, rsmi = gpu
    if torch.cuda.mem_get_info()[0] < 8 << 30:
        pytest.skip("needs 8 GiB of free device memory")
    k, m, S, nb = 4, 2, 1040, 2
    bs = 2 ** 32 + 4096
    full = stripes(k, m, S, nb)
    present = present_of(6, [(1,), (0, 5)])
    sh = stored(full, present)
    try:
        with rsmi.Codec(k, m) as c:
            d = torch.empty(2 ** 32 + 2 ** 20, dtype=torch.uint8, device="cuda")
            assert 1 + bs + (k + m) * S <= d.numel()
            for off in (0, 1):
                for b in range(nb):
                    for i in range(k + m):
                        o = off + b * bs + i * S
                        d[o:o + S].copy_(torch.from_numpy(sh[b, i]))
                got = c.reconstruct_mixed_batch_dev(d.data_ptr() + off, S, bs, S, nb, u8(present), None, False,
                                                    torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                assert got == [0, 0] and c.last_kernel() == mixed_label(4, 2, off == 0)
                for b in range(nb):
                    for i in range(k + m):
                        o = off + b * bs + i * S
                        assert np.array_equal(d[o:o + S].cpu().numpy(), full[b, i]), (off, b, i)
            del d
    finally:
        torch.cuda.empty_cache()


# ---------------------------------------------------------------- 9: the host entry
def host_case(rsmi, c, buf_of, k, m, S, sh, present, required, data_only, bs=None):
    """rsmi_reconstruct_mixed_batch_host over sh laid out at pitch S, block stride bs, in the
    buffer buf_of(nbytes) returns (a numpy view): statuses and the whole buffer."""
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
    got = c.reconstruct_mixed_batch_host_ptr(buf.ctypes.data, bs, S, nb, u8(present),
                                             None if required is None else u8(required), data_only)
    assert got == want_status
    same_bytes(buf, expect, (k, m, S, nb, bs))


@pytest.mark.gpu
def test_host_page_locked_and_small(gpu):
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
            for S in (1030, 3000, 16):
                nb = 24
                losses = rs104_losses(nb - 2, S) + [(0, 1, 2, 3, 4), ()]
                present = present_of(14, losses)
                sh = stored(stripes(k, m, S, nb), present)
                req = np.random.default_rng(S).integers(0, 2, size=(nb, 14)).astype(bool)
                for buf_of in (pinned, pageable):
                    host_case(rsmi, c, buf_of, k, m, S, sh, present, None, False)
                    assert c.last_kernel().startswith("rs_mixed_kernel<K=10,MT=4>")
                    host_case(rsmi, c, buf_of, k, m, S, sh, present, req, False, bs=14 * S + 5)
                    host_case(rsmi, c, buf_of, k, m, S, sh[:1], present[:1], None, True)
            # the small-call limit off: the same pageable call takes the upload path, as one chunk
            c.set_option("small_call_bytes", 0)
            for S in (1030, 1040):
                host_case(rsmi, c, pageable, k, m, S, stored(stripes(k, m, S, nb), present), present, None, False)
                host_case(rsmi, c, pageable, k, m, S, stored(stripes(k, m, S, nb), present), present, None, False,
                          bs=14 * S + 3)
    finally:
        for p in held:
            L.rsmi_host_free(p)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [2049, 2056])
def test_host_upload_past_one_chunk(gpu, S):
    """Pageable shards, four chunks with a short last one over the three staging slots (slot 0
    serves chunks 0 and 3).  Every block has its own pattern; blocks next to every seam and every
    97th are compared with the oracle, and in every block nothing but the wanted rows of blocks
    with status OK may change.  A too-few block sits in the last chunk."""
    torch, rsmi = gpu
    k, m = 4, 2
    n = k + m
    ch = host_chunk_blocks(n, S)
    nb = 3 * ch + 5
    assert -(-nb // ch) == 4 and nb * n * S > 2 << 20
    sample = sorted({0, nb - 1} | set(range(0, nb, 97)) |
                    {b for s in range(ch, nb, ch) for b in (s - 2, s - 1, s, s + 1)})
    pats = [lost for lost in rs42_losses() if len(lost) <= m]  # the 21 loss patterns and the intact block
    assert len(pats) == 22
    present = present_of(n, [pats[(b * 7 + b // ch) % 22] for b in range(nb)])
    present[nb - 2] = [True, False, False, False, True, True]  # too few, in the last chunk
    base = stripes(k, m, S, 64)
    sh = np.empty((nb, n, S), dtype=np.uint8)
    for b0 in range(0, nb, 64):
        sh[b0:b0 + 64] = base[:min(64, nb - b0)]
    sh[~present] = MISSING
    W = wanted(k, present, None, False)
    W[nb - 2] = False
    before = sh.copy()
    buf = sh.reshape(-1)
    with rsmi.Codec(k, m) as c:
        got = c.reconstruct_mixed_batch_host_ptr(buf.ctypes.data, n * S, S, nb, u8(present), None, False)
    assert got == [0] * (nb - 2) + [TOO_FEW, 0]
    assert np.array_equal(sh[~W], before[~W]), "a row that was not to be rebuilt changed"
    _, image = definition(k, m, before[sample], present[sample], W[sample])
    same_bytes(sh[sample], image, (S, "sampled blocks"))
    # the stripes repeat every 64 blocks: every rebuilt row against the stripe it belongs to
    for b0 in range(0, nb, 64):
        e = min(64, nb - b0)
        assert np.array_equal(sh[b0:b0 + e][W[b0:b0 + e]], base[:e][W[b0:b0 + e]]), b0


# ---------------------------------------------------------------- 10: no side effects; the Python mirror
@pytest.mark.gpu
def test_no_side_effects_on_other_calls(gpu):
    torch, rsmi = gpu
    k, m, S, nb = 10, 4, 1030, 8
    full = np.array(stripes(k, m, S, nb))
    lay = layout(rsmi, k, m, S, nb, True)
    present = present_of(14, rs104_losses(nb, 5))
    stream = torch.cuda.current_stream().cuda_stream
    with rsmi.Codec(k, m) as c:
        check(torch, c, lay, stored(full, present), present, None, False, mixed_label(10, 4, True))
        host = lay.fill(full)
        # encode
        d = torch.from_numpy(lay.fill(stored(full, present_of(14, [tuple(range(10, 14))] * nb)))).cuda()
        dd = d.data_ptr()
        c.encode_batch_dev(dd, lay.rs, lay.bs, dd + k * lay.rs, lay.rs, lay.bs, S, nb, stream)
        torch.cuda.synchronize()
        assert c.last_kernel() == fast_label(10, 4)
        same_bytes(d.cpu().numpy(), host, "encode")
        # uniform reconstruct
        d.view(-1)[:] = torch.from_numpy(lay.fill(stored(full, present_of(14, [(2,)] * nb))))
        c.reconstruct_batch_dev(dd, lay.rs, lay.bs, S, nb, [i != 2 for i in range(14)], True, stream)
        torch.cuda.synchronize()
        assert c.last_kernel() == fast_label(10, 1)
        same_bytes(d.cpu().numpy(), host, "reconstruct")
        # verify
        bad = torch.full((nb * m,), POISON, dtype=torch.int32, device="cuda")
        c.verify_batch_dev(dd, lay.rs, lay.bs, dd + k * lay.rs, lay.rs, lay.bs, S, nb, bad.data_ptr(), stream)
        torch.cuda.synchronize()
        assert c.last_kernel() == "rs_verify_kernel<K=10,MT=4>" and not bad.cpu().numpy().any()
        # heal
        dmg = full.copy()
        dmg[3, 7, 100] ^= 0x55
        d.view(-1)[:] = torch.from_numpy(lay.fill(dmg))
        cul = torch.full((nb,), POISON, dtype=torch.int32, device="cuda")
        c.heal_batch_dev(dd, lay.rs, lay.bs, dd + k * lay.rs, lay.rs, lay.bs, S, nb, cul.data_ptr(), 0, stream)
        torch.cuda.synchronize()
        assert c.last_kernel() == "rs_heal_kernel<K=10,MT=4>"
        assert cul.cpu().numpy().tolist() == [-1, -1, -1, 7, -1, -1, -1, -1]
        same_bytes(d.cpu().numpy(), host, "heal")
        # and the mixed call once more
        check(torch, c, lay, stored(full, present), present, None, False, mixed_label(10, 4, True))


@pytest.mark.gpu
def test_decode_data_blocks_many(gpu):
    torch, rsmi = gpu
    k, m = 4, 2
    e = rsmi.NewErasure(k, m, 4099)
    blocks = [bytes(np.random.default_rng(b).integers(0, 256, size=4099, dtype=np.uint8)) for b in range(5)]
    shards = [e.encode_data(b) for b in blocks]
    lossy = [list(s) for s in shards]
    for b, lost in enumerate([(0,), (1, 3), (), (4, 5), (2, 5)]):
        for i in lost:
            lossy[b][i] = None
    e.decode_data_blocks_many(lossy)
    for b in range(5):
        assert lossy[b][:k] == shards[b][:k], b
    assert lossy[3][4] is None and lossy[4][5] is None  # parity is not rebuilt, as DecodeDataBlocks
    one = [list(s) for s in shards]
    one[1][0] = None
    e.decode_data_blocks(one[1])
    assert one[1] == shards[1]


# ---------------------------------------------------------------- 11: the segment seam
def seam_period():
    """13 blocks of RS(2,2): the 4 one-lost and the 6 two-lost patterns with the classes
    alternating, an intact block, a three-lost (too few) block and one two-lost pattern again.
    13 does not divide 2^22, so the seam cuts the period."""
    one = [(i,) for i in range(4)]
    two = list(itertools.combinations(range(4), 2))
    out = [two[0], one[0], two[1], one[1], (), two[2], one[2], two[3], (0, 1, 2), one[3], two[4], two[5], two[2]]
    assert len(out) == 13 and len(set(out)) == 12 and SEAM % 13 != 0
    return out


def tiled_blocks(per_period, nb):
    """per_period[b % period] for b in range(nb), along the first axis."""
    p = per_period.shape[0]
    return np.tile(per_period, (-(-nb // p),) + (1,) * (per_period.ndim - 1))[:nb]


def seam_run(torch, c, off, rs, bs, S, sh, present, want_status, image, label, ctx):
    """One call over nb = sh.shape[0] blocks at pitch rs, block stride bs, off bytes behind a
    256-byte-aligned base, 64 guard bytes behind the last block: statuses, label, whole buffer."""
    nb, n = sh.shape[0], sh.shape[1]

    def render(rows):
        buf = np.full(off + nb * bs + 64, GAP, dtype=np.uint8)
        np.lib.stride_tricks.as_strided(buf[off:], shape=(nb, n, S), strides=(bs, rs, 1))[:] = rows
        return buf

    d = torch.from_numpy(render(sh)).cuda()
    assert d.data_ptr() % 256 == 0
    got = c.reconstruct_mixed_batch_dev(d.data_ptr() + off, rs, bs, S, nb, u8(present), None, False,
                                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert c.last_kernel() == label, (ctx, c.last_kernel(), label)
    assert np.array_equal(np.asarray(got, dtype=np.int32), want_status), ctx
    out = d.cpu().numpy()
    del d
    same_bytes(out, render(image), ctx)


@pytest.mark.gpu
def test_segment_seam_fast_classes(gpu):
    """2^22 + 5 blocks of RS(2,2), S = 16, rows at pitch 16: two segments, the second of 5 blocks.
    Its base is sbase, its entries' blk count from the seam, its lists are the call's second
    request to the stream's scratch.  The image is the period's definition, tiled."""
    from test_mixed_layouts import expected_label, rows_rebuilt

    torch, rsmi = gpu
    k, m, S, nb = 2, 2, 16, SEAM + 5
    period = seam_period()
    P = present_of(4, period)
    base = stored(stripes(k, m, S, 13), P)
    W = wanted(k, P, None, False)
    status, image = definition(k, m, base, P, W)
    assert sorted(set(status)) == [0, TOO_FEW]
    rows = tiled_blocks(rows_rebuilt(k, P, W), nb)
    seam = [period[b % 13] for b in range(SEAM - 2, SEAM + 3)]
    assert len(set(seam)) >= 3 and {1, 2} <= set(rows[SEAM - 2:SEAM + 3].tolist())
    assert {1, 2} <= set(rows[SEAM:].tolist())
    label = expected_label(k, rows, "aligned")
    assert label == mixed_label(2, 2, True)
    try:
        with rsmi.Codec(k, m) as c:
            seam_run(torch, c, 64, S, 4 * S, S, tiled_blocks(base, nb), tiled_blocks(P, nb),
                     tiled_blocks(np.asarray(status, dtype=np.int32), nb), tiled_blocks(image, nb), label,
                     "fast classes")
    finally:
        torch.cuda.empty_cache()


@pytest.mark.gpu
def test_segment_seam_cuts_a_fallback_run(gpu):
    """RS(2,2), S = 8, rows at pitch 8 from an odd base: neither form, every block takes
    launch_plan.  One pattern everywhere except blocks [2^22 - 1, 2^22 + 1), a run that the seam
    cuts into two launches, and the batch's first block."""
    from test_mixed_layouts import expected_label, rows_rebuilt

    torch, rsmi = gpu
    k, m, S, nb = 2, 2, 8, SEAM + 5
    pats = [(0,), (1, 3), (0, 1)]
    pid = np.zeros(nb, dtype=np.intp)
    pid[SEAM - 1:SEAM + 1] = 1
    pid[0] = 2
    full = stripes(k, m, S, 13)
    sh3, img3, rows3 = [], [], []
    for lost in pats:
        P = present_of(4, [lost] * 13)
        sh = stored(full, P)
        W = wanted(k, P, None, False)
        status, image = definition(k, m, sh, P, W)
        assert status == [0] * 13
        sh3.append(sh)
        img3.append(image)
        rows3.append(rows_rebuilt(k, P, W)[0])
    at = np.arange(nb) % 13
    present = present_of(4, pats)[pid]
    rows = np.asarray(rows3)[pid]
    label = expected_label(k, rows, "generic")
    assert label == generic_label(2, 1) and rows[SEAM] == 2
    try:
        with rsmi.Codec(k, m) as c:
            seam_run(torch, c, 65, S, 4 * S, S, np.stack(sh3)[pid, at], present, np.zeros(nb, dtype=np.int32),
                     np.stack(img3)[pid, at], label, "fallback run")
    finally:
        torch.cuda.empty_cache()


# ---------------------------------------------------------------- 12: past 32 caller streams
@pytest.mark.gpu
def test_past_32_caller_streams(gpu):
    """One Codec(10, 4), one mixed call on each of 40 distinct streams (collected as
    test_stream_order's leg E collects them), then the same over the streams in reverse, with no
    host sync between the calls: mixed_scratch() drains the device and frees every stream's lists
    and their page-locked mirror on the way, twice.  No gate: a closed gate would never open
    behind the eviction's hipDeviceSynchronize.  All 80 buffers and statuses against the
    definition."""
    from test_stream_order import _hip_runtime

    torch, rsmi = gpu
    k, m, nb = 10, 4, 24
    streams, seen = [], set()

    def add(s):
        if s.cuda_stream not in seen:
            seen.add(s.cuda_stream)
            streams.append(s)

    add(torch.cuda.current_stream())
    add(torch.cuda.ExternalStream(0))
    for prio in (0, -1):
        for _ in range(64):
            add(torch.cuda.Stream(priority=prio))
    hip, own = None, []
    try:
        if len(streams) < PAST_STREAMS:
            hip = _hip_runtime()
            hip.hipStreamCreateWithFlags.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
            hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
            while len(streams) < PAST_STREAMS:
                h = ctypes.c_void_p()
                assert hip.hipStreamCreateWithFlags(ctypes.byref(h), 1) == 0  # hipStreamNonBlocking
                own.append(h)
                add(torch.cuda.ExternalStream(h.value))
        handles = [s.cuda_stream for s in streams[:PAST_STREAMS]]
        assert len(set(handles)) == PAST_STREAMS > 32 and 0 in handles
        variants = [(1030, True), (1030, False), (3000, True)]
        calls = []
        for j, i in enumerate(list(range(PAST_STREAMS)) + list(reversed(range(PAST_STREAMS)))):
            S, aligned = variants[i % 3]
            lay = layout(rsmi, k, m, S, nb, aligned)
            present = present_of(14, rs104_losses(nb, 1200 + j))
            sh = stored(stripes(k, m, S, nb), present)
            status, image = definition(k, m, sh, present, wanted(k, present, None, False))
            host = lay.fill(sh)
            expect = host.copy()
            lay.rows(expect)[:] = image
            d = torch.from_numpy(host).cuda()
            assert d.data_ptr() % 256 == 0
            calls.append((handles[i], lay, present, status, expect, d))
        assert len({tuple(map(tuple, c_[2])) for c_ in calls}) == len(calls)
        torch.cuda.synchronize()
        with rsmi.Codec(k, m) as c:
            got = [c.reconstruct_mixed_batch_dev(d.data_ptr() + lay.off, lay.rs, lay.bs, lay.S, nb, u8(present), None,
                                                 False, h)
                   for h, lay, present, _, _, d in calls]
            torch.cuda.synchronize()
            assert c.last_kernel() == mixed_label(10, 4, calls[-1][1].aligned)
        for j, (h, lay, present, status, expect, d) in enumerate(calls):
            assert got[j] == status, j
            same_bytes(d.cpu().numpy(), expect, ("call", j, lay.S, lay.aligned))
    finally:
        torch.cuda.synchronize()
        for h in own:
            hip.hipStreamDestroy(h)


# ---------------------------------------------------------------- 13: the host upload, strided, with required
@pytest.mark.gpu
def test_host_upload_strided_with_required(gpu):
    """Pageable shards with 5 bytes between the blocks, three chunks over the three staging slots
    (the per-block upload branch), a seeded required mask per block, a too-few block in the last
    chunk.  The whole buffer is compared: rebuilt rows are the stripe's own, everything else (the
    gap bytes' sentinel included) comes back unchanged; blocks next to every seam and every 97th
    are also compared with the oracle under their masks."""
    torch, rsmi = gpu
    k, m, S = 4, 2, 2049
    n = k + m
    ch = host_chunk_blocks(n, S)
    nb = 2 * ch + 3
    bs = n * S + 5
    assert -(-nb // ch) == 3 and nb * n * S > 2 << 20
    sample = sorted({0, nb - 1, nb - 2} | set(range(0, nb, 97)) |
                    {b for s in range(ch, nb, ch) for b in (s - 2, s - 1, s, s + 1)})
    pats = [lost for lost in rs42_losses() if len(lost) <= m]
    present = present_of(n, [pats[(b * 7 + b // ch) % 22] for b in range(nb)])
    present[nb - 2] = [True, False, False, False, True, True]  # too few, in the last chunk
    required = np.random.default_rng(1300).integers(0, 2, size=(nb, n)).astype(bool)
    required[nb - 2] = True
    W = wanted(k, present, required, False)
    assert (required & present).any() and (~required & ~present).any()
    assert {0, 1, 2} <= set(W.sum(axis=1).tolist())
    want_status = np.zeros(nb, dtype=np.int32)
    want_status[nb - 2] = TOO_FEW
    Wok = W.copy()
    Wok[nb - 2] = False
    base = stripes(k, m, S, 64)
    buf = np.full(nb * bs + 7, GAP, dtype=np.uint8)
    rows = np.lib.stride_tricks.as_strided(buf, shape=(nb, n, S), strides=(bs, S, 1))
    for b0 in range(0, nb, 64):
        rows[b0:b0 + 64] = base[:min(64, nb - b0)]
    expect = buf.copy()
    erows = np.lib.stride_tricks.as_strided(expect, shape=(nb, n, S), strides=(bs, S, 1))
    rows[~present] = MISSING
    erows[~present & ~Wok] = MISSING
    before = rows[sample]
    with rsmi.Codec(k, m) as c:
        got = c.reconstruct_mixed_batch_host_ptr(buf.ctypes.data, bs, S, nb, u8(present), u8(required), False)
        # every chunk is a launch_mixed of its own, on rows at pitch S: the label is the last chunk's
        last = Wok[2 * ch:].sum(axis=1)
        assert last.any() and c.last_kernel() == mixed_label(4, int(last.max()), False)
    assert np.array_equal(np.asarray(got, dtype=np.int32), want_status)
    status, image = definition(k, m, before, present[sample], W[sample])
    assert status == want_status[sample].tolist()
    same_bytes(rows[sample].reshape(-1), image.reshape(-1), "sampled blocks")
    same_bytes(buf, expect, "the whole buffer")
