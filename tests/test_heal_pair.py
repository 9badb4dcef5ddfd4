"""rsmi_heal_pair on the GPU against the definition, computed with the CPU oracle, exactly.

The verdict of a block is test_locate_pair.want_pair's: (-1, -1) clean, (x, -1) where the
definition of rsmi_locate names shard x, (x, y) where no single shard explains the stripe and
exactly one pair does, else (-2, -2).  The expected image of a block is the stored shards with the
rows its verdict names replaced by the oracle's reconstruction of them with those rows absent; of
any other block, the block unchanged.  Neither comes from the library.  The whole buffer is
compared byte for byte (the sentinels of test_verify.Lay in data padding, parity padding and gaps
included), the verdicts and flags against the definition and against rsmi_locate_pair_batch_dev
run on a copy of the input, the poisoned tails of the outputs, and the launch label.  There are no
tolerances.

  1  every pair, every single culprit and clean blocks in one call; three placements, both layouts
  2  the UA layout's last window overlapping the previous tile's, both rows damaged in the overlap
  3  blocks that must not be touched: three damaged shards, the ambiguous column at RS(6,3)
  4  imitation at RS(4,4): healed to a clean codeword that is not the original
  5  m <= 2: rsmi_heal's image, the verdicts widened
  6  shapes without an rs_heal_pair_kernel: rs_heal_pair_rows_kernel, past a scratch chunk
  7  scratch regrow; waves_per_cu = 1
  8  the image equals the old route's: locate pair, masks, mixed-batch reconstruct
  9  stream order, with no host sync between damage, heal and verify
 10  block offsets past 4 GiB
 11  host paths: page-locked rows in place, the small call, one block, the upload pipeline, mixed
     page-locked and pageable halves, Erasure.heal_pair
"""
import ctypes
import os

import numpy as np
import pytest

import oracle_lib as orc
from test_heal import label as heal_label
from test_heal import run_dev as heal_run_dev
from test_heal import same_bytes, verify_flags
from test_locate_pair import (CLEAN, TILE, UNKNOWN, all_pairs, check_matrix, fallback_case, gf_solve, imitation_rs44,
                              in_span, pair_label, want_pair, want_pairs)
from test_locate_pair import run_dev as locate_pair_run_dev
from test_stream_order import Gate
from test_verify import Lay, stripes, want_flags
from test_verify_matrix import SEAM_HIT, seam_stripes

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROWS = "rs_heal_pair_rows_kernel"
POISON = 0x5EED


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    rsmi = pytest.importorskip("rsmi")
    if not torch.cuda.is_available() or rsmi.device_count() == 0:
        pytest.skip("no GPU")
    assert (rsmi.LocateClean, rsmi.LocateUnknown) == (CLEAN, UNKNOWN)
    return torch, rsmi


def label(lay):
    """m <= 2 names no pair: the launches are rsmi_heal's."""
    if lay.m <= 2:
        return heal_label(lay)
    return "rs_heal_pair_kernel<K=%d,MT=%d>%s" % (lay.k, lay.m, "" if lay.aligned else ",UA")


def want_image(k, m, sh, verdicts):
    """The definition's image of shards sh (nb, n, S) under its verdicts (nb, 2): the named rows
    replaced by the oracle's reconstruct with those rows absent."""
    out = sh.copy()
    for b, v in enumerate(np.asarray(verdicts).reshape(-1, 2)):
        gone = [int(x) for x in v if x >= 0]
        if gone:
            rc, rec = orc.reconstruct(k, m, sh[b], [i not in gone for i in range(k + m)], False)
            assert rc == 0
            for x in gone:
                out[b, x] = rec[x]
    return out


def run_dev(torch, c, lay, host, lab, flags=True):
    """rsmi_heal_pair_batch_dev over host's bytes: (verdicts (nb, 2), flags as bool or None, the
    buffer after).  Both outputs start poisoned and only their first 2 nb (nb * m) entries may
    change."""
    d = torch.from_numpy(host.copy()).cuda()
    assert d.data_ptr() % 256 == 0
    out = torch.full((2 * lay.nb + 2,), POISON, dtype=torch.int32, device="cuda")
    bad = torch.full((lay.nb * lay.m + 2,), POISON, dtype=torch.int32, device="cuda")
    base = d.data_ptr() + lay.off
    c.heal_pair_batch_dev(base, lay.rs, lay.bs, base + lay.k * lay.rs, lay.rs, lay.bs, lay.S, lay.nb, out.data_ptr(),
                          bad.data_ptr() if flags else 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert c.last_kernel() == lab, (c.last_kernel(), lab)
    out, bad = out.cpu().numpy(), bad.cpu().numpy()
    assert (out[2 * lay.nb:] == POISON).all() and (bad[lay.nb * lay.m:] == POISON).all(), "wrote past its outputs"
    after = d.cpu().numpy()
    if not flags:
        assert (bad == POISON).all()
        return out[:2 * lay.nb].reshape(-1, 2), None, after
    return out[:2 * lay.nb].reshape(-1, 2), bad[:lay.nb * lay.m].reshape(lay.nb, lay.m) != 0, after


def locate_pair_label(lay, lab):
    """The label rsmi_locate_pair_batch_dev reports on the layout whose heal reports lab."""
    if lab == ROWS:
        return "rs_locate_pair_rows_kernel"
    return pair_label(lay)


def check(torch, c, lay, sh, lab, want=None, host=None, flags=True, against_locate=True):
    """Heal sh (nb, n, S) laid out by lay (host: the buffer, when it is not lay.fill(sh)): the
    verdicts and flags are the definition's for sh and rsmi_locate_pair_batch_dev's for a copy of
    the buffer, the buffer after is host with the rows replaced by the definition's image.
    Returns (verdicts, image)."""
    if want is None:
        want = want_pairs(lay.k, lay.m, sh)
    image = want_image(lay.k, lay.m, sh, want)
    host = lay.fill(sh) if host is None else host
    assert np.array_equal(lay.rows(host), sh)
    got, bad, after = run_dev(torch, c, lay, host, lab, flags)
    ctx = (lay.k, lay.m, lay.S, lay.aligned)
    assert np.array_equal(got, want), (ctx, got.tolist(), np.asarray(want).tolist())
    if flags:
        assert np.array_equal(bad, want_flags(lay.k, lay.m, sh)), ctx
    if against_locate:
        lgot, lbad = locate_pair_run_dev(torch, c, lay, host, locate_pair_label(lay, lab), flags=flags)
        assert np.array_equal(got, lgot), ctx
        assert not flags or np.array_equal(bad, lbad), ctx
    expect = host.copy()
    lay.rows(expect)[:] = image
    same_bytes(after, expect, ctx)
    return got, image


# ---------------------------------------------------------------- 1: every pair in one call
PLACES = ("column", "cross", "stale")
POS_1 = [0, 15, 16, -17, -16, -1]
_CASE1 = {}


def every_pair_stripes(k, m, S, place):
    """One block per pair, one per single culprit and two clean ones.  column: x and y damaged in
    one byte column; cross: x in the first tile (chunk), y in the row's last chunk, partial where
    S mod 16 != 0; stale: both rows random."""
    n = k + m
    pairs = all_pairs(n)
    rng = np.random.default_rng(2000 * k + 20 * m + len(place))
    sh = stripes(k, m, S, len(pairs) + n + 2).copy()
    last = (S - 1) // 16 * 16  # the first byte of the row's last chunk
    first = TILE if S > TILE else 16  # the bytes of the first tile, or of the first chunk of a one-tile row
    for b, (x, y) in enumerate(pairs):
        if place == "column":
            pos = (b * 37 + 5) % S
            sh[b, x, pos] ^= 1 + (b * 7) % 255
            sh[b, y, pos] ^= 1 + (b * 13 + 3) % 255
        elif place == "cross":
            sh[b, x, (b * 11) % first] ^= 1 << (b % 8)
            sh[b, y, last + b % (S - last)] ^= 0x80 >> (b % 8)
        else:
            sh[b, x] = rng.integers(0, 256, size=S, dtype=np.uint8)
            sh[b, y] = rng.integers(0, 256, size=S, dtype=np.uint8)
    for x in range(n):
        sh[len(pairs) + x, x, POS_1[x % len(POS_1)] % S] ^= 0x40
    return sh


def every_pair_case(k, m, S, place):
    """(shards, want, image), the definition computed once and shared by both layouts."""
    key = (k, m, S, place)
    if key not in _CASE1:
        n = k + m
        pairs = all_pairs(n)
        sh = every_pair_stripes(k, m, S, place)
        want = want_pairs(k, m, sh)
        assert want[len(pairs):].tolist() == [[x, CLEAN] for x in range(n)] + [[CLEAN, CLEAN]] * 2
        named = [b for b in range(len(pairs)) if want[b, 1] >= 0]
        assert all(want[b].tolist() == list(pairs[b]) for b in named)
        assert all(want[b].tolist() == [UNKNOWN, UNKNOWN] for b in range(len(pairs)) if b not in named)
        if m >= 4:  # the distance promises every pair; at m = 3 the definition decides
            assert len(named) == len(pairs)
        assert len(named) * 2 > len(pairs), (key, len(named))
        image = want_image(k, m, sh, want)
        full = stripes(k, m, S, sh.shape[0])
        for b in range(sh.shape[0]):  # one or two damaged shards, named: the original bytes
            assert np.array_equal(image[b], full[b] if want[b, 0] != UNKNOWN else sh[b]), (key, b)
        _CASE1[key] = (sh, want, image)
    return _CASE1[key]


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
@pytest.mark.parametrize("k,m,S,place", [(k, m, S, p) for k, m, S in ((10, 4, 1041), (6, 3, 1041), (16, 4, 48))
                                         for p in PLACES])
def test_every_pair(gpu, k, m, S, place, aligned):
    """All C(n,2) pairs of RS(10,4) (91), RS(6,3) (36) and RS(16,4) (190), every single culprit and
    two clean blocks in one call.  S = 1041: one full tile plus a tile of one whole chunk and one
    byte (split: an overlapping last window); S = 48: three chunks."""
    torch, rsmi = gpu
    sh, want, image = every_pair_case(k, m, S, place)
    lay = Lay(rsmi, k, m, S, sh.shape[0], aligned)
    with rsmi.Codec(k, m) as c:
        _, got_image = check(torch, c, lay, sh, label(lay), want)
        assert np.array_equal(got_image, image)
        assert not verify_flags(torch, c, lay, lay.fill(image))[want[:, 0] != UNKNOWN].any()


# ---------------------------------------------------------------- 2: UA overlap across waves
@pytest.mark.gpu
@pytest.mark.parametrize("wpc", [0, 1], ids=["one-tile-per-wave", "waves_per_cu-1"])
@pytest.mark.parametrize("k,m", [(10, 4), (6, 3)])
@pytest.mark.parametrize("r", [1, 15])
def test_ua_last_window_overlaps_previous_tile(gpu, r, k, m, wpc):
    """Split layout (rows at an odd base, pitch S), S = 2048 + r: chunk 128 is the only chunk of
    tile 2, its window [S - 16, S) overlaps chunk 127's [2032, 2048) of tile 1, which another wave
    holds.  Both rows of the pair are damaged over [S - 40, S), so both waves see both rows' damage
    in the bytes they share, and either may find one row healed already.  A byte loaded twice or
    a D with D [h_x h_y] != I would leave or restore damage there.  One pair of each kind, and a
    single culprit."""
    torch, rsmi = gpu
    S = 2048 + r
    assert (S + 15) // 16 == 129 and S - 16 < 2048
    cases = [(1, 4), (2, k), (3, k + 2), (k, k + 2), (k + 1, k + 2), (0, None)]
    nb = len(cases) + 1
    lay = Lay(rsmi, k, m, S, nb, False)
    assert lay.off % 2 == 1 and lay.rs == S
    full = stripes(k, m, S, nb)
    sh = full.copy()
    rng = np.random.default_rng(50 + r + k)
    for b, (x, y) in enumerate(cases):
        for row in (x, y):
            if row is not None:
                sh[b, row, S - 40:] ^= rng.integers(1, 256, size=40, dtype=np.uint8)
    want = want_pairs(k, m, sh)
    assert want.tolist() == [[x, CLEAN if y is None else y] for x, y in cases] + [[CLEAN, CLEAN]], want.tolist()
    with rsmi.Codec(k, m) as c:
        if wpc:
            c.set_option("waves_per_cu", wpc)
        _, image = check(torch, c, lay, sh, label(lay), want)
        assert np.array_equal(image, full)


# ---------------------------------------------------------------- 3: blocks that must not be touched
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
def test_unknown_blocks_are_not_touched(gpu, aligned):
    """RS(10,4): healed blocks mixed with blocks of three damaged shards, (-2, -2), which come back
    byte for byte, like the clean ones.  RS(6,3): test_locate_pair.py's ambiguous column, which two
    pairs explain, beside a pair that is healed."""
    torch, rsmi = gpu
    k, m, S, nb = 10, 4, 1041, 7
    lay = Lay(rsmi, k, m, S, nb, aligned)
    sh = stripes(k, m, S, nb).copy()
    sh[0, 4, 1040] ^= 0x01; sh[0, 9, 3] ^= 0x10                             # healed, two data shards
    sh[1, 0, 1] ^= 0x01; sh[1, 6, 1000] ^= 0x02; sh[1, k + 3, 1040] ^= 0x03   # three damaged shards
    sh[2, k + 3, 0] ^= 0x80                                                 # healed, a single parity shard
    sh[3, 2, 100] ^= 0x21; sh[3, 7, 100] ^= 0x9C; sh[3, k, 100] ^= 0x55     # three, one byte column
    sh[5, k, 16] ^= 0x02; sh[5, k + 3, 1039] ^= 0x02                        # healed, two parity shards
    sh[6, 1, :] ^= 0xA5; sh[6, 2, :] ^= 0x5A; sh[6, 3, 512] ^= 0x01         # two stale rows and a byte
    with rsmi.Codec(k, m) as c:
        got, image = check(torch, c, lay, sh, label(lay))
        assert got.tolist() == [[4, 9], [UNKNOWN] * 2, [k + 3, CLEAN], [UNKNOWN] * 2, [CLEAN] * 2, [k, k + 3],
                                [UNKNOWN] * 2]
        assert all(np.array_equal(image[b], sh[b]) for b in (1, 3, 4, 6))
    k, m, S, nb = 6, 3, 1040, 4
    H = check_matrix(k, m)
    mul = orc.lib().rs_oracle_gal_mul
    lam = gf_solve(H[:, [1, 4, 2]], H[:, 7])   # h_7 = lam_1 h_1 + lam_4 h_4 + lam_2 h_2
    assert all(lam)
    sh = stripes(k, m, S, nb).copy()
    for b, (e, pos) in enumerate([(0x01, 3), (0x5D, 1039)]):
        sh[b, 1, pos] ^= mul(lam[0], e)
        sh[b, 4, pos] ^= mul(lam[1], e)
    cols = (orc.encode(k, m, np.ascontiguousarray(sh[0, :k])) ^ sh[0, k:])[:, [3]]
    assert in_span(H[:, [1, 4]], cols) and in_span(H[:, [2, 7]], cols)
    sh[2, 1, 3] ^= 0x11; sh[2, 4, 900] ^= 0x22; sh[2, 1, 500] ^= 0x33; sh[2, 4, 500] ^= 0x44
    lay = Lay(rsmi, k, m, S, nb, aligned)
    with rsmi.Codec(k, m) as c:
        got, image = check(torch, c, lay, sh, label(lay))
        assert got.tolist() == [[UNKNOWN] * 2, [UNKNOWN] * 2, [1, 4], [CLEAN] * 2], got.tolist()
        assert all(np.array_equal(image[b], sh[b]) for b in (0, 1, 3))
        assert np.array_equal(image[2], stripes(k, m, S, nb)[2])


# ---------------------------------------------------------------- 4: imitation
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
def test_imitated_pair_is_healed_to_another_codeword(gpu, aligned):
    """test_locate_pair.py's construction at RS(4,4), distance 5: errors in shards 0, 2 and 5 that
    imitate errors in shards 1 and 6.  The verdict is (1, 6), so shards 1 and 6 are rewritten to
    the definition's image: Verify is clean afterwards, and the stripe is not the original one.  A
    property of the code, pinned here."""
    torch, rsmi = gpu
    k, m, three, pair, lam = imitation_rs44()
    mul = orc.lib().rs_oracle_gal_mul
    S, nb = 1040, 3
    full = stripes(k, m, S, nb)
    sh = full.copy()
    for b, (e, pos) in enumerate([(0x01, 7), (0xC3, 1033)]):
        sh[b, three[0], pos] ^= mul(lam[0], e)
        sh[b, three[1], pos] ^= mul(lam[1], e)
        sh[b, three[2], pos] ^= e
    lay = Lay(rsmi, k, m, S, nb, aligned)
    with rsmi.Codec(k, m) as c:
        got, image = check(torch, c, lay, sh, label(lay))
        assert got.tolist() == [list(pair), list(pair), [CLEAN, CLEAN]]
        for b in (0, 1):
            assert all(not np.array_equal(image[b, i], sh[b, i]) for i in pair)            # the pair was rewritten
            assert all(np.array_equal(image[b, i], sh[b, i]) for i in range(k + m) if i not in pair)
        assert not verify_flags(torch, c, lay, lay.fill(image)).any()                      # a clean codeword
        assert not np.array_equal(image[:2], full[:2])                                     # but not the original


# ---------------------------------------------------------------- 5: m <= 2
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
@pytest.mark.parametrize("k,m", [(4, 2), (2, 1)])
def test_m_le_2_is_heal_widened(gpu, k, m, aligned):
    """RS(4,2) and RS(2,1) with two damaged shards, one damaged shard and a clean block: the buffer
    equals rsmi_heal_batch_dev's, the verdicts are its verdicts widened, and the label is heal's."""
    torch, rsmi = gpu
    S, nb = 1041, 4
    sh = stripes(k, m, S, nb).copy()
    sh[0, 0, 5] ^= 0x10
    sh[0, k, 1030] ^= 0x01
    sh[1, 1, 1040] ^= 0x80
    sh[3, 0, 100] ^= 0x33
    sh[3, 1, 100] ^= 0x44
    lay = Lay(rsmi, k, m, S, nb, aligned)
    host = lay.fill(sh)
    with rsmi.Codec(k, m) as c:
        got, image = check(torch, c, lay, sh, label(lay))
        assert got[1].tolist() == ([1, CLEAN] if m == 2 else [UNKNOWN, UNKNOWN])
        cul, _, healed = heal_run_dev(torch, c, lay, host, heal_label(lay))
        wide = np.stack([cul, np.where(cul < CLEAN, UNKNOWN, CLEAN)], axis=1)
        assert np.array_equal(got, wide)
        expect = host.copy()
        lay.rows(expect)[:] = image
        same_bytes(healed, expect, ("heal", k, m, aligned))


# ---------------------------------------------------------------- 6: fallback shapes
@pytest.mark.gpu
@pytest.mark.parametrize("k,m,S,aligned", [(20, 4, 333, True), (7, 3, 1025, True), (5, 5, 1040, True),
                                           (5, 5, 1040, False), (10, 4, 7, False)],
                         ids=["20-4", "7-3", "5-5", "5-5-split", "10-4-S7-pitch7"])
def test_fallback_shapes(gpu, k, m, S, aligned):
    """K > 16, K without an instantiation, m > 4 (two launch tiles) and unaligned rows shorter than
    16 bytes at an odd pitch: test_locate_pair.py's batch, pairs of every kind, a single culprit, a
    clean block and three damaged shards in one call; then the clean stripes."""
    torch, rsmi = gpu
    sh, want = fallback_case(k, m, S)
    nb = sh.shape[0]
    assert want[3].tolist() == [k + m - 1, CLEAN] and want[4].tolist() == [CLEAN, CLEAN]
    if m >= 4:
        assert want[:3].tolist() == [[0, k - 1], [k - 1, k], [k + 1, k + m - 1]]
    lay = Lay(rsmi, k, m, S, nb, aligned)
    assert aligned or lay.rs == S
    assert S != 7 or (lay.rs % 2 == 1 and lay.off % 2 == 1)
    full = stripes(k, m, S, nb)
    with rsmi.Codec(k, m) as c:
        _, image = check(torch, c, lay, sh, ROWS, want)
        for b in range(nb):
            assert np.array_equal(image[b], sh[b] if want[b, 0] == UNKNOWN else full[b]), b
        check(torch, c, lay, full, ROWS, np.full((nb, 2), CLEAN, dtype=np.int32))


@pytest.mark.gpu
def test_fallback_past_a_scratch_chunk(gpu):
    """The fallback's scratch rows are reused every 64 MiB: a chunk must be healed from its own
    encode.  test_verify_matrix's seam layout (RS(1,4), S = 15, rows back to back from an odd base,
    2^20 + 3 blocks, computed once and shared), with a pair on each side of the y grid's wrap, of
    the chunk seam and at both ends, the pair rotating over all ten."""
    torch, rsmi = gpu
    k, m = 1, 4
    lay, full, fill = seam_stripes(rsmi)
    pairs = all_pairs(k + m)
    sh = full.copy()
    want = np.full((lay.nb, 2), CLEAN, dtype=np.int32)
    for i, b in enumerate(SEAM_HIT):
        x, y = pairs[(3 * i) % len(pairs)]
        sh[b, x, (i * 7) % lay.S] ^= 1 << (i % 8)
        sh[b, y, (i * 5 + 1) % lay.S] ^= 0x80 >> (i % 8)
        want[b] = want_pair(k, m, sh[b])
        assert want[b].tolist() == [x, y], (b, want[b])
    image = sh.copy()
    image[SEAM_HIT] = want_image(k, m, sh[SEAM_HIT], want[SEAM_HIT])
    assert np.array_equal(image[SEAM_HIT], full[SEAM_HIT])
    host = fill(sh)
    with rsmi.Codec(k, m) as c:
        got, bad, after = run_dev(torch, c, lay, host, ROWS)
        assert np.array_equal(np.flatnonzero(got[:, 0] != CLEAN), np.array(SEAM_HIT))
        assert np.array_equal(got, want), (got[SEAM_HIT], want[SEAM_HIT])
        assert np.array_equal(np.flatnonzero(bad.any(axis=1)), np.array(SEAM_HIT))
        same_bytes(after, fill(image), "seam")


# ---------------------------------------------------------------- 7: scratch regrow, strided walk
@pytest.mark.gpu
@pytest.mark.parametrize("k,m,fused", [(5, 3, True), (7, 3, False)], ids=["fused", "fallback"])
def test_scratch_regrow(gpu, k, m, fused):
    """One context, one stream: 3 blocks at S = 1025, 40 blocks at S = 65541 (the stream's scratch
    is freed and reallocated behind the first call), then 3 blocks again in the larger scratch with
    no flags pointer.  One pair per call, at a different block."""
    torch, rsmi = gpu
    with rsmi.Codec(k, m) as c:
        for S, nb, (b, x, y), with_flags in ((1025, 3, (1, 0, k + 1), True), (65541, 40, (38, 2, 3), True),
                                             (1025, 3, (2, k, k + 2), False)):
            lay = Lay(rsmi, k, m, S, nb, True)
            full = stripes(k, m, S, nb)
            sh = full.copy()
            sh[b, x, S - 1] ^= 0x20
            sh[b, y, 0] ^= 0x02
            want = np.full((nb, 2), CLEAN, dtype=np.int32)
            want[b] = want_pair(k, m, sh[b])
            assert want[b].tolist() == [x, y]
            assert np.array_equal(want_image(k, m, sh[b:b + 1], want[b:b + 1])[0], full[b])
            got, bad, after = run_dev(torch, c, lay, lay.fill(sh), label(lay) if fused else ROWS, flags=with_flags)
            assert np.array_equal(got, want), (S, nb, got[b])
            if with_flags:
                assert np.array_equal(np.flatnonzero(bad.any(axis=1)), [b])
            same_bytes(after, lay.fill(full), (S, nb))


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
def test_waves_per_cu_1(gpu, aligned):
    """RS(10,4), S = 4099 (5 tiles a block) with option waves_per_cu = 1 and more tiles than the
    capped grid has waves, so every wave strides to further tiles, named blocks beside clean ones:
    the pair rotates over the blocks, every fifth block is clean, every seventh a single culprit."""
    torch, rsmi = gpu
    k, m, S = 10, 4, 4099
    n = k + m
    waves = max(1, torch.cuda.get_device_properties(0).multi_processor_count // 4) * 4
    nb = max(40, waves // 5 + 8)
    assert nb * 5 > waves
    pairs = all_pairs(n)
    full = stripes(k, m, S, nb)
    sh = full.copy()
    want = np.full((nb, 2), CLEAN, dtype=np.int32)
    for b in range(nb):
        if b % 5 == 4:
            continue
        x, y = pairs[(7 * b) % len(pairs)]
        sh[b, x, (b * 101) % S] ^= 0x10
        want[b] = (x, CLEAN)
        if b % 7 != 6:
            sh[b, y, S - 1 - (b * 53) % S] ^= 0x01
            want[b] = (x, y)
    for b in (0, 1, 4, 6, nb - 2, nb - 1):  # the definition on a sample: the distance promises the rest
        assert want_pair(k, m, sh[b]) == tuple(want[b])
    lay = Lay(rsmi, k, m, S, nb, aligned)
    with rsmi.Codec(k, m) as c:
        c.set_option("waves_per_cu", 1)
        got, bad, after = run_dev(torch, c, lay, lay.fill(sh), label(lay))
        assert np.array_equal(got, want)
        assert np.array_equal(bad, want_flags(k, m, sh))
        same_bytes(after, lay.fill(full), ("waves_per_cu", aligned))  # one or two damaged shards, m = 4


# ---------------------------------------------------------------- 8: the old route
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
def test_image_equals_the_old_route(gpu, aligned):
    """A mixed batch: the buffer after rsmi_heal_pair_batch_dev equals the one that pair verdicts
    read back, present and required masks built from them and one
    rsmi_reconstruct_mixed_batch_dev leave on a copy."""
    torch, rsmi = gpu
    k, m, S, nb = 10, 4, 4099, 7
    n = k + m
    full = stripes(k, m, S, nb)
    sh = full.copy()
    sh[0, 2, 100:3100] ^= 0xFF
    sh[0, 9, :] ^= 0x5A                                           # two stale data rows
    sh[1, 5, 4098] ^= 0x01                                        # a single culprit
    sh[3, 0, 0] ^= 0x80
    sh[3, k + 3, 2000:2100] ^= 0x33                               # data and parity
    sh[4, k, 1024] ^= 0x04
    sh[4, k + 1, 1023] ^= 0x40                                    # two parity rows
    sh[6, 0, 1] ^= 0x01
    sh[6, 6, 2000] ^= 0x02
    sh[6, k + 3, 4000] ^= 0x03                                    # three damaged shards
    want = [[2, 9], [5, CLEAN], [CLEAN, CLEAN], [0, k + 3], [k, k + 1], [CLEAN, CLEAN], [UNKNOWN, UNKNOWN]]
    lay = Lay(rsmi, k, m, S, nb, aligned)
    host = lay.fill(sh)
    with rsmi.Codec(k, m) as c:
        got, _, healed = run_dev(torch, c, lay, host, label(lay))
        assert got.tolist() == want == want_pairs(k, m, sh).tolist()
        lgot, _ = locate_pair_run_dev(torch, c, lay, host, pair_label(lay))
        assert np.array_equal(lgot, got)
        present = np.ones((nb, n), dtype=np.uint8)
        for b in range(nb):
            for x in lgot[b]:
                if x >= 0:
                    present[b, x] = 0
        required = (1 - present).astype(np.uint8)
        d = torch.from_numpy(host.copy()).cuda()
        base = d.data_ptr() + lay.off
        status = np.full(nb, POISON, dtype=np.int32)
        rc = rsmi.lib().rsmi_reconstruct_mixed_batch_dev(c._h, base, lay.rs, lay.bs, S, nb, present.ctypes.data,
                                                         required.ctypes.data, 0, status.ctypes.data,
                                                         torch.cuda.current_stream().cuda_stream)
        assert rc == 0 and (status == 0).all(), (rc, status)
        torch.cuda.synchronize()
        same_bytes(healed, d.cpu().numpy(), ("old route", aligned))
        expect = full.copy()
        expect[6] = sh[6]
        same_bytes(healed, lay.fill(expect), ("original", aligned))


# ---------------------------------------------------------------- 9: stream order
@pytest.mark.gpu
@pytest.mark.parametrize("k,m", [(10, 4), (7, 3)], ids=["fast", "fallback"])
def test_stream_order(gpu, k, m):
    """The damage is written by a side stream behind a delay, and the call's stream waits for it by
    an event; then heal pair (no flags pointer) and verify on the call's stream, with one sync at
    the end.  A heal that ran ahead of its stream would see clean stripes and leave the late damage
    in place; a heal kernel that ran ahead of the verdicts would heal nothing; a verify that ran
    ahead of the heal's stores would see the damage."""
    torch, rsmi = gpu
    S, nb = 4099, 3
    rs = rsmi.recommended_pitch(S)
    bs = (k + m) * rs
    full = stripes(k, m, S, nb)
    host = np.full(nb * bs, 0x11, dtype=np.uint8)
    rows = np.lib.stride_tricks.as_strided(host, shape=(nb, k + m, S), strides=(bs, rs, 1))
    rows[:] = full
    dirty = full.copy()
    dirty[1, 3, 1024] ^= 0x08
    dirty[1, k + 1, 7] ^= 0x80
    dirty[2, k + 1, 4098] ^= 0x80
    second = [[CLEAN, CLEAN], [3, k + 1], [k + 1, CLEAN]]
    assert want_pairs(k, m, dirty).tolist() == second
    pinned = torch.from_numpy(host).pin_memory()
    gate = Gate(torch)
    st, side = torch.cuda.Stream(), torch.cuda.Stream()
    with rsmi.Codec(k, m) as c:
        for warm in (True, False):  # the first pass builds the plans and the scratch; the second is the test
            d = torch.empty(nb * bs, dtype=torch.uint8, device="cuda")
            out = torch.empty(2 * nb, dtype=torch.int32, device="cuda")
            bad = torch.empty(nb * m, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                d.copy_(pinned, non_blocking=True)
                out.fill_(0x0BAD)
                bad.fill_(0x0BAD)
                loaded = st.record_event()
            with torch.cuda.stream(side):
                side.wait_event(loaded)
                gate()
                d[1 * bs + 3 * rs + 1024] ^= 0x08
                d[1 * bs + (k + 1) * rs + 7] ^= 0x80
                d[2 * bs + (k + 1) * rs + 4098] ^= 0x80
                damaged = side.record_event()
            with torch.cuda.stream(st):
                h = st.cuda_stream
                st.wait_event(damaged)
                c.heal_pair_batch_dev(d.data_ptr(), rs, bs, d.data_ptr() + k * rs, rs, bs, S, nb, out.data_ptr(), 0, h)
                c.verify_batch_dev(d.data_ptr(), rs, bs, d.data_ptr() + k * rs, rs, bs, S, nb, bad.data_ptr(), h)
            st.synchronize()
            side.synchronize()
            assert out.cpu().numpy().reshape(-1, 2).tolist() == second, warm
            assert not bad.cpu().numpy().any(), warm
            same_bytes(d.cpu().numpy(), host, ("stream order", warm))


# ---------------------------------------------------------------- 10: far offsets
@pytest.mark.gpu
def test_offsets_past_4gib(gpu):
    """Two blocks at block_stride = 2^32 + 256, the pair in the far block, aligned and shifted by
    one byte (the UA kernel).  Only the rows are touched: a store offset of either row truncated to
    32 bits would land in the near block, whose rows must come back as they were, like the far
    block's other rows."""
    torch, rsmi = gpu
    if torch.cuda.mem_get_info()[0] < 8 << 30:
        pytest.skip("needs 8 GiB of free device memory")
    k, m, S, nb = 4, 3, 1040, 2
    bs = 2 ** 32 + 256
    full = stripes(k, m, S, nb)
    try:
        with rsmi.Codec(k, m) as c:
            d = torch.empty(2 ** 32 + 2 ** 20, dtype=torch.uint8, device="cuda")
            assert 1 + bs + (k + m) * S <= d.numel()
            for off, (x, y) in ((0, (1, 2)), (0, (0, k)), (1, (3, k + 2)), (1, (k + 1, k + 2))):
                sh = full.copy()
                sh[1, x, 1033] ^= 0x10
                sh[1, y, 3] ^= 0x02
                assert want_pairs(k, m, sh).tolist() == [[CLEAN, CLEAN], [x, y]]
                for b in range(nb):
                    for i in range(k + m):
                        o = off + b * bs + i * S
                        d[o:o + S].copy_(torch.from_numpy(sh[b, i]))
                out = torch.full((2 * nb + 2,), POISON, dtype=torch.int32, device="cuda")
                base = d.data_ptr() + off
                c.heal_pair_batch_dev(base, S, bs, base + k * S, S, bs, S, nb, out.data_ptr(), 0,
                                      torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                assert c.last_kernel() == "rs_heal_pair_kernel<K=4,MT=3>" + ("" if off == 0 else ",UA")
                assert out.cpu().numpy().tolist() == [CLEAN, CLEAN, x, y, POISON, POISON]
                for b in range(nb):
                    for i in range(k + m):
                        o = off + b * bs + i * S
                        assert np.array_equal(d[o:o + S].cpu().numpy(), full[b, i]), (off, x, y, b, i)
            del d
    finally:
        torch.cuda.empty_cache()


# ---------------------------------------------------------------- 11: host paths
def _host_heal(c, data, dbs, parity, pbs, S, nb, flags=True):
    out = np.full(2 * nb + 2, POISON, dtype=np.int32)
    bad = np.full(nb * c.m + 2, POISON, dtype=np.uint32)
    c.heal_pair_batch_host_ptr(data, dbs, parity, pbs, S, nb, out.ctypes.data, bad.ctypes.data if flags else 0)
    assert (out[2 * nb:] == POISON).all() and (bad[nb * c.m:] == POISON).all()
    if not flags:
        assert (bad == POISON).all()
        return out[:2 * nb].reshape(-1, 2), None
    return out[:2 * nb].reshape(-1, 2), bad[:nb * c.m].reshape(nb, c.m) != 0


@pytest.mark.gpu
def test_host_page_locked_in_place(gpu):
    """Data and parity in one rsmi_host_alloc allocation, zero_copy 1: the kernels read and heal
    them where they lie, over PCIe at pitch S, the unaligned-window form."""
    torch, rsmi = gpu
    k, m, S, nb = 4, 3, 2049, 5
    full = stripes(k, m, S, nb)
    L = rsmi.lib()
    size = nb * (k + m) * S + 64
    p = L.rsmi_host_alloc(size)
    assert p
    try:
        buf = np.ctypeslib.as_array((ctypes.c_uint8 * size).from_address(p))
        rows = buf[:size - 64].reshape(nb, k + m, S)
        with rsmi.Codec(k, m) as c:
            c.set_option("zero_copy", 1)
            bs = (k + m) * S
            for damage in (None, [(3, 2, 2048), (3, k + 1, 0)], [(4, 0, 5), (4, 1, 1030), (0, k, 2040)],
                           [(1, 0, 7), (1, 1, 7), (1, k + 2, 7)]):
                buf[:] = 0x77
                rows[:] = full
                for at in damage or []:
                    rows[at] ^= 0x20
                sh = rows.copy()
                want = want_pairs(k, m, sh)
                assert (want[:, 0] != CLEAN).any() == (damage is not None)
                expect = buf.copy()
                expect[:size - 64].reshape(nb, k + m, S)[:] = want_image(k, m, sh, want)
                got, bad = _host_heal(c, p, bs, p + k * S, bs, S, nb, flags=damage is not None)
                assert c.last_kernel() == "rs_heal_pair_kernel<K=4,MT=3>,UA"
                assert np.array_equal(got, want), (damage, got)
                if bad is not None:
                    assert np.array_equal(bad, want_flags(k, m, sh))
                same_bytes(buf, expect, damage)
    finally:
        L.rsmi_host_free(p)


@pytest.mark.gpu
def test_small_call_and_one_block(gpu):
    """A small pageable batch and rsmi_heal_pair of one pageable block go through the page-locked
    staging, and only the one or two healed rows of a block return; Erasure.heal_pair on the golden
    RS(10,4) vectors, clean, with one stale shard and with two shards swapped."""
    torch, rsmi = gpu
    k, m, S, nb = 10, 4, 4099, 3
    full = stripes(k, m, S)
    assert nb * (k + m) * S * 2 <= (2 << 20)
    with rsmi.Codec(k, m) as c:
        sh = full.copy()
        sh[1, k + 2, 4098] ^= 0x02
        sh[1, 4, 0] ^= 0x02
        sh[2, 0, 0] ^= 0x80
        data = np.full((nb, k * S + 32), 0xA5, dtype=np.uint8)   # block strides past the rows: gaps
        par = np.full((nb, m * S + 16), 0x3C, dtype=np.uint8)
        data[:, :k * S] = sh[:, :k].reshape(nb, k * S)
        par[:, :m * S] = sh[:, k:].reshape(nb, m * S)
        want = want_pairs(k, m, sh)
        image = want_image(k, m, sh, want)
        d1, p1 = data.copy(), par.copy()
        d1[:, :k * S] = image[:, :k].reshape(nb, k * S)
        p1[:, :m * S] = image[:, k:].reshape(nb, m * S)
        got, bad = _host_heal(c, data.ctypes.data, k * S + 32, par.ctypes.data, m * S + 16, S, nb)
        assert c.last_kernel() == "rs_heal_pair_kernel<K=10,MT=4>,UA"
        assert got.tolist() == want.tolist() == [[CLEAN, CLEAN], [4, k + 2], [0, CLEAN]]
        assert np.array_equal(bad, want_flags(k, m, sh))
        same_bytes(data.reshape(-1), d1.reshape(-1), "small data")
        same_bytes(par.reshape(-1), p1.reshape(-1), "small parity")
        assert np.array_equal(image, full)
        # one block, in place
        one = bytearray(full[0].tobytes())
        assert c.heal_pair(one, S) == (CLEAN, CLEAN) and one == full[0].tobytes()
        one[5 * S + 17] ^= 0x01
        assert c.heal_pair(one, S) == (5, CLEAN) and one == full[0].tobytes()
        one[5 * S + 17] ^= 0x01
        one[(k + 3) * S + S - 1] ^= 0x01
        assert c.heal_pair(one, S) == (5, k + 3) and one == full[0].tobytes()
        one[5 * S + 17] ^= 0x01
        one[(k + 3) * S + S - 1] ^= 0x01
        one[2 * S + 100] ^= 0x01
        three = bytes(one)
        assert want_pair(k, m, np.frombuffer(three, dtype=np.uint8).reshape(k + m, S)) == (UNKNOWN, UNKNOWN)
        assert c.heal_pair(one, S) == (UNKNOWN, UNKNOWN) and one == three  # three damaged shards: untouched
    z = np.load(os.path.join(GOLDEN, "vectors_k10_m4.npz"))
    shards = [bytes(r.tobytes()) for r in z["shards_4099"]]
    e = rsmi.NewErasure(10, 4, 4099)
    assert e.heal_pair(shards) == ((CLEAN, CLEAN), shards)
    stale = list(shards)
    stale[12] = bytes(len(shards[12]))
    assert e.heal_pair(stale) == ((12, CLEAN), shards)
    sw = list(shards)
    sw[3], sw[12] = sw[12], sw[3]
    assert want_pair(10, 4, np.stack([np.frombuffer(s, dtype=np.uint8) for s in sw])) == (3, 12)
    v, healed = e.heal_pair(sw)
    assert v == (3, 12) and healed == shards
    assert all(a is b for i, (a, b) in enumerate(zip(healed, sw)) if i not in (3, 12))  # the caller's entries
    e._codec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("S,past_chunk", [(2048, False), (2049, False), (2049, True)],
                         ids=["2d-copy", "odd", "odd-past-64MiB"])
def test_host_pipeline_pageable(gpu, S, past_chunk):
    """RS(2,3), pageable buffers, small_call_bytes 0: the upload pipeline, with 2D copies and with
    linear copies and the repitch kernel (odd S); the last case has more blocks than one 64 MiB
    chunk holds, with pairs on both sides of the seam.  Only the named rows of the caller's arrays
    change."""
    torch, rsmi = gpu
    k, m = 2, 3
    chunk = max(1, (64 << 20) // (5 * rsmi.recommended_pitch(S)))
    nb = chunk + 3 if past_chunk else 9
    rng = np.random.default_rng(S + nb)
    data = rng.integers(0, 256, size=(nb, k, S), dtype=np.uint8)
    parity = orc.encode_fast(k, m, data, threads=8)
    hit = sorted({0, nb - 1, chunk - 1, chunk, chunk + 1} if past_chunk else {0, 4, nb - 1})
    pairs = all_pairs(k + m)
    want = np.full((nb, 2), CLEAN, dtype=np.int32)
    for i, b in enumerate(hit):
        x, y = pairs[(3 * i + 1) % len(pairs)]
        for r, pos in ((x, (i * 211) % S), (y, (i * 17 + 1) % S)):
            (data if r < k else parity)[b, r if r < k else r - k, pos] ^= 1 << (i % 8)
    d1, p1 = data.copy(), parity.copy()
    for b in hit:
        sh = np.concatenate([data[b], parity[b]])
        want[b] = want_pair(k, m, sh)  # m = 3: the definition decides
        im = want_image(k, m, sh[None], want[b:b + 1])[0]
        d1[b], p1[b] = im[:k], im[k:]
    assert (want[hit, 1] >= 0).any()
    with rsmi.Codec(k, m) as c:
        c.set_option("small_call_bytes", 0)
        got, bad = _host_heal(c, data.ctypes.data, k * S, parity.ctypes.data, m * S, S, nb)
        assert c.last_kernel() == "rs_heal_pair_kernel<K=2,MT=3>"
        assert np.array_equal(np.flatnonzero(got[:, 0] != CLEAN), np.array(hit))
        assert np.array_equal(got, want)
        assert np.array_equal(np.flatnonzero(bad.any(axis=1)), np.array(hit))
        same_bytes(data.reshape(-1), d1.reshape(-1), "pipeline data")
        same_bytes(parity.reshape(-1), p1.reshape(-1), "pipeline parity")


@pytest.mark.gpu
@pytest.mark.parametrize("pinned_half", ["data", "parity"])
def test_host_mixed_page_locked_and_pageable(gpu, pinned_half):
    """One half page-locked (rsmi_host_alloc), the other pageable, a small call: the page-locked
    half is healed where it lies, the other in the staging, from which only the named rows return.
    A pair across the halves, a pair inside each half, and a clean block."""
    torch, rsmi = gpu
    k, m, S, nb = 4, 3, 2049, 4
    full = stripes(k, m, S, nb)
    sh = full.copy()
    sh[0, 1, 2048] ^= 0x01; sh[0, k + 2, 5] ^= 0x02
    sh[1, 0, 17] ^= 0x10; sh[1, 3, 1024] ^= 0x20
    sh[3, k, 0] ^= 0x40; sh[3, k + 1, 2047] ^= 0x80
    want = want_pairs(k, m, sh)
    assert (want[[0, 1, 3], 1] >= 0).any() and want[2].tolist() == [CLEAN, CLEAN]
    image = want_image(k, m, sh, want)
    rows = k if pinned_half == "data" else m
    L = rsmi.lib()
    size = nb * rows * S + 64
    p = L.rsmi_host_alloc(size)
    assert p
    try:
        pin = np.ctypeslib.as_array((ctypes.c_uint8 * size).from_address(p))
        pin[:] = 0x77
        lo, hi = (0, k) if pinned_half == "data" else (k, k + m)
        pin[:size - 64].reshape(nb, rows, S)[:] = sh[:, lo:hi]
        other = np.ascontiguousarray(sh[:, k:] if pinned_half == "data" else sh[:, :k])
        with rsmi.Codec(k, m) as c:
            c.set_option("zero_copy", 1)
            if pinned_half == "data":
                got, bad = _host_heal(c, p, k * S, other.ctypes.data, m * S, S, nb)
            else:
                got, bad = _host_heal(c, other.ctypes.data, k * S, p, m * S, S, nb)
            assert c.last_kernel() == "rs_heal_pair_kernel<K=4,MT=3>,UA"
            assert np.array_equal(got, want) and np.array_equal(bad, want_flags(k, m, sh))
            assert np.array_equal(pin[:size - 64].reshape(nb, rows, S), image[:, lo:hi])
            assert (pin[size - 64:] == 0x77).all()
            assert np.array_equal(other, image[:, k:] if pinned_half == "data" else image[:, :k])
    finally:
        L.rsmi_host_free(p)
