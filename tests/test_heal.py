"""rsmi_heal on the GPU against the definition, computed with the CPU oracle, exactly.

The verdict of a block is test_locate.want_verdict's (replace shard x by its reconstruction from
the others, re-encode, compare).  The expected image of a block with verdict x >= 0 is the stored
shards with row x replaced by the oracle's reconstruction of it from the other rows; of any other
block, the block unchanged.  Neither comes from the library.  The whole buffer is compared byte
for byte (the sentinels of test_verify.Lay in data padding, parity padding and gaps included),
the verdicts and flags against the definition, the poisoned tails of the outputs, and the launch
label.  There are no tolerances.

  1  clean stripes, damage in padding and gaps only: nothing is written
  2  every shard as the culprit in one call
  3  a stale shard, S = 4099
  4  the UA layout's last window overlapping the previous tile's, across waves
  5  blocks that must not be touched: two damaged shards, m = 1
  6  aliasing: the named third shard is rewritten; clean, but not the original
  7  shapes without an rs_heal_kernel: rs_heal_rows_kernel, and the 64 MiB scratch seam
  8  waves_per_cu = 1: the grid-stride loop
  9  stream order, with no host sync between damage, heal and verify; no flags pointer
 10  host paths: page-locked rows in place, the small call, the upload pipeline, Erasure.heal
 11  the image equals reconstruct_rows_batch_dev's with the culprit marked missing
 12  no side effects on the encode, reconstruct, verify and locate of the same context
 13  offsets past 4 GiB
"""
import ctypes
import os

import numpy as np
import pytest

import oracle_lib as orc
from test_locate import CLEAN, UNKNOWN, gf_solve2, want_verdict, want_verdicts
from test_locate import label as locate_label
from test_stream_order import Gate
from test_verify import Lay, stripes, want_flags
from test_verify_matrix import SEAM_HIT, seam_stripes

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROWS = "rs_heal_rows_kernel"
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
    """m = 1 never heals: the launches are locate's, that is Verify's."""
    if lay.m == 1:
        return locate_label(lay)
    return "rs_heal_kernel<K=%d,MT=%d>%s" % (lay.k, lay.m, "" if lay.aligned else ",UA")


def want_image(k, m, sh, verdicts):
    """The definition's image of shards sh (nb, n, S) under its verdicts."""
    out = sh.copy()
    for b, x in enumerate(verdicts):
        if x >= 0:
            rc, rec = orc.reconstruct(k, m, sh[b], [i != x for i in range(k + m)], False)
            assert rc == 0
            out[b, x] = rec[x]
    return out


def run_dev(torch, c, lay, host, lab, flags=True):
    """rsmi_heal_batch_dev over host's bytes: (verdicts, flags as bool or None, the buffer after).
    Both outputs start poisoned and only their first nb (nb * m) entries may change."""
    d = torch.from_numpy(host.copy()).cuda()
    assert d.data_ptr() % 256 == 0
    cul = torch.full((lay.nb + 2,), POISON, dtype=torch.int32, device="cuda")
    bad = torch.full((lay.nb * lay.m + 2,), POISON, dtype=torch.int32, device="cuda")
    base = d.data_ptr() + lay.off
    c.heal_batch_dev(base, lay.rs, lay.bs, base + lay.k * lay.rs, lay.rs, lay.bs, lay.S, lay.nb, cul.data_ptr(),
                     bad.data_ptr() if flags else 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert c.last_kernel() == lab, (c.last_kernel(), lab)
    cul, bad = cul.cpu().numpy(), bad.cpu().numpy()
    assert (cul[lay.nb:] == POISON).all() and (bad[lay.nb * lay.m:] == POISON).all(), "wrote past its outputs"
    after = d.cpu().numpy()
    if not flags:
        assert (bad == POISON).all()
        return cul[:lay.nb], None, after
    return cul[:lay.nb], bad[:lay.nb * lay.m].reshape(lay.nb, lay.m) != 0, after


def same_bytes(got, want, ctx):
    if not np.array_equal(got, want):
        at = np.flatnonzero(got != want)
        raise AssertionError("%r: %d bytes differ, first at offset %d: got %#x, want %#x" %
                             (ctx, at.size, at[0], got[at[0]], want[at[0]]))


def verify_flags(torch, c, lay, host):
    d = torch.from_numpy(host.copy()).cuda()
    bad = torch.full((lay.nb * lay.m,), POISON, dtype=torch.int32, device="cuda")
    base = d.data_ptr() + lay.off
    c.verify_batch_dev(base, lay.rs, lay.bs, base + lay.k * lay.rs, lay.rs, lay.bs, lay.S, lay.nb, bad.data_ptr(),
                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return bad.cpu().numpy().reshape(lay.nb, lay.m) != 0


def check(torch, c, lay, sh, lab, want=None, host=None, flags=True):
    """Heal sh (nb, n, S) laid out by lay (host: the buffer, when it is not lay.fill(sh)): the
    verdicts and flags are the definition's for sh, the buffer after is host with the rows
    replaced by the definition's image.  Returns (verdicts, image)."""
    if want is None:
        want = want_verdicts(lay.k, lay.m, sh)
    image = want_image(lay.k, lay.m, sh, want)
    host = lay.fill(sh) if host is None else host
    assert np.array_equal(lay.rows(host), sh)
    got, bad, after = run_dev(torch, c, lay, host, lab, flags)
    ctx = (lay.k, lay.m, lay.S, lay.aligned)
    assert np.array_equal(got, want), (ctx, got, want)
    if flags:
        assert np.array_equal(bad, want_flags(lay.k, lay.m, sh)), ctx
    expect = host.copy()
    lay.rows(expect)[:] = image
    same_bytes(after, expect, ctx)
    return got, image


# ---------------------------------------------------------------- 1: clean stripes
SIZES_1 = [16, 17, 31, 1008, 1024, 1025, 1040, 4099]


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
@pytest.mark.parametrize("k,m", [(2, 1), (2, 2), (4, 2), (10, 4), (16, 4)])
def test_clean_stripes_are_not_written(gpu, k, m, aligned):
    torch, rsmi = gpu
    nb = 3
    clean = np.full(nb, CLEAN, dtype=np.int32)
    with rsmi.Codec(k, m) as c:
        for S in SIZES_1:
            lay = Lay(rsmi, k, m, S, nb, aligned)
            full = stripes(k, m, S)
            assert (want_verdicts(k, m, full) == CLEAN).all()
            host = lay.fill(full)
            # damage where no row byte is: the gap after a block and, aligned, the padding of a
            # data row and of a parity row at offset S
            spots = [lay.off + 1 * lay.bs + (k + m) * lay.rs] if aligned else [0, lay.off + nb * lay.bs]
            if aligned and lay.rs > S:
                spots += [lay.off + 1 * lay.bs + r * lay.rs + S for r in (0, k, k + m - 1)]
            for o in [None] + spots:
                h2 = host.copy()
                if o is not None:
                    h2[o] ^= 0xFF
                got, _ = check(torch, c, lay, full, label(lay), clean, h2)
                assert (got == CLEAN).all()


# ---------------------------------------------------------------- 2: every shard as the culprit
POS_2 = [0, 15, 16, 1023, 1024, -1]


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
@pytest.mark.parametrize("S", [1025, 1040])
@pytest.mark.parametrize("k,m", [(4, 2), (10, 4), (16, 4)])
def test_every_shard_as_culprit(gpu, k, m, S, aligned):
    """n + 2 blocks, block b < n with one flipped byte in shard b, the byte placed in turn at the
    chunk and tile edges and at S - 1; two clean blocks.  One call heals them all."""
    torch, rsmi = gpu
    n = k + m
    lay = Lay(rsmi, k, m, S, n + 2, aligned)
    full = stripes(k, m, S, n + 2)
    sh = full.copy()
    for b in range(n):
        sh[b, b, POS_2[b % len(POS_2)] % S] ^= 0x40
    want = want_verdicts(k, m, sh)
    assert want.tolist() == list(range(n)) + [CLEAN, CLEAN]  # what the distance promises
    with rsmi.Codec(k, m) as c:
        _, image = check(torch, c, lay, sh, label(lay), want)
        assert np.array_equal(image, full)  # one damaged shard, m >= 2: the original bytes
        assert not verify_flags(torch, c, lay, lay.fill(image)).any()
        # and straight after the heal, on the device
        d = torch.from_numpy(lay.fill(sh)).cuda()
        cul = torch.empty(n + 2, dtype=torch.int32, device="cuda")
        bad = torch.full(((n + 2) * m,), POISON, dtype=torch.int32, device="cuda")
        base, h = d.data_ptr() + lay.off, torch.cuda.current_stream().cuda_stream
        c.heal_batch_dev(base, lay.rs, lay.bs, base + k * lay.rs, lay.rs, lay.bs, S, n + 2, cul.data_ptr(), 0, h)
        c.verify_batch_dev(base, lay.rs, lay.bs, base + k * lay.rs, lay.rs, lay.bs, S, n + 2, bad.data_ptr(), h)
        torch.cuda.synchronize()
        assert not bad.cpu().numpy().any()
        assert cul.cpu().numpy().tolist() == want.tolist()


# ---------------------------------------------------------------- 3: a stale shard
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
@pytest.mark.parametrize("k,m", [(10, 4), (4, 2)])
def test_stale_shard(gpu, k, m, aligned):
    """A whole row of random bytes, S = 4099 (5 tiles; the last chunk is partial on aligned rows
    and an overlapping window on split ones): a data row and a parity row, in different blocks."""
    torch, rsmi = gpu
    S, nb = 4099, 3
    lay = Lay(rsmi, k, m, S, nb, aligned)
    rng = np.random.default_rng(34)
    full = stripes(k, m, S)
    sh = full.copy()
    sh[0, k - 2] = rng.integers(0, 256, size=S, dtype=np.uint8)
    sh[2, k + m - 1] = rng.integers(0, 256, size=S, dtype=np.uint8)
    with rsmi.Codec(k, m) as c:
        got, image = check(torch, c, lay, sh, label(lay))
        assert got.tolist() == [k - 2, CLEAN, k + m - 1]
        assert np.array_equal(image, full)


# ---------------------------------------------------------------- 4: UA overlap across waves
@pytest.mark.gpu
@pytest.mark.parametrize("wpc", [0, 1], ids=["one-tile-per-wave", "waves_per_cu-1"])
@pytest.mark.parametrize("r", [1, 15])
def test_ua_last_window_overlaps_previous_tile(gpu, r, wpc):
    """Split layout, S = 2048 + r: chunk 128 is the only chunk of tile 2, its window [S - 16, S)
    overlaps chunk 127's [2032, 2048) of tile 1, which another wave holds.  The culprit row is
    damaged over [S - 40, S), so both waves see damage in the bytes they share; a data culprit and
    a parity culprit.  A delta applied twice to one byte would restore the damage."""
    torch, rsmi = gpu
    k, m, nb = 10, 4, 3
    S = 2048 + r
    assert (S + 15) // 16 == 129 and S - 16 < 2048
    lay = Lay(rsmi, k, m, S, nb, False)
    full = stripes(k, m, S, nb)
    sh = full.copy()
    rng = np.random.default_rng(40 + r)
    for b, x in ((0, 3), (2, k + 2)):
        sh[b, x, S - 40:] ^= rng.integers(1, 256, size=40, dtype=np.uint8)
    with rsmi.Codec(k, m) as c:
        if wpc:
            c.set_option("waves_per_cu", wpc)
        got, image = check(torch, c, lay, sh, label(lay))
        assert got.tolist() == [3, CLEAN, k + 2]
        assert np.array_equal(image, full)


# ---------------------------------------------------------------- 5: blocks that must not be touched
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
def test_unknown_blocks_are_not_touched(gpu, aligned):
    """RS(10,4): healed blocks mixed with blocks of two damaged shards (UNKNOWN by the distance),
    which come back byte for byte; RS(2,1): every dirty block is UNKNOWN and nothing is written."""
    torch, rsmi = gpu
    k, m, S, nb = 10, 4, 1040, 6
    lay = Lay(rsmi, k, m, S, nb, aligned)
    sh = stripes(k, m, S, nb).copy()
    sh[0, 4, 1039] ^= 0x01                                  # healed, data
    sh[1, 2, 100] ^= 0x21; sh[1, 7, 100] ^= 0x9C            # two data shards, one byte column
    sh[2, k + 3, 0] ^= 0x80                                 # healed, parity
    sh[3, 3, 5] ^= 0x10; sh[3, k + 1, 1030] ^= 0x10         # a data and a parity shard, two tiles
    sh[5, k, 16] ^= 0x02; sh[5, k + 3, 17] ^= 0x02          # two parity shards
    with rsmi.Codec(k, m) as c:
        got, image = check(torch, c, lay, sh, label(lay))
        assert got.tolist() == [4, UNKNOWN, k + 3, UNKNOWN, CLEAN, UNKNOWN]
        assert all(np.array_equal(image[b], sh[b]) for b in (1, 3, 4, 5))
    k, m, S, nb = 2, 1, 1025, 4
    lay = Lay(rsmi, k, m, S, nb, aligned)
    sh = stripes(k, m, S, nb).copy()
    sh[0, 0, 1024] ^= 0x01
    sh[1, 2, 0] ^= 0x80
    sh[3, 1, 512] ^= 0x10
    with rsmi.Codec(k, m) as c:
        got, image = check(torch, c, lay, sh, label(lay))
        assert got.tolist() == [UNKNOWN, UNKNOWN, CLEAN, UNKNOWN] and np.array_equal(image, sh)
        assert label(lay).startswith("rs_verify_kernel<K=2,MT=1>")


# ---------------------------------------------------------------- 6: aliasing
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
def test_aliasing_rewrites_the_named_shard(gpu, aligned):
    """test_locate.py case 5's construction at RS(4,2), distance 3: errors in shards 0 and 1 that
    imitate an error in shard 2 alone.  The verdict is 2, so shard 2 is rewritten to the
    definition's image: Verify is clean afterwards, and the stripe is not the original one.  A
    property of the code, pinned here."""
    torch, rsmi = gpu
    k, m, S, nb = 4, 2, 1040, 3
    P = orc.build_matrix(k, m)[k:]
    mul = orc.lib().rs_oracle_gal_mul
    lay = Lay(rsmi, k, m, S, nb, aligned)
    full = stripes(k, m, S)
    sh = full.copy()
    for b, (e, pos) in enumerate([(0x01, 5), (0xB7, 1029)]):
        e0, e1 = gf_solve2(P[:, :2], [mul(e, int(P[0, 2])), mul(e, int(P[1, 2]))])
        assert e0 and e1
        sh[b, 0, pos] ^= e0
        sh[b, 1, pos] ^= e1
    with rsmi.Codec(k, m) as c:
        got, image = check(torch, c, lay, sh, label(lay))
        assert got.tolist() == [2, 2, CLEAN]
        for b in (0, 1):
            assert not np.array_equal(image[b, 2], sh[b, 2])                       # shard 2 was rewritten
            assert all(np.array_equal(image[b, i], sh[b, i]) for i in range(k + m) if i != 2)
        assert not verify_flags(torch, c, lay, lay.fill(image)).any()              # a clean codeword
        assert not np.array_equal(image[:2], full[:2])                             # but not the original


# ---------------------------------------------------------------- 7: fallback shapes
@pytest.mark.gpu
@pytest.mark.parametrize("k,m,S,aligned", [(17, 3, 333, True), (5, 5, 1040, True), (5, 5, 1040, False),
                                           (7, 2, 1025, True), (4, 2, 9, False)],
                         ids=["17-3", "5-5", "5-5-split", "7-2", "4-2-S9-pitch9"])
def test_fallback_shapes(gpu, k, m, S, aligned):
    """K > 16, m > 4 (two launch tiles), K without an instantiation, and unaligned rows shorter
    than 16 bytes: a data culprit, a parity culprit (the last row, across the tile seam), two
    damaged shards, a clean block and a stale data row in one call."""
    torch, rsmi = gpu
    nb = 5
    lay = Lay(rsmi, k, m, S, nb, aligned)
    assert aligned or lay.rs == S
    full = stripes(k, m, S, nb)
    sh = full.copy()
    sh[0, k - 1, S - 1] ^= 0x10
    sh[1, k + m - 1, 0] ^= 0x01
    sh[2, 0, S // 2] ^= 0x33
    sh[2, k, S // 2] ^= 0x44
    sh[4, 1] = np.random.default_rng(5).integers(0, 256, size=S, dtype=np.uint8)
    with rsmi.Codec(k, m) as c:
        got, image = check(torch, c, lay, sh, ROWS)
        got = got.tolist()
        assert got[:2] + got[3:] == [k - 1, k + m - 1, CLEAN, 1]
        assert m < 4 or got[2] == UNKNOWN
        assert all(np.array_equal(image[b], full[b]) for b in (0, 1, 3, 4))
        got, _ = check(torch, c, lay, full, ROWS, np.full(nb, CLEAN, dtype=np.int32))


@pytest.mark.gpu
def test_fallback_scratch_chunk_seam(gpu):
    """The fallback's scratch rows are reused every 64 MiB: a chunk must be healed from its own
    encode.  A chunk boundary needs nblocks * m * round_up(S, 16) > 64 MiB whatever the shape, so
    the image cannot be a few MB; this is test_verify_matrix's seam layout (RS(1,4), S = 15, rows
    back to back from an odd base, 2^20 + 3 blocks, computed once and shared), with a culprit on
    each side of the y grid's wrap, of the chunk seam and at both ends, the shard rotating over
    all five."""
    torch, rsmi = gpu
    k, m, S = 1, 4, 15
    lay, full, fill = seam_stripes(rsmi)
    sh = full.copy()
    want = np.full(lay.nb, CLEAN, dtype=np.int32)
    for i, b in enumerate(SEAM_HIT):
        x = i % (k + m)
        sh[b, x, (i * 7) % S] ^= 1 << (i % 8)
        want[b] = want_verdict(k, m, sh[b])
        assert want[b] == x
    image = sh.copy()
    image[SEAM_HIT] = want_image(k, m, sh[SEAM_HIT], want[SEAM_HIT])
    assert np.array_equal(image[SEAM_HIT], full[SEAM_HIT])
    host = fill(sh)
    with rsmi.Codec(k, m) as c:
        got, bad, after = run_dev(torch, c, lay, host, ROWS)
        assert np.array_equal(np.flatnonzero(got != CLEAN), np.array(SEAM_HIT))
        assert np.array_equal(got, want)
        assert np.array_equal(np.flatnonzero(bad.any(axis=1)), np.array(SEAM_HIT))
        same_bytes(after, fill(image), "seam")


# ---------------------------------------------------------------- 8: waves_per_cu = 1
_WANT8 = {}


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
@pytest.mark.parametrize("many", [False, True], ids=["40-blocks", "past-the-grid"])
def test_waves_per_cu_1(gpu, many, aligned):
    """RS(10,4), S = 4099 (5 tiles a block), option waves_per_cu = 1: 40 blocks, and as many as it
    takes for more tiles than the capped grid has waves, so that every wave strides to a second
    tile.  Block i has byte 4098 of shard i % n flipped; every seventh block a second shard as
    well (UNKNOWN, untouched), every eleventh is clean."""
    torch, rsmi = gpu
    k, m, S = 10, 4, 4099
    n, tpb = k + m, 5
    waves = max(1, torch.cuda.get_device_properties(0).multi_processor_count // 4) * 4
    nb = max(40, waves // tpb + 8) if many else 40
    assert not many or nb * tpb > waves
    lay = Lay(rsmi, k, m, S, nb, aligned)
    sh = stripes(k, m, S, nb).copy()
    for i in range(nb):
        if i % 11 == 10:
            continue
        sh[i, i % n, 4098] ^= 0x40
        if i % 7 == 6:
            sh[i, (i + 5) % n, 77] ^= 0x04
    if nb not in _WANT8:
        _WANT8[nb] = want_verdicts(k, m, sh)
    want = _WANT8[nb]
    assert all(want[i] == (CLEAN if i % 11 == 10 else UNKNOWN if i % 7 == 6 else i % n) for i in range(nb))
    with rsmi.Codec(k, m) as c:
        c.set_option("waves_per_cu", 1)
        check(torch, c, lay, sh, label(lay), want)


# ---------------------------------------------------------------- 9: stream order
@pytest.mark.gpu
@pytest.mark.parametrize("k,m", [(10, 4), (7, 2)], ids=["fast", "fallback"])
def test_stream_order(gpu, k, m):
    """The damage is written by a side stream behind a delay, and the call's stream waits for it by
    an event; then heal (no flags pointer) and verify on the call's stream, with one sync at the
    end.  A heal that ran ahead of its stream would see clean stripes and leave the late damage in
    place; a verify that ran ahead of the heal's stores would see the damage."""
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
    dirty[2, k + 1, 4098] ^= 0x80
    assert want_verdicts(k, m, dirty).tolist() == [CLEAN, 3, k + 1]
    pinned = torch.from_numpy(host).pin_memory()
    gate = Gate(torch)
    st, side = torch.cuda.Stream(), torch.cuda.Stream()
    with rsmi.Codec(k, m) as c:
        for warm in (True, False):  # the first pass builds the plans and the scratch; the second is the test
            d = torch.empty(nb * bs, dtype=torch.uint8, device="cuda")
            cul = torch.empty(nb, dtype=torch.int32, device="cuda")
            bad = torch.empty(nb * m, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                d.copy_(pinned, non_blocking=True)
                cul.fill_(0x0BAD)
                bad.fill_(0x0BAD)
                loaded = st.record_event()
            with torch.cuda.stream(side):
                side.wait_event(loaded)
                gate()
                d[1 * bs + 3 * rs + 1024] ^= 0x08
                d[2 * bs + (k + 1) * rs + 4098] ^= 0x80
                damaged = side.record_event()
            with torch.cuda.stream(st):
                h = st.cuda_stream
                st.wait_event(damaged)
                c.heal_batch_dev(d.data_ptr(), rs, bs, d.data_ptr() + k * rs, rs, bs, S, nb, cul.data_ptr(), 0, h)
                c.verify_batch_dev(d.data_ptr(), rs, bs, d.data_ptr() + k * rs, rs, bs, S, nb, bad.data_ptr(), h)
            st.synchronize()
            side.synchronize()
            assert cul.cpu().numpy().tolist() == [CLEAN, 3, k + 1], warm
            assert not bad.cpu().numpy().any(), warm
            same_bytes(d.cpu().numpy(), host, ("stream order", warm))


# ---------------------------------------------------------------- 10: host paths
def _host_heal(c, data, dbs, parity, pbs, S, nb, flags=True):
    cul = np.full(nb + 2, POISON, dtype=np.int32)
    bad = np.full(nb * c.m + 2, POISON, dtype=np.uint32)
    c.heal_batch_host_ptr(data, dbs, parity, pbs, S, nb, cul.ctypes.data, bad.ctypes.data if flags else 0)
    assert (cul[nb:] == POISON).all() and (bad[nb * c.m:] == POISON).all()
    if not flags:
        assert (bad == POISON).all()
        return cul[:nb], None
    return cul[:nb], bad[:nb * c.m].reshape(nb, c.m) != 0


@pytest.mark.gpu
def test_host_page_locked_in_place(gpu):
    """Data and parity in one rsmi_host_alloc allocation, zero_copy 1: the kernels read and heal
    them where they lie, over PCIe at pitch S, the unaligned-window form."""
    torch, rsmi = gpu
    k, m, S, nb = 4, 2, 2049, 5
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
            for damage in (None, [(3, 2, 2048)], [(4, k + 1, 0), (0, 0, 1024)], [(1, 0, 7), (1, 1, 7)]):
                buf[:] = 0x77
                rows[:] = full
                for at in damage or []:
                    rows[at] ^= 0x20
                sh = rows.copy()
                want = want_verdicts(k, m, sh)
                assert (want != CLEAN).any() == (damage is not None)
                expect = buf.copy()
                expect[:size - 64].reshape(nb, k + m, S)[:] = want_image(k, m, sh, want)
                got, bad = _host_heal(c, p, bs, p + k * S, bs, S, nb, flags=damage is not None)
                assert c.last_kernel() == "rs_heal_kernel<K=4,MT=2>,UA"
                assert np.array_equal(got, want), (damage, got)
                if bad is not None:
                    assert np.array_equal(bad, want_flags(k, m, sh))
                same_bytes(buf, expect, damage)
    finally:
        L.rsmi_host_free(p)


@pytest.mark.gpu
def test_small_call_and_one_block(gpu):
    """A small pageable batch and rsmi_heal of one pageable block go through the page-locked
    staging, and only the healed rows return; Erasure.heal on the golden RS(10,4) vectors."""
    torch, rsmi = gpu
    k, m, S, nb = 10, 4, 4099, 3
    full = stripes(k, m, S)
    assert nb * (k + m) * S * 2 <= (2 << 20)
    with rsmi.Codec(k, m) as c:
        sh = full.copy()
        sh[1, k + 2, 4098] ^= 0x02
        sh[2, 0, 0] ^= 0x80
        data = np.full((nb, k * S + 32), 0xA5, dtype=np.uint8)   # block strides past the rows: gaps
        par = np.full((nb, m * S + 16), 0x3C, dtype=np.uint8)
        data[:, :k * S] = sh[:, :k].reshape(nb, k * S)
        par[:, :m * S] = sh[:, k:].reshape(nb, m * S)
        want = want_verdicts(k, m, sh)
        image = want_image(k, m, sh, want)
        d1, p1 = data.copy(), par.copy()
        d1[:, :k * S] = image[:, :k].reshape(nb, k * S)
        p1[:, :m * S] = image[:, k:].reshape(nb, m * S)
        got, bad = _host_heal(c, data.ctypes.data, k * S + 32, par.ctypes.data, m * S + 16, S, nb)
        assert c.last_kernel() == "rs_heal_kernel<K=10,MT=4>,UA"
        assert got.tolist() == want.tolist() == [CLEAN, k + 2, 0]
        assert np.array_equal(bad, want_flags(k, m, sh))
        same_bytes(data.reshape(-1), d1.reshape(-1), "small data")
        same_bytes(par.reshape(-1), p1.reshape(-1), "small parity")
        assert np.array_equal(image, full)
        # one block, in place
        one = bytearray(full[0].tobytes())
        assert c.heal(one, S) == CLEAN and one == full[0].tobytes()
        one[5 * S + 17] ^= 0x01
        assert c.heal(one, S) == 5 and one == full[0].tobytes()
        one[(k + 3) * S + S - 1] ^= 0x01
        assert c.heal(one, S) == k + 3 and one == full[0].tobytes()
        one[5 * S + 17] ^= 0x01
        one[(k + 3) * S + S - 1] ^= 0x01
        two = bytes(one)
        assert c.heal(one, S) == UNKNOWN and one == two  # two damaged shards, m >= 4: untouched
    z = np.load(os.path.join(GOLDEN, "vectors_k10_m4.npz"))
    shards = [bytes(r.tobytes()) for r in z["shards_4099"]]
    e = rsmi.NewErasure(10, 4, 4099)
    assert e.heal(shards) == (CLEAN, shards)
    stale = list(shards)
    stale[12] = bytes(len(shards[12]))
    assert want_verdict(10, 4, np.stack([np.frombuffer(s, dtype=np.uint8) for s in stale])) == 12
    assert e.heal(stale) == (12, shards)
    sw = list(shards)
    sw[3], sw[12] = sw[12], sw[3]
    assert e.heal(sw) == (UNKNOWN, sw)
    e._codec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("S,chunks", [(2048, 0), (2049, 0), (2049, 3)], ids=["2d-copy", "odd", "odd-slot-reuse"])
def test_host_pipeline_pageable(gpu, S, chunks):
    """RS(2,2), pageable buffers, small_call_bytes 0: the upload pipeline, with 2D copies (S a
    multiple of 8) and with linear copies and the repitch kernel (odd S).  The last case has
    3 * chunk + 3 blocks: the fourth chunk takes the first chunk's staging slot, so that slot's
    healed rows must have been copied back before; culprits in the first, last and seam blocks
    of every chunk.  Only the healed rows of the caller's arrays change."""
    torch, rsmi = gpu
    k, m = 2, 2
    chunk = max(1, (64 << 20) // (4 * rsmi.recommended_pitch(S)))
    nb = 3 * chunk + 3 if chunks else 9
    rng = np.random.default_rng(S + nb)
    data = rng.integers(0, 256, size=(nb, k, S), dtype=np.uint8)
    parity = orc.encode_fast(k, m, data, threads=8)
    d0, p0 = data.copy(), parity.copy()
    hit = sorted({b for c0 in range(0, nb, chunk) for b in (c0, c0 + 1, min(c0 + chunk, nb) - 1)} if chunks
                 else {0, 4, nb - 1})
    want = np.full(nb, CLEAN, dtype=np.int32)
    for i, b in enumerate(hit):
        x = i % (k + m)
        (data if x < k else parity)[b, x % k, (i * 211) % S] ^= 1 << (i % 8)
        sh = np.concatenate([data[b], parity[b]])
        want[b] = want_verdict(k, m, sh)
        assert want[b] == x
        assert np.array_equal(want_image(k, m, sh[None], want[b:b + 1])[0], np.concatenate([d0[b], p0[b]]))
    with rsmi.Codec(k, m) as c:
        c.set_option("small_call_bytes", 0)
        got, bad = _host_heal(c, data.ctypes.data, k * S, parity.ctypes.data, m * S, S, nb)
        assert c.last_kernel() == "rs_heal_kernel<K=2,MT=2>"
        assert np.array_equal(np.flatnonzero(got != CLEAN), np.array(hit)), np.flatnonzero(got != CLEAN)
        assert np.array_equal(got, want)
        assert np.array_equal(np.flatnonzero(bad.any(axis=1)), np.array(hit))
        # the image is the original: every culprit row restored, every other byte as it was
        same_bytes(data.reshape(-1), d0.reshape(-1), "pipeline data")
        same_bytes(parity.reshape(-1), p0.reshape(-1), "pipeline parity")
        got, bad = _host_heal(c, data.ctypes.data, k * S, parity.ctypes.data, m * S, S, nb, flags=False)
        assert (got == CLEAN).all()


# ---------------------------------------------------------------- 11: against the existing path
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
def test_image_equals_reconstruct_rows(gpu, aligned):
    """One culprit pattern for the whole batch, which reconstruct_rows_batch_dev can serve: the
    heal's buffer equals the one reconstruct leaves with the culprit marked missing and required."""
    torch, rsmi = gpu
    k, m, S, nb = 10, 4, 4099, 2
    n = k + m
    lay = Lay(rsmi, k, m, S, nb, aligned)
    full = stripes(k, m, S, nb)
    h = torch.cuda.current_stream().cuda_stream
    with rsmi.Codec(k, m) as c:
        for x in (4, k + 1):
            sh = full.copy()
            sh[:, x, 100:3100] ^= 0xFF
            host = lay.fill(sh)
            got, _, healed = run_dev(torch, c, lay, host, label(lay))
            assert got.tolist() == [x, x] == want_verdicts(k, m, sh).tolist()
            d = torch.from_numpy(host).cuda()
            base = d.data_ptr() + lay.off
            c.reconstruct_rows_batch_dev(base, lay.rs, lay.bs, S, nb, [i != x for i in range(n)],
                                         [i == x for i in range(n)], h)
            torch.cuda.synchronize()
            same_bytes(healed, d.cpu().numpy(), ("reconstruct", x))
            same_bytes(healed, lay.fill(full), ("original", x))


# ---------------------------------------------------------------- 12: no side effects
@pytest.mark.gpu
def test_no_side_effects_on_the_other_calls(gpu):
    """The plan cache, the ratio plan (whose slot 0 heal fills) and the scratch are shared: after
    a heal (and after a fallback heal's scratch encodes) the context's encode, reconstruct, verify
    and locate still match the oracle and report their own labels."""
    torch, rsmi = gpu
    for k, m, S, hlabel, llabel, vlabel, elabel, rlabel in (
            (10, 4, 4099, "rs_heal_kernel<K=10,MT=4>", "rs_locate_kernel<K=10,MT=4>", "rs_verify_kernel<K=10,MT=4>",
             "rs_fast_kernel<K=10,MT=4,NT=1>", "rs_fast_kernel<K=10,MT=2,NT=2>"),
            (7, 2, 1025, ROWS, "rs_locate_rows_kernel", "rs_compare_rows_kernel", "rs_generic_kernel<K=7,MT=2>",
             "rs_generic_kernel<K=7,MT=2>")):
        nb = 3
        lay = Lay(rsmi, k, m, S, nb, True)
        full = stripes(k, m, S)
        sh = full.copy()
        sh[1, 2, 1000] ^= 0x77
        want = want_verdicts(k, m, sh)
        assert want.tolist() == [CLEAN, 2, CLEAN]
        with rsmi.Codec(k, m) as c:
            check(torch, c, lay, sh, hlabel, want)
            h = torch.cuda.current_stream().cuda_stream
            host = lay.fill(full)
            lay.rows(host)[:, k:] = 0xEE
            d = torch.from_numpy(host).cuda()
            c.encode_batch_dev(d.data_ptr(), lay.rs, lay.bs, d.data_ptr() + k * lay.rs, lay.rs, lay.bs, S, nb, h)
            torch.cuda.synchronize()
            assert c.last_kernel() == elabel
            assert np.array_equal(d.cpu().numpy(), lay.fill(full))
            lost = [1, k + 1]
            host = lay.fill(full)
            lay.rows(host)[:, lost] = 0xEE
            d = torch.from_numpy(host).cuda()
            c.reconstruct_batch_dev(d.data_ptr(), lay.rs, lay.bs, S, nb, [i not in lost for i in range(k + m)],
                                    False, h)
            torch.cuda.synchronize()
            assert c.last_kernel() == rlabel
            assert np.array_equal(d.cpu().numpy(), lay.fill(full))
            host = lay.fill(sh)
            assert np.array_equal(verify_flags(torch, c, lay, host), want_flags(k, m, sh))
            assert c.last_kernel() == vlabel
            d = torch.from_numpy(host).cuda()
            cul = torch.full((nb,), POISON, dtype=torch.int32, device="cuda")
            c.locate_batch_dev(d.data_ptr(), lay.rs, lay.bs, d.data_ptr() + k * lay.rs, lay.rs, lay.bs, S, nb,
                               cul.data_ptr(), 0, h)
            torch.cuda.synchronize()
            assert c.last_kernel() == llabel
            assert cul.cpu().numpy().tolist() == want.tolist()
            assert np.array_equal(d.cpu().numpy(), host), "locate wrote to the shards"
            check(torch, c, lay, sh, hlabel, want)


# ---------------------------------------------------------------- 13: far offsets
@pytest.mark.gpu
def test_offsets_past_4gib(gpu):
    """Two blocks at block_stride = 2^32 + 256, the culprit in the far block, aligned and shifted
    by one byte (the UA kernel).  Only the rows are touched: a store offset truncated to 32 bits
    would land in the near block, whose rows must come back as they were, like the far block's
    other rows."""
    torch, rsmi = gpu
    if torch.cuda.mem_get_info()[0] < 8 << 30:
        pytest.skip("needs 8 GiB of free device memory")
    k, m, S, nb = 4, 2, 1040, 2
    bs = 2 ** 32 + 256
    rng = np.random.default_rng(3100)
    data = rng.integers(0, 256, size=(nb, k, S), dtype=np.uint8)
    full = np.concatenate([data, np.stack([orc.encode(k, m, data[b]) for b in range(nb)])], axis=1)
    try:
        with rsmi.Codec(k, m) as c:
            d = torch.empty(2 ** 32 + 2 ** 20, dtype=torch.uint8, device="cuda")
            assert 1 + bs + (k + m) * S <= d.numel()
            for off, x in ((0, 1), (0, k + 1), (1, 2), (1, k)):
                sh = full.copy()
                sh[1, x, 1033] ^= 0x10
                sh[1, x, 3] ^= 0x02
                assert want_verdicts(k, m, sh).tolist() == [CLEAN, x]
                for b in range(nb):
                    for i in range(k + m):
                        o = off + b * bs + i * S
                        d[o:o + S].copy_(torch.from_numpy(sh[b, i]))
                cul = torch.full((nb + 2,), POISON, dtype=torch.int32, device="cuda")
                base = d.data_ptr() + off
                c.heal_batch_dev(base, S, bs, base + k * S, S, bs, S, nb, cul.data_ptr(), 0,
                                 torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                assert c.last_kernel() == "rs_heal_kernel<K=4,MT=2>" + ("" if off == 0 else ",UA")
                assert cul.cpu().numpy().tolist() == [CLEAN, x, POISON, POISON]
                for b in range(nb):
                    for i in range(k + m):
                        o = off + b * bs + i * S
                        assert np.array_equal(d[o:o + S].cpu().numpy(), full[b, i]), (off, x, b, i)
            del d
    finally:
        torch.cuda.empty_cache()
