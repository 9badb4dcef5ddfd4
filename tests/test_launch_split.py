"""The launch splits of the five launchers, run in pieces through option launch_units_max, and the
launches at the default cap that are large enough to matter.  Exact, no tolerances.

A launcher cuts a batch into launches of whole blocks once one launch would take more than
launch_units_max tiles (launch_plan, launch_stripe_tiles, a segment of launch_mixed) or units
(launch_plan_crc's matrix-core branch, launch_scrub), and moves every pointer and output on by the
blocks before the piece.  Every case runs a call twice on identical inputs, under the default cap
and under a small one, and compares both runs with the CPU references of the other test modules
(the oracle's encode and reconstruct, crc16_ibm, the definitions of test_locate, test_locate_pair,
test_heal, test_heal_pair, test_scrub, test_mixed_reconstruct), never the two runs with each other.
Outputs lie between guard words and start as garbage.  rsmi_get_stat "split_launches" is the
witness that the call ran in the pieces the test works out from S, the blocks and the cap.

A tile is 1 KiB of every row of a block (tpb per block), a unit 4 tiles (upb per block):
S = 16: tpb 1; S = 1025: tpb 2; S = 4097: tpb 5, upb 2.

  1  encode and reconstruct (launch_plan), RS(5,5) for a two-tile plan
  2  the fused encode + CRC-16: the matrix-core fold (launch_plan_crc: the combine inside and the
     separate combine) and the nibble fold (launch_plan's rec and tail offsets)
  3  verify, locate, locate pair, heal, heal pair (launch_stripe_tiles), scrub (launch_scrub)
  4  the mixed reconstruct's segments, with and without the rebuilt rows' CRC-16
  5  verify and scrub, and the encode and reconstruct with both checksums, from pageable host
     memory past one staging chunk
  6  a coalesced group whose table launch would pass the cap runs per block
  7  at the default cap: a Verify just past 2^32 threads' worth of tiles, the fused encode and scrub
     just past 2^24 units, and the largest grids the cap allows against the device's limits
"""
import ctypes
import threading
import time
import zlib

import numpy as np
import pytest

import oracle_lib as orc
import test_heal
import test_heal_pair
import test_host_pipeline as hp
import test_mixed_reconstruct as mr
from test_crc16 import raw_crc
from test_host_pipeline import Bufs
from test_locate import want_verdicts
from test_locate_pair import want_pairs
from test_named_rows import Halves, Outputs, geometry
from test_scrub import _host_scrub, assert_raws, entries_of, want_entries
from test_verify import stripes, want_flags
from test_verify_host import _ref, _rows, chunk_blocks

DEFAULT_CAP = (1 << 24) - 1
WG = 256                      # threads of a workgroup: 4 waves, one tile each
THREADS_OK = (1 << 32) - 1    # the most threads of one launch: measured once, recorded in DESIGN.md 4.12
CODES = [(10, 4), (4, 2)]
SIZES = [16, 1025, 4097]
NBS = [1, 5, 7]
LAYOUTS = ["aligned", "ua"]
LOST_FILL = 0xEE
TIMES = {}


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    rsmi = pytest.importorskip("rsmi")
    if not torch.cuda.is_available() or rsmi.device_count() == 0:
        pytest.skip("no GPU")
    yield torch, rsmi
    if TIMES:
        print("\nlaunch split: wall seconds of the large launches:", ", ".join("%s %.2f" % kv for kv in TIMES.items()))


def tpb(S):
    return ((S + 15) // 16 + 63) // 64


def upb(S):
    return (tpb(S) + 3) // 4


def blocks_per_launch(cap, per_block):
    return max(1, cap // per_block)


def pieces(nb, cap, per_block):
    return -(-nb // blocks_per_launch(cap, per_block))


def caps(per_block, nb):
    """One block per launch; a cap below one block (still one block per launch, the same as the
    first for per_block = 1); uneven pieces; a last piece of one block; exactly one launch."""
    return sorted({c for c in (1, 2 * per_block, 2 * per_block + 1, per_block * nb - 1, per_block * nb) if c >= 1})


def test_the_shapes_reach_every_piece_pattern():
    assert [tpb(S) for S in SIZES] == [1, 2, 5] and [upb(S) for S in SIZES] == [1, 1, 2]
    seen = set()
    for per_block in (1, 2, 5):
        for nb in NBS:
            for cap in caps(per_block, nb):
                mb = blocks_per_launch(cap, per_block)
                seen.add(tuple(min(mb, nb - s) for s in range(0, nb, mb)))
    assert {(1,) * 5, (1,) * 7, (2, 2, 1), (2, 2, 2, 1), (4, 1), (6, 1), (5,), (7,), (1,)} <= seen
    assert blocks_per_launch(1, 5) == 1 and blocks_per_launch(4, 5) == 1   # a block is never cut
    assert pieces((1 << 26) + 5, DEFAULT_CAP, 1) == 5 and pieces((1 << 24) + 3, DEFAULT_CAP, 1) == 2
    assert default_grids_fit()


def default_grids_fit():
    """The largest grids the default cap can request: a workgroup per unit, or per 4 tiles."""
    return DEFAULT_CAP * WG <= THREADS_OK and -(-DEFAULT_CAP // 4) * WG <= THREADS_OK


class Witness:
    """split_launches around a call."""

    def __init__(self, c):
        self.c, self.at = c, c.stat("split_launches")
        assert self.at >= 0

    def grew(self):
        now = self.c.stat("split_launches")
        d, self.at = now - self.at, now
        return d


def run_twice(c, cap, want_small, run, ctx):
    """run() under the default cap and under cap; the counter grows by want_small under cap, which is
    more than under the default unless cap holds the whole batch."""
    c.set_option("launch_units_max", 0)
    assert c.stat("launch_units_max") == DEFAULT_CAP
    w = Witness(c)
    run(ctx + ("default",))
    base = w.grew()
    c.set_option("launch_units_max", cap)
    assert c.stat("launch_units_max") == cap
    run(ctx + ("cap %d" % cap,))
    small = w.grew()
    c.set_option("launch_units_max", 0)
    assert small == want_small, (ctx, cap, small, want_small)
    assert base >= 1 and (small > base or (small == base and want_small == base)), (ctx, cap, base, small)
    return base


def same_bytes(got, want, ctx):
    if not np.array_equal(got, want):
        at = np.flatnonzero(got != want)
        raise AssertionError("%r: %d bytes differ, first at offset %d: got %#x, want %#x" %
                             (ctx, at.size, at[0], got[at[0]], want[at[0]]))


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def half_rows(buf, off, nb, rows, S, bs, rs):
    return np.lib.stride_tricks.as_strided(buf[off:], shape=(nb, rows, S), strides=(bs, rs, 1))


def halves_after(h, image, ctx):
    """Both allocations of h against their fill with the rows of image (nb, n, S) in place."""
    d_off, d_rs, d_bs, p_off, p_rs, p_bs = h.geo
    wd, wp = h.hd.copy(), h.hp.copy()
    half_rows(wd, d_off, h.nb, h.k, h.S, d_bs, d_rs)[:] = image[:, :h.k]
    half_rows(wp, p_off, h.nb, h.n - h.k, h.S, p_bs, p_rs)[:] = image[:, h.k:]
    same_bytes(h.dd.cpu().numpy(), wd, ctx + ("data half",))
    same_bytes(h.dp.cpu().numpy(), wp, ctx + ("parity half",))


def half_args(h):
    d_off, d_rs, d_bs, p_off, p_rs, p_bs = h.geo
    return (h.dd.data_ptr() + d_off, d_rs, d_bs, h.dp.data_ptr() + p_off, p_rs, p_bs, h.S, h.nb)


# ---------------------------------------------------------------- 1: encode and reconstruct
def encode_tiles(m):
    return -(-m // 4)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,m", CODES + [(5, 5)])
def test_encode(gpu, k, m, layout):
    torch, rsmi = gpu
    with rsmi.Codec(k, m) as c:
        for S in SIZES:
            for nb in NBS:
                full = stripes(k, m, S, nb)
                before = np.array(full)
                before[:, k:] = LOST_FILL
                geo = geometry(rsmi, k, m, S, layout)

                def run(ctx):
                    h = Halves(torch, before, k, geo)
                    c.encode_batch_dev(*half_args(h), stream_of(torch))
                    torch.cuda.synchronize()
                    assert c.last_kernel().startswith("rs_fast_kernel<K=%d," % k), c.last_kernel()
                    halves_after(h, full, ctx)

                for i, cap in enumerate(caps(tpb(S), nb)):
                    c.set_option("waves_per_cu", 1 if (S, nb, i) == (4097, 7, 1) else 0)
                    run_twice(c, cap, encode_tiles(m) * pieces(nb, cap, tpb(S)), run, (k, m, S, nb, layout))
                c.set_option("waves_per_cu", 0)


def lost_sets(k, m):
    """One data row, one parity row, and m rows over data and parity."""
    many = tuple(range(m - 1)) + (k + m - 1,)
    return [(0,), (k,), many]


_REC = {}


def reconstructed(k, m, S, nb, lost):
    """The oracle's reconstruction of every block of stripes() with the rows of lost missing."""
    key = (k, m, S, nb, lost)
    if key not in _REC:
        full = stripes(k, m, S, nb)
        sh = np.array(full)
        sh[:, list(lost)] = LOST_FILL
        out = sh.copy()
        for b in range(nb):
            rc, rec = orc.reconstruct(k, m, sh[b], [i not in lost for i in range(k + m)], False)
            assert rc == 0
            out[b] = rec
        assert np.array_equal(out, full)   # the oracle's encode and its reconstruct agree
        _REC[key] = (sh, out)
    return _REC[key]


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=LAYOUTS)
@pytest.mark.parametrize("k,m", CODES + [(5, 5)])
def test_reconstruct(gpu, k, m, aligned):
    """In place, rows of one buffer (test_mixed_reconstruct.layout: the UA form one byte past an
    aligned base at pitch S); the whole buffer against the oracle's image."""
    torch, rsmi = gpu
    n = k + m
    with rsmi.Codec(k, m) as c:
        for S in SIZES:
            for nb in NBS:
                lay = mr.layout(rsmi, k, m, S, nb, aligned)
                for li, lost in enumerate(lost_sets(k, m)):
                    sh, image = reconstructed(k, m, S, nb, lost)
                    host = lay.fill(sh)
                    expect = host.copy()
                    lay.rows(expect)[:] = image

                    def run(ctx):
                        d = torch.from_numpy(host.copy()).cuda()
                        c.reconstruct_batch_dev(d.data_ptr() + lay.off, lay.rs, lay.bs, S, nb,
                                                [i not in lost for i in range(n)], False, stream_of(torch))
                        torch.cuda.synchronize()
                        assert c.last_kernel().startswith("rs_fast_kernel<K=%d," % k), c.last_kernel()
                        same_bytes(d.cpu().numpy(), expect, ctx)

                    for i, cap in enumerate(caps(tpb(S), nb)):
                        c.set_option("waves_per_cu", 1 if (S, nb, li, i) == (4097, 7, 2, 1) else 0)
                        run_twice(c, cap, -(-len(lost) // 4) * pieces(nb, cap, tpb(S)), run,
                                  (k, m, S, nb, aligned, lost))
                    c.set_option("waves_per_cu", 0)


# ---------------------------------------------------------------- 2: the fused encode + CRC-16
_ENTRIES = {}


def clean_entries(k, m, S, nb):
    key = (k, m, S, nb)
    if key not in _ENTRIES:
        _ENTRIES[key] = want_entries(stripes(k, m, S, nb))
    return _ENTRIES[key]


@pytest.mark.gpu
@pytest.mark.parametrize("fold", [1, 0], ids=["mfma", "nibble"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,m", CODES)
def test_encode_crc(gpu, k, m, layout, fold):
    """fold 1 is cut by units (launch_plan_crc), fold 0 by tiles (launch_plan with the records and,
    UA, the tails).  33 blocks of S = 4097 are 66 units: past the 64 that combine inside the kernel,
    so the pieces' records are read by one combine launch over all blocks."""
    torch, rsmi = gpu
    n = k + m
    per = upb if fold else tpb
    with rsmi.Codec(k, m) as c:
        c.set_option("crc16_fused_fold", fold)
        for S, nb in [(S, nb) for S in SIZES for nb in NBS] + [(4097, 33)]:
            full = stripes(k, m, S, nb)
            entries = clean_entries(k, m, S, nb)
            before = np.array(full)
            before[:, k:] = LOST_FILL
            geo = geometry(rsmi, k, m, S, layout)
            form = {"last": None}

            def run(ctx):
                h = Halves(torch, before, k, geo)
                out = Outputs(torch, nb * n, True, False)
                c.encode_batch_dev_crc(*half_args(h), out.ptr(0), stream_of(torch))
                torch.cuda.synchronize()
                form["last"] = c.last_kernel()
                halves_after(h, full, ctx)
                raws = out.read((nb, n))[0]
                assert (raws >> 16 == 0).all(), ctx
                assert np.array_equal(entries_of(rsmi, raws, S), entries), ctx
                if S <= 2048:
                    assert raws[nb - 1, n - 1] == raw_crc(full[nb - 1, n - 1].tobytes()), ctx

            cs = caps(per(S), nb) if nb < 33 else [2 * per(S) * 5 + 1, per(S) * nb - 1]
            for i, cap in enumerate(cs):
                c.set_option("waves_per_cu", 1 if (S, nb, i) == (4097, 7, 1) else 0)
                run_twice(c, cap, pieces(nb, cap, per(S)), run, (k, m, S, nb, layout, fold))
                if fold:
                    assert form["last"].startswith("rs_fused_mfma_kernel"), form
                    assert (",INL" in form["last"]) == (nb * upb(S) <= 64), (form, nb, S)
                else:
                    assert ",CRC" in form["last"], form
            c.set_option("waves_per_cu", 0)


# ---------------------------------------------------------------- 3: the stripe calls
PASSES = {  # kernel launches of a call that launch_stripe_tiles (or launch_scrub) cuts: m >= 3, m == 2
    "verify": (1, 1), "scrub": (1, 1), "locate": (1, 1), "locate_pair": (2, 1), "heal": (2, 2), "heal_pair": (3, 2)}
WORDS = {"verify": 0, "locate": 1, "heal": 1, "locate_pair": 2, "heal_pair": 2}


def dirty_blocks(nb, mb):
    """The first and last block of every piece of mb blocks but one piece, which stays clean, and a
    block in the middle; of a lone piece its first, last and middle block."""
    ps = [list(range(s, min(s + mb, nb))) for s in range(0, nb, mb)]
    if len(ps) == 1:
        return tuple(sorted({0, nb // 2, nb - 1}))
    out = set()
    for i, p in enumerate(ps):
        if i != 1:
            out |= {p[0], p[-1]}
    if nb // 2 not in ps[1]:
        out.add(nb // 2)
    return tuple(sorted(out))


_CASES = {}


def damaged_shard(b, n):
    return (5 * b + 1) % n


def stripe_case(k, m, S, nb, dirty, pairs):
    """Stored shards with one damaged shard per dirty block (a different shard from block to block,
    so a result that lands in another block's place is seen), with pairs a second one in every
    other dirty block; and the definitions' answers, computed once."""
    key = (k, m, S, nb, dirty, pairs)
    if key not in _CASES:
        n = k + m
        sh = np.array(stripes(k, m, S, nb))
        for i, b in enumerate(dirty):
            x = damaged_shard(b, n)
            sh[b, x, S - 1 if b % 2 else (131 * b) % S] ^= 0x40
            if pairs and i % 2 == 0:
                sh[b, (x + 5) % n, (977 * (b + 1)) % S] ^= 0x09
        sh.setflags(write=False)
        case = {"sh": sh, "flags": want_flags(k, m, sh), "entries": want_entries(sh)}
        assert np.array_equal(case["flags"].any(axis=1), np.isin(np.arange(nb), dirty))
        case["locate"] = want_verdicts(k, m, sh)
        case["heal"] = case["locate"]
        case["heal_image"] = test_heal.want_image(k, m, sh, case["locate"])
        case["locate_pair"] = want_pairs(k, m, sh)
        case["heal_pair"] = case["locate_pair"]
        case["heal_pair_image"] = test_heal_pair.want_image(k, m, sh, case["locate_pair"])
        if not pairs:   # the one damaged shard is what the definition names
            assert case["locate"][list(dirty)].tolist() == [damaged_shard(b, n) for b in dirty]
        _CASES[key] = case
    return _CASES[key]


def stripe_call(torch, rsmi, c, call, case, k, geo, ctx):
    sh = case["sh"]
    nb, n, S = sh.shape
    m = n - k
    h = Halves(torch, sh, k, geo)
    bad = Outputs(torch, nb * m, True, False)
    W = n if call == "scrub" else WORDS[call]
    words = Outputs(torch, nb * W, True, False) if W else None
    args, st = half_args(h), stream_of(torch)
    if call == "verify":
        c.verify_batch_dev(*args, bad.ptr(0), st)
    elif call == "scrub":
        c.scrub_batch_dev(*args, bad.ptr(0), words.ptr(0), st)
    else:
        getattr(c, call + "_batch_dev")(*args, words.ptr(0), bad.ptr(0), st)
    torch.cuda.synchronize()
    flags = bad.read((nb, m))[0] != 0
    assert np.array_equal(flags, case["flags"]), (ctx, np.argwhere(flags != case["flags"]))
    if call == "scrub":
        raws = words.read((nb, n))[0]
        assert (raws >> 16 == 0).all(), ctx
        got = entries_of(rsmi, raws, S)
        assert np.array_equal(got, case["entries"]), (ctx, np.argwhere(got != case["entries"]))
    elif W:
        got = words.read((nb, W))[0].astype(np.int32).reshape(case[call].shape)
        assert np.array_equal(got, case[call]), (ctx, got.tolist(), case[call].tolist())
    halves_after(h, case[call + "_image"] if call.startswith("heal") else sh, ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("call", list(PASSES))
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,m", CODES)
def test_stripe_calls(gpu, k, m, layout, call):
    torch, rsmi = gpu
    per = upb if call == "scrub" else tpb
    passes = PASSES[call][0 if m >= 3 else 1]
    pairs = call in ("locate_pair", "heal_pair") and m >= 3
    with rsmi.Codec(k, m) as c:
        for S in SIZES:
            geo = geometry(rsmi, k, m, S, layout)
            for nb in NBS:
                for i, cap in enumerate(caps(per(S), nb)):
                    dirty = dirty_blocks(nb, blocks_per_launch(cap, per(S)))
                    case = stripe_case(k, m, S, nb, dirty, pairs)
                    c.set_option("waves_per_cu", 1 if (S, nb, i) == (4097, 7, 1) else 0)
                    run_twice(c, cap, passes * pieces(nb, cap, per(S)),
                              lambda ctx: stripe_call(torch, rsmi, c, call, case, k, geo, ctx),
                              (call, k, m, S, nb, layout))
                c.set_option("waves_per_cu", 0)


def test_damage_leaves_a_piece_clean():
    for nb in NBS:
        for mb in range(1, nb + 1):
            d = dirty_blocks(nb, mb)
            ps = [list(range(s, min(s + mb, nb))) for s in range(0, nb, mb)]
            if len(ps) > 1:
                assert not set(ps[1]) & set(d)
                assert all(p[0] in d and p[-1] in d for i, p in enumerate(ps) if i != 1)
                assert nb // 2 in d or nb // 2 in ps[1]
            else:
                assert {0, nb // 2, nb - 1} == set(d)


# ---------------------------------------------------------------- 4: the mixed reconstruct
def mixed_launches(k, S, cap, present, W):
    """launch_mixed's class launches: per segment one for every number of rows (1..4) that a block
    of the segment with enough rows present rebuilds."""
    nb = present.shape[0]
    seg = min(blocks_per_launch(cap, tpb(S)), 1 << 22)
    total = 0
    for s0 in range(0, nb, seg):
        rows = {int(W[b].sum()) for b in range(s0, min(s0 + seg, nb)) if present[b].sum() >= k}
        total += len(rows - {0})
    return total


@pytest.mark.gpu
@pytest.mark.parametrize("crcs", [0, 16, 32], ids=["rows", "rows+crc16", "rows+crc32"])
@pytest.mark.parametrize("aligned", [True, False], ids=LAYOUTS)
@pytest.mark.parametrize("k,m", CODES)
def test_mixed_reconstruct(gpu, k, m, aligned, crcs):
    """Every block its own pattern (rs42_losses: 23 blocks; rs104_losses: 23 blocks of 1..4 lost
    rows), so a segment's base, its list entries and its rows' words all depend on the cut.  With one
    checksum output (the other NULL) the segment's offset into that output is live as well: R(row)
    against crc16_ibm, R32(row) against zlib.crc32 through crc32_entry, zero wherever nothing was
    rebuilt."""
    torch, rsmi = gpu
    n = k + m
    losses = mr.rs42_losses() if (k, m) == (4, 2) else mr.rs104_losses(23, 7)
    nb = len(losses)
    present = mr.present_of(n, losses)
    W = mr.wanted(k, present, None, False)
    with rsmi.Codec(k, m) as c:
        for S in SIZES:
            lay = mr.layout(rsmi, k, m, S, nb, aligned)
            sh = mr.stored(stripes(k, m, S, nb), present)
            want_status, image = mr.definition(k, m, sh, present, W)
            rebuilt = W & (np.array(want_status) == 0)[:, None]
            if crcs == 16:
                want_sums = np.where(rebuilt, want_entries(image), 0)
            elif crcs == 32:
                want_sums = np.where(rebuilt, [[zlib.crc32(r.tobytes()) for r in blk] for blk in image], 0)

            def run(ctx):
                if not crcs:
                    mr.check(torch, c, lay, sh, present, None, False, None)
                    return
                host = lay.fill(sh)
                d = torch.from_numpy(host.copy()).cuda()
                out = Outputs(torch, nb * n, crcs == 16, crcs == 32)
                got = c.reconstruct_mixed_batch_dev_crcs(d.data_ptr() + lay.off, lay.rs, lay.bs, S, nb, mr.u8(present),
                                                         None, False, out.ptr(0), out.ptr(1), stream_of(torch))
                torch.cuda.synchronize()
                assert got == want_status, ctx
                expect = host.copy()
                lay.rows(expect)[:] = image
                same_bytes(d.cpu().numpy(), expect, ctx)
                raws = out.read((nb, n))[0 if crcs == 16 else 1]
                assert (raws[~rebuilt] == 0).all(), ctx
                if crcs == 16:
                    sums = entries_of(rsmi, raws, S)
                else:
                    sums = np.array([[rsmi.crc32_entry(b"", int(x), S) for x in row] for row in raws], dtype=np.uint32)
                assert np.array_equal(np.where(rebuilt, sums, 0), want_sums), (ctx, np.argwhere(np.where(rebuilt, sums, 0) != want_sums)[:4])

            for i, cap in enumerate(caps(tpb(S), nb)):
                assert S == 16 or blocks_per_launch(cap, tpb(S)) < nb or cap == tpb(S) * nb
                c.set_option("waves_per_cu", 1 if (S, i) == (4097, 1) else 0)
                run_twice(c, cap, mixed_launches(k, S, cap, present, W), run, (k, m, S, aligned, crcs))
            c.set_option("waves_per_cu", 0)


# ---------------------------------------------------------------- 5: host paths past one chunk
def host_case(rsmi, k, m, S, per_launch):
    """One block more than a staging chunk and one more, with damage around the chunk seam and
    around the launches' seams inside the first chunk: (nb, blocks hit)."""
    ch = chunk_blocks(k, m, S)
    nb = ch + 2
    assert nb * (k + m) * S > (2 << 20)    # not the small call
    assert 2 * per_launch < ch             # the first chunk runs in three launches or more
    hit = sorted({0, per_launch - 1, per_launch, 2 * per_launch - 1, 2 * per_launch, ch - 1, ch, nb - 1})
    return ch, nb, hit


@pytest.mark.gpu
@pytest.mark.parametrize("call", ["verify", "scrub"])
def test_host_pipeline_past_one_chunk(gpu, call):
    """RS(4,2), S = 1025, pageable: the upload pipeline's chunk of 5461 blocks and two blocks on the
    next staging slot, each chunk cut into launches of 2000 blocks, so a result's place is the sum
    of the chunk's first block and the launch's.  Blocks between the seams stay clean."""
    torch, rsmi = gpu
    k, m, S, per_launch = 4, 2, 1025, 2000
    ch, nb, hit = host_case(rsmi, k, m, S, per_launch)
    per = upb(S) if call == "scrub" else tpb(S)
    cap = per_launch * per + (per - 1)
    assert blocks_per_launch(cap, per) == per_launch
    data, par = _ref(k, m, S, nb)
    bufs = Bufs(rsmi)
    dptr, dbuf = bufs.full(nb * k * S, 0, False)
    pptr, pbuf = bufs.full(nb * m * S, 0, False)
    _rows(dbuf, nb, k, S, k * S)[:] = data
    prows = _rows(pbuf, nb, m, S, m * S)
    prows[:] = par
    want = np.zeros((nb, m), dtype=bool)
    for i, b in enumerate(hit):
        assert np.array_equal(orc.encode(k, m, data[b]), par[b]), b
        prows[b, i % m, (i * 211 + b) % S] ^= 1 << (i % 8)
        want[b, i % m] = True
    d0, p0 = dbuf.copy(), pbuf.copy()
    with rsmi.Codec(k, m) as c:
        def run(ctx):
            if call == "verify":
                bad = np.full(nb * m, 0x5EED, dtype=np.uint32)
                c.verify_batch_host_ptr(dptr, k * S, pptr, m * S, S, nb, bad.ctypes.data)
                flags = bad.reshape(nb, m) != 0
            else:
                flags, raws = _host_scrub(c, dptr, k * S, pptr, m * S, S, nb)
                sample = sorted(set(hit) | {1, per_launch + 1, ch + 1})
                stored = np.concatenate([_rows(dbuf, nb, k, S, k * S), prows], axis=1)
                assert_raws(rsmi, raws[sample], stored[sample], ctx)
                assert (raws >> 16 == 0).all()
            assert np.array_equal(np.argwhere(flags), np.argwhere(want)), (ctx, np.argwhere(flags)[:16])
            assert np.array_equal(dbuf, d0) and np.array_equal(pbuf, p0), ctx

        run_twice(c, cap, pieces(ch, cap, per) + pieces(nb - ch, cap, per), run, (call, "host"))
        assert pieces(ch, cap, per) == 3


@pytest.mark.gpu
@pytest.mark.parametrize("call", ["encode", "reconstruct_rows"])
def test_host_crcs_pipeline_past_one_chunk(gpu, call):
    """rsmi_encode_batch_host_crcs and rsmi_reconstruct_rows_batch_host_crcs, RS(4,2), S = 2049 (3
    tiles), pageable, both checksum outputs: a chunk of 2730 blocks and two blocks on the next
    staging slot, each chunk's launch_plan cut into launches of 1000 blocks beside the per-chunk
    offsets of the rows and of both checksum buffers.  The buffers whole and the checksums of the
    blocks around every seam against the oracle (test_host_pipeline's cases and checks)."""
    torch, rsmi = gpu
    k, m, S, per_launch = 4, 2, 2049, 1000
    n = k + m
    ch = hp.chunk_blocks(k, m, S)
    nb = ch + 2
    assert ch == 2730 and tpb(S) == 3 and nb * n * S > (2 << 20)
    cap = per_launch * tpb(S) + 2
    assert blocks_per_launch(cap, tpb(S)) == per_launch and pieces(ch, cap, tpb(S)) == 3
    ref = hp._ref(k, m, S, nb)
    seams = sorted({b for s in (per_launch, 2 * per_launch, ch) for b in (s - 1, s)} | {0, nb - 1})
    bufs = Bufs(rsmi)
    with rsmi.Codec(k, m) as c:
        if call == "encode":
            case = hp.EncodeCase(rsmi, bufs, ref, nb)

            def run(ctx):
                case.call(c, True, True, hp.fast_label(k, m), chunk=per_launch)
        else:
            case = hp.ReconstructCase(rsmi, bufs, ref, nb)
            lost, required = [1, 5], [1, 5]    # a data row and a parity row, both rebuilt
            present = [i not in lost for i in range(n)]

            def run(ctx):
                case.lose(lost)
                raw16 = np.full((nb, n), 0xA5A5A5A5, dtype=np.uint32)
                raw32 = np.full((nb, n), 0xA5A5A5A5, dtype=np.uint32)
                c.reconstruct_rows_batch_host_crcs_ptr(case.ptr, case.bs, S, nb, present, [i in required for i in range(n)],
                                                       raw16.ctypes.data, raw32.ctypes.data)
                assert c.last_kernel() == hp.fast_label(k, len(required)), c.last_kernel()
                case.check(lost, required, ctx)
                others = [i for i in range(n) if i not in required]
                assert (raw16[:, others] == 0).all() and (raw32[:, others] == 0).all(), ctx
                assert (raw16[:, required] < 0x10000).all(), ctx
                hp._check_crcs(rsmi, ref, raw16, raw32, sorted(set(seams) | set(hp.sampled_blocks(nb, per_launch))),
                               required, required, ctx)

        run_twice(c, cap, pieces(ch, cap, tpb(S)) + pieces(nb - ch, cap, tpb(S)), run, (call, "host crcs"))


# ---------------------------------------------------------------- 6: the table launch
@pytest.mark.gpu
@pytest.mark.parametrize("flag", [1, 0], ids=["flag", "no-flag"])
@pytest.mark.parametrize("crc", [True, False], ids=["crc16", "plain"])
def test_table_launch_over_the_cap_runs_per_block(gpu, crc, flag):
    """A coalesced group of 12 requests in page-locked buffers is one launch over a table of the
    blocks' bases.  A table is never cut (its entries are bases, not a range): when the group's
    units (fused encode + CRC-16) or tiles (plain encode) pass the cap, the table form declines and
    the group runs a launch per block; at a cap that holds the group it is the table launch again.
    Every shard and R(shard) is the oracle's either way.  The requests come in through
    rsmi_encode_block_coalesced_crcs with raw32_out NULL (rsmi_encode_block_coalesced is that call);
    a request that asks for R32 as well keeps its group off the table forms altogether."""
    torch, rsmi = gpu
    k, m, B, T = 4, 2, 4099, 12
    n, S = k + m, (B + k - 1) // k
    assert S == 1025
    group = T * (upb(S) if crc else tpb(S))
    L = rsmi.lib()
    rng = np.random.default_rng(B + T)
    blocks = [bytes(rng.integers(0, 256, size=B, dtype=np.uint8)) for _ in range(T)]
    want = []
    for b in blocks:
        w = orc.split(k, m, b)
        w[k:] = orc.encode(k, m, w[:k])
        want.append(w)
    ptrs = [L.rsmi_host_alloc(n * S) for _ in range(T)]
    assert all(ptrs)
    try:
        views = [np.ctypeslib.as_array((ctypes.c_uint8 * (n * S)).from_address(p)).reshape(n, S) for p in ptrs]
        with rsmi.Codec(k, m) as c:
            c.set_option("coalesce_lanes", 1)
            c.set_option("coalesce_us", 100000)
            c.set_option("coalesce_max", T)
            c.set_option("coalesce_flag", flag)
            c.warm()
            for cap, table in ((0, True), (group - 1, False), (group, True), (1, False)):
                c.set_option("launch_units_max", cap)
                raws = [(ctypes.c_uint32 * n)() for _ in range(T)]
                rcs = [None] * T
                for t in range(T):
                    flat = views[t].reshape(-1)
                    flat[:] = 0xA5
                    flat[:B] = np.frombuffer(blocks[t], dtype=np.uint8)

                def enc(t):
                    rcs[t] = L.rsmi_encode_block_coalesced_crcs(c._h, ptrs[t], B, ptrs[t], raws[t] if crc else None, None)

                w, b0 = Witness(c), c.stat("coalesced_batches")
                th = [threading.Thread(target=enc, args=(t,)) for t in range(T)]
                for x in th:
                    x.start()
                for x in th:
                    x.join()
                assert rcs == [0] * T, (cap, rcs)
                assert c.stat("coalesced_batches") - b0 == 1
                assert (",TB" in c.last_kernel()) == table, (cap, c.last_kernel())
                assert w.grew() == (1 if table else T), cap
                for t in range(T):
                    assert np.array_equal(views[t], want[t]), (cap, t)
                    for r in range(n if crc else 0):
                        assert rsmi.crc16_entry(b"", raws[t][r], S) == orc.crc16_ibm(want[t][r].tobytes()), (cap, t, r)
    finally:
        for p in ptrs:
            L.rsmi_host_free(p)


# ---------------------------------------------------------------- 7: the large launches at the default cap
PERIOD = 4096


def need_memory(torch, gib=16):
    free, _ = torch.cuda.mem_get_info()
    if free < gib << 30:
        pytest.skip("less than %d GiB of device memory free" % gib)


def tiled(torch, period, nb):
    """nb blocks on the device: period (PERIOD, bytes per block) repeated."""
    d = torch.from_numpy(np.array(period)).cuda().repeat(-(-nb // PERIOD), 1)[:nb]
    assert d.is_contiguous() and d.shape[0] == nb
    return d


def equals_tiled(torch, got, period):
    """got (nb, w) on the device equals period (PERIOD, w) repeated: the blocks that differ."""
    nb = got.shape[0]
    full = nb // PERIOD * PERIOD
    bad = []
    step = 1024 * PERIOD
    for s in range(0, full, step):
        e = min(s + step, full)
        ne = (got[s:e].view(-1, PERIOD, got.shape[1]) != period[None]).any(dim=2)
        if bool(ne.any()):
            bad += (torch.nonzero(ne.view(-1)).flatten()[:8] + s).tolist()
    if nb > full:
        ne = (got[full:] != period[:nb - full]).any(dim=1)
        bad += (torch.nonzero(ne).flatten() + full).tolist()
    return bad


@pytest.mark.gpu
def test_verify_past_2_32_threads_of_tiles(gpu):
    """RS(4,2), S = 16, rows at pitch 16: 2^26 + 5 blocks are as many tiles, which one launch would
    run in 2^24 + 2 workgroups, 2^32 + 512 threads.  Under the default cap it is 5 launches.  (In
    one launch, under the cap of 2^31 that came before, the MI355X runtime wrapped the thread count
    at 2^32: two workgroups strode over every tile and gave the same flags after 10.6 s; the 2^26 - 4
    blocks that fit below 2^32 threads took 0.03 s.  DESIGN.md 4.12.)"""
    torch, rsmi = gpu
    need_memory(torch)
    k, m, S = 4, 2, 16
    nb = (1 << 26) + 5
    period = np.ascontiguousarray(stripes(k, m, S, PERIOD)).reshape(PERIOD, 6 * S)
    t0 = time.perf_counter()
    d = tiled(torch, period, nb)
    hits = [0, (1 << 26) - 1, 1 << 26, (1 << 26) + 4]
    for i, b in enumerate(hits):
        d[b, k * S + (i % m) * S + 3 * i] ^= 0x10
        blk = d[b].cpu().numpy().reshape(1, 6, S)
        assert want_flags(k, m, blk)[0].tolist() == [j == i % m for j in range(m)]
    bad = torch.full((nb * m + 2,), 0x5EED, dtype=torch.int32, device="cuda")
    with rsmi.Codec(k, m) as c:
        w = Witness(c)
        c.verify_batch_dev(d.data_ptr(), S, 6 * S, d.data_ptr() + k * S, S, 6 * S, S, nb, bad.data_ptr(), stream_of(torch))
        torch.cuda.synchronize()
        assert c.last_kernel() == "rs_verify_kernel<K=4,MT=2>"
        assert w.grew() == pieces(nb, DEFAULT_CAP, 1) == 5
    assert bad[nb * m:].tolist() == [0x5EED] * 2
    got = torch.nonzero(bad[:nb * m]).flatten().tolist()
    assert got == [b * m + i % m for i, b in enumerate(hits)], got
    TIMES["verify 2^26+5"] = time.perf_counter() - t0


@pytest.mark.gpu
def test_fused_encode_and_scrub_past_2_24_units(gpu):
    """RS(4,2), S = 16: 2^24 + 3 blocks are as many units, a workgroup each: 2^32 + 768 threads in
    one launch, two launches under the default cap.  The parity and the raws of every block against
    the oracle's period, then the scrub of the result with block 2^24 damaged.  (In one launch, under
    the cap of 2^31 that came before, the MI355X runtime wrapped the thread count at 2^32: three
    workgroups coded blocks 0..2, every later block kept its stale parity and raws, and both calls
    returned OK.  DESIGN.md 4.12.)"""
    torch, rsmi = gpu
    need_memory(torch)
    k, m, S = 4, 2, 16
    n = k + m
    nb = (1 << 24) + 3
    full = stripes(k, m, S, PERIOD)
    raw_period = np.array([[raw_crc(full[b, r].tobytes()) for r in range(n)] for b in range(PERIOD)], dtype=np.int32)
    assert np.array_equal(entries_of(rsmi, raw_period.astype(np.uint32), S), want_entries(full))
    t0 = time.perf_counter()
    before = np.array(full)
    before[:, k:] = LOST_FILL
    d = tiled(torch, before.reshape(PERIOD, n * S), nb)
    period = torch.from_numpy(np.array(full).reshape(PERIOD, n * S)).cuda()
    raws_want = torch.from_numpy(raw_period).cuda()
    raw = torch.full((nb, n), 0x7EA5, dtype=torch.int32, device="cuda")
    args = (d.data_ptr(), S, n * S, d.data_ptr() + k * S, S, n * S, S, nb)
    with rsmi.Codec(k, m) as c:
        w = Witness(c)
        c.encode_batch_dev_crc(*args, raw.data_ptr(), stream_of(torch))
        torch.cuda.synchronize()
        assert c.last_kernel() == "rs_fused_mfma_kernel<K=4,MT=2,NT=1>", c.last_kernel()
        assert w.grew() == pieces(nb, DEFAULT_CAP, 1) == 2
        assert equals_tiled(torch, d, period) == []
        assert equals_tiled(torch, raw, raws_want) == []
        TIMES["fused encode 2^24+3"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        hit = 1 << 24
        d[hit, 2 * S + 5] ^= 0x21
        blk = d[hit].cpu().numpy().reshape(1, n, S)
        assert want_flags(k, m, blk)[0].all()
        bad = torch.full((nb * m,), 0x5EED, dtype=torch.int32, device="cuda")
        raw.fill_(0x7EA5)
        c.scrub_batch_dev(*args, bad.data_ptr(), raw.data_ptr(), stream_of(torch))
        torch.cuda.synchronize()
        assert c.last_kernel() == "rs_scrub_mfma_kernel<K=4,MT=2>", c.last_kernel()
        assert w.grew() == 2
        assert torch.nonzero(bad).flatten().tolist() == [hit * m, hit * m + 1]
        assert equals_tiled(torch, raw, raws_want) == [hit]
        got = raw[hit].cpu().numpy().astype(np.uint32)
        assert got.tolist() == [raw_crc(blk[0, r].tobytes()) for r in range(n)]
    TIMES["scrub 2^24+3"] = time.perf_counter() - t0


def loaded_hip():
    """The HIP runtime this process already has loaded."""
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    assert paths, "no libamdhip64 is loaded"
    return [ctypes.CDLL(p) for p in paths]


@pytest.mark.gpu
def test_grid_limits(gpu):
    """The largest grid the default cap can request fits the device's maximum grid x, and its threads
    stay below 2^32.  That bound is not observed by this suite, whose launches are all smaller: it
    is the measurement recorded in DESIGN.md 4.12, taken once with one launch per call (2^24 - 1
    units and 2^26 - 4 tiles were right and fast; 2^24 + 3 units lost all but three, 2^26 + 5 tiles
    took 300 times as long).  The MI355X
    reports a maximum grid x of 2^31 - 1, which a unit launch of exactly 2^31 units (the cap before
    this one, with a power-of-two number of units per block) would have passed by one.
    hipDeviceAttributeMaxGridDimX is 29 in hipDeviceAttribute_t, behind MaxBlockDimX, Y, Z."""
    torch, rsmi = gpu
    torch.zeros(1, device="cuda")
    def attr(i):
        got = set()
        for hip in loaded_hip():
            v = ctypes.c_int(0)
            assert hip.hipDeviceGetAttribute(ctypes.byref(v), i, torch.cuda.current_device()) == 0
            got.add(v.value)
        assert len(got) == 1, got
        return got.pop()

    assert [attr(i) for i in (26, 27, 28)] == [1024, 1024, 1024]   # MaxBlockDimX, Y, Z: the enum is where it was
    max_x, max_y, max_z = attr(29), attr(30), attr(31)
    print("\nmaximum grid: x %d, y %d, z %d" % (max_x, max_y, max_z))
    assert max_x >= 65535 and max_y >= 65535 and max_z >= 65535
    with rsmi.Codec(4, 2) as c:
        cap = c.stat("launch_units_max")
    assert cap == DEFAULT_CAP
    unit_grid, tile_grid = cap, -(-cap // 4)
    assert unit_grid <= max_x and tile_grid <= max_x
    assert unit_grid * WG <= THREADS_OK and tile_grid * WG <= THREADS_OK
