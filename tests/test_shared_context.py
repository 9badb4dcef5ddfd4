"""Every device entry point interleaved on one long-lived context.

The family modules open a fresh Codec, run one family on it, drain the device and close it.  A
Dag Node keeps one context for its lifetime and sends it a ragged encode, a mixed reconstruct with
checksums and a scrub, locate, heal, verify loop back to back, from several threads and streams.
The state those calls share inside the context (DESIGN.md 4.15 lists it) is crossed here by two
different families with nothing drained between them: the mixed_words head that the mixed
reconstruct and the ragged encode both move, the per-stream locate, verify, scrub and mixed-verify
scratch, the fused encode's records and unit counters, the CRC tables and the cached CRC-32 end
shift built on first use, the plan map, the fold geometry and the options read at launch.

The harness is test_stream_order's (poisoned buffers, a producer behind the gate, a consumer that
clones then fills, whole-buffer compares, nothing written after the consumer).  Every expected value
comes from the CPU references of the family modules (oracle_lib's encode and reconstruct, crc16_ibm,
zlib, want_flags, want_verdicts, want_pairs, the heal images, the mixed definition), never from a
second run of the library.  Everything is bit-exact.

Codes RS(10,4) and RS(4,2); S in {16, 1025, 4097}: 1 tile, 2 tiles, 5 tiles = 2 units with a
one-byte last chunk; 1 to 7 blocks a call (33 where the fused encode has to take its two-launch
form); the aligned layout and the unaligned-window one.  Damage for locate and heal is one byte in
a row's last 16-byte chunk, in a block that is neither first nor last.

  0  (CPU) the constants leg 3 rests on, read from rsmi_mixed.cpp and rs_plan.hpp; the seeds of
     leg 7 draw every builder twice and every neighbour pair of leg 1
  S  every new builder alone on a fresh context, behind the gate
  1  all families back to back on one stream behind one gate, none of them waiting
  2  first use (tables, plans, scratch) behind pending kernels of another family
  3  mixed_words starts over and regrows while calls of the other family are pending
  4  options changed between queued launches of different families; split_launches the witness
  5  two streams, the families crossed in opposite orders
  6  four host threads, a family and a stream each, five rounds
  7  seeded random interleave of every builder over two streams
  8  the host entry points of every family alternating over one staging, small, large, small

There is no rsmi_encode_batch_dev form with both checksums (the CRC-32 of an encode comes from the
rows passes), so the builders are twelve new ones beside test_stream_order's four; the named rows
and rows-pass builders carry the CRC-32.
"""
import os
import re
import threading
import time
import zlib

import numpy as np
import pytest

import oracle_lib as orc
import test_heal
import test_heal_pair
import test_mixed_crcs as mc
import test_mixed_reconstruct as mr
import test_mixed_verify as mv
from test_kernel_matrix import fused_label
from test_launch_split import DEFAULT_CAP, PASSES, half_rows, pieces, tpb, upb
from test_locate import want_verdicts
from test_locate_pair import want_pairs
from test_named_rows import PAD, assert_named, geometry, refs_of
from test_ragged_encode import FALLBACK, Batch, segment_launches
from test_scrub import entries_of, want_entries
from test_stream_order import (M32, POISON_RAW, Bytes, Call, Gate, Raw, _full, _rows_data, crc_rows_call, encode_call,
                               reconstruct_call, run_plan, warm_then_gated)
from test_verify import want_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "filedag-storage_amd", "csrc")
CODES = [(10, 4), (4, 2)]
SIZES = [16, 1025, 4097]
LAYOUTS = ["aligned", "ua"]
TAIL = 32                      # guard bytes behind the last row of a half
FLOOR = 1 << 20                # mixed_words' first size (the CPU leg pins it)
RAGGED_DESC, RAGGED_UNIT, MIXED_ENTRY = 64, 8, 8   # sizeof RaggedBlockDev, RaggedUnit, MixedEntry (the CPU leg pins them)
WALL = {}


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    rsmi = pytest.importorskip("rsmi")
    if not torch.cuda.is_available() or rsmi.device_count() == 0:
        pytest.skip("no GPU")
    gate = Gate(torch)
    yield torch, rsmi, gate
    print("\nshared context: wall seconds per leg:", ", ".join("%s %.2f" % kv for kv in sorted(WALL.items())))


class _leg:
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.t0 = time.perf_counter()

    def __exit__(self, *a):
        WALL[self.name] = WALL.get(self.name, 0.0) + time.perf_counter() - self.t0


# ---------------------------------------------------------------- shared pieces of the builders
def round16(x):
    return (x + 15) // 16 * 16


def damaged(rng, full):
    """full with one byte changed in the last 16-byte chunk of one row of a block that is neither
    first nor last; batches of fewer than three blocks stay clean."""
    sh = np.array(full)
    nb, n, S = sh.shape
    if nb >= 3:
        b, x = int(rng.integers(1, nb - 1)), int(rng.integers(0, n))
        sh[b, x, int(rng.integers((S - 1) // 16 * 16, S))] ^= int(rng.integers(1, 256))
    return sh


class HalfBufs:
    """Data and parity rows in two guarded allocations laid out by test_named_rows.geometry (aligned:
    rows at recommended_pitch with gaps between the blocks; ua: rows back to back at pitch S from an
    odd base), the rows of sh going in and the rows of image expected back, everything else PAD."""

    def __init__(self, torch, rsmi, c, sh, layout, image=None):
        nb, n, S = sh.shape
        k = c.k
        self.geo = geometry(rsmi, k, c.m, S, layout)
        d_off, d_rs, d_bs, p_off, p_rs, p_bs = self.geo
        hd = np.full(d_off + (nb - 1) * d_bs + (k - 1) * d_rs + S + TAIL, PAD, dtype=np.uint8)
        hp = np.full(p_off + (nb - 1) * p_bs + (n - k - 1) * p_rs + S + TAIL, PAD, dtype=np.uint8)
        wd, wp = hd.copy(), hp.copy()
        image = sh if image is None else image
        for bufd, bufp, rows in ((hd, hp, sh), (wd, wp, image)):
            half_rows(bufd, d_off, nb, k, S, d_bs, d_rs)[:] = rows[:, :k]
            half_rows(bufp, p_off, nb, n - k, S, p_bs, p_rs)[:] = rows[:, k:]
        self.d, self.p = Bytes(torch, hd, wd), Bytes(torch, hp, wp)
        self.S, self.nb = S, nb

    def args(self):
        d_off, d_rs, d_bs, p_off, p_rs, p_bs = self.geo
        return (self.d.dev.data_ptr() + d_off, d_rs, d_bs, self.p.dev.data_ptr() + p_off, p_rs, p_bs, self.S, self.nb)


def _spare(r, ctx):
    assert r[-1] == POISON_RAW, ctx + ("the slot past the output was written",)
    return r[:-1]


def flags_raw(torch, want):
    """nb * m flag words and a spare slot; want (nb, m) bool."""
    def check(r, ctx):
        got = _spare(r, ctx).reshape(want.shape) != 0
        assert np.array_equal(got, want), ctx + ("flags", np.argwhere(got != want)[:4].tolist())
    return Raw(torch, (want.size + 1,), check)


def words_raw(torch, want):
    """int32 verdict words and a spare slot."""
    w = np.asarray(want, dtype=np.int64).reshape(-1) & M32

    def check(r, ctx):
        got = _spare(r, ctx)
        assert np.array_equal(got, w), ctx + ("verdicts", got.tolist(), w.tolist())
    return Raw(torch, (w.size + 1,), check)


def untouched_raw(torch, words):
    """An output the call is not given: it keeps the poison."""
    def check(r, ctx):
        assert (r == POISON_RAW).all(), ctx + ("an output that was not passed was written",)
    return Raw(torch, (words + 1,), check)


def rows16_raw(torch, rsmi, stored):
    """R of every row of stored (nb, n, S) and a spare slot."""
    nb, n, S = stored.shape
    want = want_entries(stored)

    def check(r, ctx):
        raws = _spare(r, ctx).reshape(nb, n)
        assert (raws >> 16 == 0).all(), ctx
        got = entries_of(rsmi, raws, S)
        assert np.array_equal(got, want), ctx + ("R(row)", np.argwhere(got != want)[:4].tolist())
    return Raw(torch, (nb * n + 1,), check)


def _stripe_call(name, torch, rsmi, c, rng, S, nb, layout, flags=None):
    """The five stripe calls that take (rows, words, flags): locate, locate pair, heal, heal pair
    write verdict words; the heals also rewrite the named rows."""
    k, m = c.k, c.m
    flags = bool(rng.integers(2)) if flags is None else flags
    sh = damaged(rng, _full(k, m, _rows_data(rng, nb, k, S)))
    if name in ("locate", "heal"):
        verdicts = want_verdicts(k, m, sh)
    else:
        verdicts = want_pairs(k, m, sh)
    image = None
    if name == "heal":
        image = test_heal.want_image(k, m, sh, verdicts)
    elif name == "heal_pair":
        image = test_heal_pair.want_image(k, m, sh, verdicts)
    if image is not None:  # undamaged stripes byte-identical, damaged ones repaired
        dirty = want_flags(k, m, sh).any(axis=1)
        assert np.array_equal(image[~dirty], sh[~dirty])
        assert m < 2 or not want_flags(k, m, image).any()
    h = HalfBufs(torch, rsmi, c, sh, layout, image)
    words = words_raw(torch, verdicts)
    bad = flags_raw(torch, want_flags(k, m, sh)) if flags else untouched_raw(torch, nb * m)
    f = getattr(c, name + "_batch_dev")

    def fn(st):
        f(*h.args(), words.dev.data_ptr(), bad.dev.data_ptr() if flags else 0, st)

    return Call((name, k, m, S, nb, layout, flags), c, [h.d, h.p, words, bad], fn)


def verify_call(torch, rsmi, c, rng, S, nb, layout):
    """rsmi_verify_batch_dev: the flags of want_flags, the rows unchanged."""
    k, m = c.k, c.m
    sh = damaged(rng, _full(k, m, _rows_data(rng, nb, k, S)))
    h = HalfBufs(torch, rsmi, c, sh, layout)
    bad = flags_raw(torch, want_flags(k, m, sh))

    def fn(st):
        c.verify_batch_dev(*h.args(), bad.dev.data_ptr(), st)

    return Call(("verify", k, m, S, nb, layout), c, [h.d, h.p, bad], fn)


def scrub_call(torch, rsmi, c, rng, S, nb, layout):
    """rsmi_scrub_batch_dev: Verify's flags and R of every row as stored."""
    k, m = c.k, c.m
    sh = damaged(rng, _full(k, m, _rows_data(rng, nb, k, S)))
    h = HalfBufs(torch, rsmi, c, sh, layout)
    bad, raw = flags_raw(torch, want_flags(k, m, sh)), rows16_raw(torch, rsmi, sh)

    def fn(st):
        c.scrub_batch_dev(*h.args(), bad.dev.data_ptr(), raw.dev.data_ptr(), st)

    return Call(("scrub", k, m, S, nb, layout), c, [h.d, h.p, bad, raw], fn)


def locate_call(torch, rsmi, c, rng, S, nb, layout, flags=None):
    return _stripe_call("locate", torch, rsmi, c, rng, S, nb, layout, flags)


def locate_pair_call(torch, rsmi, c, rng, S, nb, layout, flags=None):
    return _stripe_call("locate_pair", torch, rsmi, c, rng, S, nb, layout, flags)


def heal_call(torch, rsmi, c, rng, S, nb, layout, flags=None):
    return _stripe_call("heal", torch, rsmi, c, rng, S, nb, layout, flags)


def heal_pair_call(torch, rsmi, c, rng, S, nb, layout, flags=None):
    return _stripe_call("heal_pair", torch, rsmi, c, rng, S, nb, layout, flags)


def random_losses(rng, n, m, nb):
    """0 to m rows lost per block, and now and then one more than the code can rebuild."""
    out = []
    for _ in range(nb):
        cnt = int(rng.integers(0, m + 1))
        if rng.integers(8) == 0:
            cnt = m + 1
        out.append(tuple(sorted(rng.choice(n, size=cnt, replace=False).tolist())))
    return out


def mixed_bytes(n, nb):
    """An upper bound of one mixed call's share of mixed_words under any launch_units_max.
    launch_mixed asks once per segment, and a segment is at least one block, so at most nb times:
    each time the plan pointers of all the call's patterns (at most nb), rounded up to 16, and the
    request itself rounded up to 16; over the segments together a list entry and k + m row words
    per block, the lists rounded up to 16 per segment."""
    return nb * (round16(nb * 8) + 16 + 16) + nb * MIXED_ENTRY + nb * n * 4


def mixed_call(torch, rsmi, c, rng, S, nb, layout, form="plain", losses=None, outs=None):
    """rsmi_reconstruct_mixed_batch_dev (form plain), _dev_crcs (crcs: outs says which of R, R32) and
    _dev_verify (verify): statuses, the whole buffer against the definition's image (missing rows
    nobody rebuilt keep MISSING), the checksums of test_mixed_crcs / test_mixed_verify."""
    k, m, n = c.k, c.m, c.n
    aligned = layout == "aligned"
    lay = mr.layout(rsmi, k, m, S, nb, aligned)
    losses = random_losses(rng, n, m, nb) if losses is None else losses
    present = mr.present_of(n, losses)
    sh = mr.stored(_full(k, m, _rows_data(rng, nb, k, S)), present)
    W = mr.wanted(k, present, None, False)
    want_status, image = mr.definition(k, m, sh, present, W)
    host = lay.fill(sh)
    expect = host.copy()
    lay.rows(expect)[:] = image
    d = Bytes(torch, host, expect)
    bufs = [d]
    P = mr.u8(present)
    if form == "crcs":
        if outs is None:
            outs = [(True, True), (True, False), (False, True)][int(rng.integers(3))]
        wr = mc.written(W, want_status)
        raws = []
        for i, on in enumerate(outs):
            if not on:
                raws.append(None)
                continue

            def check(r, ctx, i=i):
                got = _spare(r, ctx).reshape(nb, n)
                mc.assert_raws(rsmi, image, wr, got if i == 0 else None, got if i == 1 else None, ctx)
            raws.append(Raw(torch, (nb * n + 1,), check))
        bufs += [r for r in raws if r is not None]
    elif form == "verify":
        T = mv.touched(k, present, W, want_status)

        def check(r, ctx):
            mv.assert_raws(rsmi, image, T, _spare(r, ctx).reshape(nb, n), ctx)
        raw = Raw(torch, (nb * n + 1,), check)
        bufs.append(raw)

    def fn(st):
        base = d.dev.data_ptr() + lay.off
        if form == "plain":
            got = c.reconstruct_mixed_batch_dev(base, lay.rs, lay.bs, S, nb, P, None, False, st)
        elif form == "crcs":
            got = c.reconstruct_mixed_batch_dev_crcs(base, lay.rs, lay.bs, S, nb, P, None, False,
                                                     raws[0].dev.data_ptr() if raws[0] else 0,
                                                     raws[1].dev.data_ptr() if raws[1] else 0, st)
        else:
            got = c.reconstruct_mixed_batch_dev_verify(base, lay.rs, lay.bs, S, nb, P, None, False, raw.dev.data_ptr(), st)
        assert got == want_status, (form, got, want_status)

    call = Call(("mixed_" + form, k, m, S, nb, layout, tuple(losses), outs), c, bufs, fn)
    call.mixed_bytes = mixed_bytes(n, nb)
    return call


def mixed_plain_call(torch, rsmi, c, rng, S, nb, layout, **kw):
    return mixed_call(torch, rsmi, c, rng, S, nb, layout, "plain", **kw)


def mixed_crcs_call(torch, rsmi, c, rng, S, nb, layout, **kw):
    return mixed_call(torch, rsmi, c, rng, S, nb, layout, "crcs", **kw)


def mixed_verify_call(torch, rsmi, c, rng, S, nb, layout, **kw):
    return mixed_call(torch, rsmi, c, rng, S, nb, layout, "verify", **kw)


def named_rows_call(torch, rsmi, c, rng, S, nb, layout, outs=None, slots=None):
    """rsmi_crc_named_rows_dev over one or two slots of entries that name any row, the seam and
    nothing at all (the entries are a device input, produced behind the gate like the rows)."""
    k, m, n = c.k, c.m, c.n
    if outs is None:
        outs = [(True, True), (True, False), (False, True)][int(rng.integers(3))]
    slots = int(rng.integers(1, 3)) if slots is None else slots
    sh = _full(k, m, _rows_data(rng, nb, k, S))
    entries = rng.integers(-2, n + 2, size=(nb, slots)).astype(np.int32)
    entries[0, 0] = k - (nb % 2)   # the seam between the halves: row k - 1 or row k
    h = HalfBufs(torch, rsmi, c, sh, layout)
    eb = entries.view(np.uint8).reshape(-1)
    e = Bytes(torch, eb, eb.copy())
    refs = refs_of(sh)
    raws = []
    for i, on in enumerate(outs):
        if not on:
            raws.append(None)
            continue

        def check(r, ctx, i=i):
            got = _spare(r, ctx).reshape(nb, slots)
            assert_named(rsmi, sh, entries, got if i == 0 else None, got if i == 1 else None, refs, ctx)
        raws.append(Raw(torch, (nb * slots + 1,), check))

    def fn(st):
        c.crc_named_rows_dev(*h.args(), e.dev.data_ptr(), slots, raws[0].dev.data_ptr() if raws[0] else 0,
                             raws[1].dev.data_ptr() if raws[1] else 0, st)

    return Call(("named_rows", k, m, S, nb, layout, outs, slots), c, [h.d, h.p, e] + [r for r in raws if r is not None], fn)


def ragged_bytes(sizes):
    """One ragged call's share of mixed_words: a descriptor per block, a unit entry per 4 KiB of a
    row, the two unit lists rounded up to 16 each."""
    return len(sizes) * RAGGED_DESC + sum(-(-tpb(S) // 4) for S in sizes) * RAGGED_UNIT + 32


def ragged_call(torch, rsmi, c, rng, S, nb, layout, sizes=None):
    """rsmi_encode_ragged_batch_dev over nb blocks whose sizes start at S and then run through the
    sizes of this module (test_ragged_encode.Batch: aligned, or data rows at an odd phase); the
    data image unchanged, the parity image the oracle's, gaps and padding included."""
    k, m = c.k, c.m
    if sizes is None:
        at = SIZES.index(S)
        sizes = [SIZES[(at + i) % 3] for i in range(nb)]
    b = Batch(k, m, *((1, 3) if layout == "ua" else (0, 0)))
    for i, s in enumerate(sizes):
        b.place(s, "a" if layout == "aligned" else "u", v=int(rng.integers(1 << 30)), gap=i % 3, extra=i % 2)
    d_img, p_img, want = b.images()
    d, p = Bytes(torch, d_img, d_img.copy()), Bytes(torch, p_img, want)
    blocks = b.blocks()

    def fn(st):
        c.encode_ragged_batch_dev(d.dev.data_ptr(), p.dev.data_ptr(), blocks, st)

    call = Call(("ragged", k, m, tuple(sizes), layout), c, [d, p], fn)
    call.mixed_bytes = ragged_bytes(sizes)
    call.batch = b
    return call


def ragged_tiny_call(torch, rsmi, c, rng, nb, S=16):
    """nb aligned blocks of S bytes back to back in one ragged call; the parity of all of them from
    one oracle batch."""
    k, m = c.k, c.m
    P = round16(S)
    data = _rows_data(rng, nb, k, S)
    par = orc.encode_fast(k, m, data, threads=4)
    rows = np.zeros((nb, 5), dtype=np.uint64)
    i = np.arange(nb, dtype=np.uint64)
    rows[:, 0], rows[:, 1], rows[:, 2] = S, i * np.uint64(k * P), P
    rows[:, 3], rows[:, 4] = i * np.uint64(m * P), P
    d_img = np.full((nb, k, P), 0xC3, dtype=np.uint8)
    p_img = np.full((nb, m, P), 0xC3, dtype=np.uint8)
    want = p_img.copy()
    d_img[:, :, :S] = data
    want[:, :, :S] = par
    tail = np.full(TAIL, 0xC3, dtype=np.uint8)
    d_img, p_img, want = (np.concatenate([x.reshape(-1), tail]) for x in (d_img, p_img, want))
    d, p = Bytes(torch, d_img, d_img.copy()), Bytes(torch, p_img, want)

    def fn(st):
        c.encode_ragged_batch_dev(d.dev.data_ptr(), p.dev.data_ptr(), rows, st)

    call = Call(("ragged_tiny", k, m, S, nb), c, [d, p], fn)
    call.mixed_bytes = ragged_bytes([S] * nb)
    return call


def _lost(rng, c):
    return sorted(rng.choice(c.n, size=int(rng.integers(1, c.m + 1)), replace=False).tolist())


def reconstruct_rows_call(torch, rsmi, c, rng, S, nb, layout):
    """rsmi_reconstruct_rows_batch_dev: the last lost row alone is required; the others keep 0xEE."""
    lost = _lost(rng, c)
    return reconstruct_call(torch, rsmi, c, S, nb, layout, rng, lost, None, required=[lost[-1]])


# the four of test_stream_order behind this module's signature (labels are left to that module)
def b_encode(torch, rsmi, c, rng, S, nb, layout):
    return encode_call(torch, rsmi, c, S, nb, layout, rng, None)


def b_encode_crc(torch, rsmi, c, rng, S, nb, layout):
    return encode_call(torch, rsmi, c, S, nb, layout, rng, None, crc=True)


def b_reconstruct(torch, rsmi, c, rng, S, nb, layout):
    return reconstruct_call(torch, rsmi, c, S, nb, layout, rng, _lost(rng, c), None)


def _b_crc_rows(bits):
    def build(torch, rsmi, c, rng, S, nb, layout):
        call = crc_rows_call(torch, rsmi, c, bits, 1, S, nb, layout == "aligned", _rows_data(rng, nb, 3, S))
        call.label = None
        return call
    return build


NEW = {"verify": verify_call, "scrub": scrub_call, "locate": locate_call, "locate_pair": locate_pair_call,
       "heal": heal_call, "heal_pair": heal_pair_call, "mixed": mixed_plain_call, "mixed_crcs": mixed_crcs_call,
       "mixed_verify": mixed_verify_call, "named_rows": named_rows_call, "ragged": ragged_call,
       "reconstruct_rows": reconstruct_rows_call}
BUILDERS = dict(NEW, encode=b_encode, encode_crc=b_encode_crc, reconstruct=b_reconstruct,
                crc16_rows=_b_crc_rows(16), crc32_rows=_b_crc_rows(32))
NAMES = sorted(BUILDERS)
# the successions of leg 1 that cross one row of the shared-state table each
NEIGHBOURS = [("mixed", "ragged"), ("ragged", "mixed_verify"), ("locate", "locate_pair"), ("locate_pair", "heal"),
              ("heal", "heal_pair"), ("encode_crc", "scrub"), ("scrub", "mixed_verify"), ("mixed_verify", "encode_crc"),
              ("crc32_rows", "named_rows"), ("named_rows", "mixed_crcs")]


def no_start_over(calls, runs):
    """The calls' shares of one stream's mixed_words over runs runs fit the scratch's first size:
    the head never starts over, so no call has to wait for the stream."""
    return runs * sum(getattr(x, "mixed_bytes", 0) for x in calls) <= FLOOR


# ---------------------------------------------------------------- 0: the constants, on the CPU
def tiny_blocks():
    """Blocks of RS(4,2), S = 16 in one ragged call whose upload is just past half of FLOOR."""
    per = RAGGED_DESC + RAGGED_UNIT
    return FLOOR // 2 // per + 1


def test_scratch_constants_match_source():
    """Leg 3 reaches start-over and regrow only while mixed_words keeps its floor, its fit test and
    its growth rule, and the descriptors their sizes."""
    with open(os.path.join(CSRC, "rsmi_mixed.cpp")) as f:
        src = f.read()
    body = src[src.index("int mixed_words("):src.index("int launch_mixed(")]
    body = " ".join(body.split())
    assert "need = round_up(need, 16);" in body
    assert "if (ms.cap - ms.head < need) { if (ms.d) HIP_TRY(hipStreamSynchronize(st)); ms.head = 0;" in body
    assert ("if (ms.cap < need) { const size_t cap = std::max<size_t>(std::max(need, ms.cap + ms.cap / 2), "
            "size_t(1) << 20);") in body
    assert FLOOR == 1 << 20
    with open(os.path.join(CSRC, "rs_plan.hpp")) as f:
        hpp = f.read()
    got = re.findall(r"static_assert\(sizeof\(RaggedUnit\) == (\d+) && sizeof\(RaggedBlockDev\) == (\d+)", hpp)
    assert got == [(str(RAGGED_UNIT), str(RAGGED_DESC))]
    entry = re.search(r"struct MixedEntry \{\s*uint32_t (\w+), (\w+);\s*\};", hpp)
    assert entry and MIXED_ENTRY == 2 * 4
    with open(os.path.join(CSRC, "rsmi_ragged.cpp")) as f:
        rag = " ".join(f.read().split())
    assert "mixed_words(c, stream, desc_bytes + u0_bytes + u1_bytes, h, d)" in rag
    assert "const size_t desc_bytes = descs.size() * sizeof(RaggedBlockDev);" in rag
    # leg 3's sizes: one tiny call is past half the floor and within it, two are past it
    nb = tiny_blocks()
    one = ragged_bytes([16] * nb)
    assert FLOOR // 2 < nb * (RAGGED_DESC + RAGGED_UNIT) <= one < FLOOR < 2 * nb * (RAGGED_DESC + RAGGED_UNIT)
    assert (nb - 1) * (RAGGED_DESC + RAGGED_UNIT) <= FLOOR // 2   # the fewest blocks that do


# ---------------------------------------------------------------- S: every new builder alone
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(NEW))
def test_builder_alone(gpu, name):
    """Each new builder on a fresh Codec(10, 4), warm and then behind the gate, in both layouts: a
    failure in a leg is then about sharing, not about the builder."""
    torch, rsmi, gate = gpu
    with _leg("S"), rsmi.Codec(10, 4) as c:
        st = torch.cuda.Stream()
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        calls = [NEW[name](torch, rsmi, c, rng, S, nb, layout)
                 for S, nb, layout in ((1025, 3, "aligned"), (4097, 5, "ua"), (16, 7, "aligned"))]
        assert no_start_over(calls, 2)
        for x in calls:
            warm_then_gated(torch, gate, [(st, x)])


# ---------------------------------------------------------------- 1: all families back to back
def leg1_calls(torch, rsmi, c, rng):
    al, ua = "aligned", "ua"
    k, m = c.k, c.m
    inl, two = fused_label(k, m, 4097, 3), fused_label(k, m, 4097, 33)
    assert inl.endswith(",INL") and ",INL" not in two
    a = (torch, rsmi, c, rng)
    return [
        b_encode(*a, 4097, 3, al),
        # mixed_words: mixed -> ragged -> mixed _verify
        mixed_plain_call(*a, 1025, 5, ua),
        ragged_call(*a, 16, 5, al),
        mixed_verify_call(*a, 4097, 4, al),
        verify_call(*a, 1025, 3, ua),
        # locate_scratch: locate -> locate pair -> heal -> heal pair
        locate_call(*a, 4097, 5, al, flags=True),
        locate_pair_call(*a, 1025, 4, ua, flags=False),
        heal_call(*a, 4097, 3, al, flags=False),
        heal_pair_call(*a, 16, 7, ua, flags=True),
        # the fold geometry, the records and unit counters: three geometries between two fused encodes
        encode_call(torch, rsmi, c, 4097, 3, al, rng, inl, crc=True),
        scrub_call(*a, 1025, 5, al),
        mixed_verify_call(*a, 16, 6, ua),
        encode_call(torch, rsmi, c, 4097, 33, al, rng, two, crc=True),
        # the CRC-32 tables and the cached end shift: three sizes, three families
        crc_rows_call(torch, rsmi, c, 32, 1, 1025, 2, True, _rows_data(rng, 2, 3, 1025)),
        named_rows_call(*a, 4097, 3, al, outs=(False, True), slots=2),
        mixed_crcs_call(*a, 16, 5, ua, outs=(True, True)),
        crc_rows_call(torch, rsmi, c, 16, 1, 1025, 2, True, _rows_data(rng, 2, 3, 1025)),
        b_reconstruct(*a, 4097, 3, al),
        reconstruct_rows_call(*a, 1025, 3, ua),
        ragged_call(*a, 4097, 7, ua),
        scrub_call(*a, 4097, 2, ua),
    ]


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", CODES)
def test_all_families_back_to_back(gpu, k, m):
    """Leg 1: 21 calls of one Codec on one side stream behind one gate, every builder at least once,
    ordered so that each piece of shared state is crossed by two different families in succession.
    The uploads of the warm and the gated run together stay within the mixed scratch's first size,
    so nothing starts over and no call may wait."""
    torch, rsmi, gate = gpu
    with _leg("1"), rsmi.Codec(k, m) as c:
        st = torch.cuda.Stream()
        calls = leg1_calls(torch, rsmi, c, np.random.default_rng(0x1000 + k))
        assert {x.name[0] for x in calls} >= {"mixed_plain", "mixed_crcs", "mixed_verify", "ragged", "scrub", "verify",
                                              "locate", "locate_pair", "heal", "heal_pair", "named_rows", "encode",
                                              "encode_crc", "reconstruct", "crc16_rows", "crc32_rows"}
        assert any(x.name[0] == "reconstruct" and x.name[-1] is not None for x in calls)
        assert no_start_over(calls, 2)
        warm_then_gated(torch, gate, [(st, x) for x in calls])


# ---------------------------------------------------------------- 2: first use behind pending work
@pytest.mark.gpu
def test_first_use_behind_pending_work(gpu):
    """Leg 2: a fresh Codec(10, 4), no warm run: a plain encode, then behind its pending kernels the
    calls whose first use builds state: scrub (CRC-16 tables, scrub scratch), locate (its table and
    scratch), mixed _verify with three unseen patterns (three plans, mixed and mixed-verify scratch),
    named rows with CRC-32 (its tables), ragged encode (plan and scratch already there).  The
    library may block; every output is exact and nothing is written after the consumer."""
    torch, rsmi, gate = gpu
    with _leg("2"), rsmi.Codec(10, 4) as c:
        st = torch.cuda.Stream()
        rng = np.random.default_rng(0x2)
        a = (torch, rsmi, c, rng)
        calls = [b_encode(*a, 1025, 3, "aligned"),
                 scrub_call(*a, 4097, 5, "aligned"),
                 locate_call(*a, 1025, 5, "ua", flags=True),
                 mixed_verify_call(*a, 4097, 3, "aligned", losses=[(2,), (5, 7, 10), (0, 1, 12, 13)]),
                 named_rows_call(*a, 1025, 3, "ua", outs=(False, True)),
                 ragged_call(*a, 16, 6, "aligned")]
        done = run_plan(torch, gate, [(st, x) for x in calls], gated=True, must_not_wait=False)
        print("\nshared context: first use of five families behind the gate: the delay had %s when the calls "
              "returned" % ("ended (a call waited)" if any(done.values()) else "not ended (no wait)"))


def behind_busy_null_stream(torch, gate, call):
    """call with the gate's delay queued on the NULL stream just before it."""
    inner = call.fn

    def fn(st):
        with torch.cuda.stream(torch.cuda.default_stream()):
            gate()
        t0 = time.perf_counter()
        inner(st)
        print("\nshared context: %s with the NULL stream busy for %.0f ms returned after %.1f ms"
              % (call.name[0], gate.ms, 1e3 * (time.perf_counter() - t0)))

    call.fn = fn
    return call


@pytest.mark.gpu
def test_first_use_with_the_null_stream_busy(gpu):
    """Leg 2, second variant: the side stream is free and the NULL stream is busy (the delay is
    queued there) when a scrub builds the CRC-16 tables and then a named rows call the CRC-32
    tables.  The library fills a table with a blocking copy, which waits for the NULL stream and
    returns with the table in place; this pins that the results are right in that order of events.
    It does not tell a blocking copy from an asynchronous one out of pageable memory: the runtime
    stages such a copy and returns only when it has run, so that change computes the same (tried on
    a scratch build).  Only an asynchronous copy out of page-locked memory would leave the side
    stream's kernels reading an empty table; torch's side streams do not wait for the NULL stream."""
    torch, rsmi, gate = gpu
    assert torch.cuda.default_stream().cuda_stream == 0
    with _leg("2"), rsmi.Codec(10, 4) as c:
        st = torch.cuda.Stream()
        rng = np.random.default_rng(0x2B)
        a = (torch, rsmi, c, rng)
        calls = [behind_busy_null_stream(torch, gate, scrub_call(*a, 4097, 5, "aligned")),
                 behind_busy_null_stream(torch, gate, named_rows_call(*a, 1025, 3, "ua", outs=(False, True)))]
        run_plan(torch, gate, [(st, x) for x in calls], gated=False)


# ---------------------------------------------------------------- 3: start over and regrow
@pytest.mark.gpu
def test_mixed_words_start_over_and_regrow_across_families(gpu):
    """Leg 3: Codec(4, 2), one stream, one gate: a mixed reconstruct; a ragged encode of tiny blocks
    whose upload is past half the scratch's first size; a mixed _verify; the same ragged encode once
    more, which no longer fits behind the three (the head starts over while they are pending); a
    ragged encode past one and a half times the first size (the scratch is freed and regrown); a
    mixed _crcs.  The library may block."""
    torch, rsmi, gate = gpu
    with _leg("3"), rsmi.Codec(4, 2) as c:
        st = torch.cuda.Stream()
        rng = np.random.default_rng(0x3)
        a = (torch, rsmi, c, rng)
        nb = tiny_blocks()
        calls = [mixed_plain_call(*a, 16, 5, "aligned"),
                 ragged_tiny_call(*a, nb),
                 mixed_verify_call(*a, 1025, 4, "ua"),
                 ragged_tiny_call(*a, nb),
                 ragged_tiny_call(*a, 2 * nb + 100),
                 mixed_crcs_call(*a, 4097, 3, "aligned", outs=(True, True))]
        need = [x.mixed_bytes for x in calls]
        per = RAGGED_DESC + RAGGED_UNIT
        assert sum(need[:3]) <= FLOOR          # calls 1 to 3 lie behind one another (need: upper bounds)
        assert 2 * nb * per > FLOOR            # call 4 does not fit behind call 2: the head starts over
        assert need[3] <= FLOOR < (2 * nb + 100) * per   # call 4 keeps the first size, call 5 regrows
        done = run_plan(torch, gate, [(st, x) for x in calls], gated=True, must_not_wait=False)
        print("\nshared context: start over and regrow behind the gate: the delay had %s when the calls returned"
              % ("ended (a call waited)" if any(done.values()) else "not ended"))


# ---------------------------------------------------------------- 4: options between queued launches
def with_options(call, options, want_split, seen):
    """call with options set just before it and the growth of split_launches recorded around it."""
    inner, c = call.fn, call.codec

    def fn(st):
        for key, value in options:
            c.set_option(key, value)
        at = c.stat("split_launches")
        inner(st)
        seen.append((call.name[0], c.stat("split_launches") - at, want_split))

    call.fn = fn
    return call


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", CODES)
def test_options_between_queued_launches(gpu, k, m):
    """Leg 4: on one stream behind one gate, waves_per_cu, launch_units_max and crc16_fused_fold
    change between a scrub, a ragged encode, a mixed _verify, a heal pair and a fused encode.  Each
    call's pieces, counted by split_launches, are those of the cap set just before it."""
    torch, rsmi, gate = gpu
    with _leg("4"), rsmi.Codec(k, m) as c:
        st = torch.cuda.Stream()
        rng = np.random.default_rng(0x4000 + k)
        a = (torch, rsmi, c, rng)
        seen = []
        scrub = scrub_call(*a, 4097, 5, "aligned")
        ragged = ragged_call(*a, 16, 6, "aligned")
        losses = [(0,), (1, k), (2,), (), (3, k + 1), (k,)]
        mixed = mixed_verify_call(*a, 4097, 6, "aligned", losses=losses)
        heal = heal_pair_call(*a, 1025, 5, "ua", flags=True)
        enc = encode_call(torch, rsmi, c, 4097, 7, "aligned", rng, None, crc=True)
        classes, units = ragged.batch.classes(0, 0), ragged.batch.units(0, 0)
        assert FALLBACK not in classes
        seg = max(1, 7 // tpb(4097))
        mixed_cut = sum(len({len(lost) for lost in losses[s:s + seg] if lost}) for s in range(0, 6, seg))
        assert seg == 1 and mixed_cut == 5
        passes = PASSES["heal_pair"][0 if m >= 3 else 1]
        plan = [
            with_options(scrub, [("waves_per_cu", 1), ("launch_units_max", 3), ("crc16_fused_fold", 0)],
                         pieces(5, 3, upb(4097)), seen),
            with_options(ragged, [("waves_per_cu", 0), ("launch_units_max", 0)],
                         segment_launches(units, classes, DEFAULT_CAP, (m + 3) // 4), seen),
            with_options(mixed, [("launch_units_max", 7)], mixed_cut, seen),
            with_options(heal, [("waves_per_cu", 1), ("launch_units_max", 4)], passes * pieces(5, 4, tpb(1025)), seen),
            with_options(enc, [("waves_per_cu", 0), ("launch_units_max", 5), ("crc16_fused_fold", 1)],
                         pieces(7, 5, upb(4097)), seen),
        ]
        assert [pieces(5, 3, 2), pieces(5, 4, 2), pieces(7, 5, 2)] == [5, 3, 4]   # none of them one launch
        assert no_start_over(plan, 2)
        try:
            warm_then_gated(torch, gate, [(st, x) for x in plan])
        finally:
            for key in ("waves_per_cu", "launch_units_max"):
                c.set_option(key, 0)
            c.set_option("crc16_fused_fold", 1)
        assert len(seen) == 10
        for name, got, want in seen:
            assert got == want, (name, got, want, seen)


# ---------------------------------------------------------------- 5: two streams, families crossed
@pytest.mark.gpu
def test_two_streams_families_crossed(gpu):
    """Leg 5: one Codec(10, 4), two gated streams that start together: A runs ragged, scrub, locate
    pair, mixed _verify; B the same four families in the opposite order at other sizes.  Each stream
    has its own scratch of each kind while the other's launches overlap."""
    torch, rsmi, gate = gpu
    with _leg("5"), rsmi.Codec(10, 4) as c:
        sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
        assert len({sa.cuda_stream, sb.cuda_stream, torch.cuda.current_stream().cuda_stream}) == 3
        rng = np.random.default_rng(0x5)
        a = (torch, rsmi, c, rng)
        A = [ragged_call(*a, 4097, 5, "aligned"), scrub_call(*a, 1025, 7, "ua"),
             locate_pair_call(*a, 4097, 3, "aligned", flags=True), mixed_verify_call(*a, 16, 6, "ua")]
        B = [mixed_verify_call(*a, 4097, 5, "aligned"), locate_pair_call(*a, 1025, 5, "ua", flags=False),
             scrub_call(*a, 4097, 3, "aligned"), ragged_call(*a, 1025, 7, "ua")]
        assert no_start_over(A, 2) and no_start_over(B, 2)
        plan = [(s, x) for pair in zip(A, B) for s, x in zip((sa, sb), pair)]
        warm_then_gated(torch, gate, plan, rendezvous=True)


# ---------------------------------------------------------------- 6: four host threads
def _thread_rounds(torch, st, rounds, barrier, snaps, errs):
    """The producer, the calls and the consumer of every round on st, with no host sync until the
    last round is queued."""
    try:
        barrier.wait()
        with torch.cuda.stream(st):
            for calls in rounds:
                for x in calls:
                    for b in x.bufs:
                        if b.inp is not None:
                            b.dev.copy_(b.inp, non_blocking=True)
                        else:
                            b.dev.fill_(b.poison)
                    x.fn(st.cuda_stream)
                for x in calls:
                    snaps.append([b.dev.clone() for b in x.bufs])
                    for b in x.bufs:
                        b.dev.fill_(b.fillv)
        st.synchronize()
    except BaseException as e:  # noqa: B036 - handed to the main thread
        errs.append(e)


@pytest.mark.gpu
def test_four_host_threads_one_context(gpu):
    """Leg 6: one Codec(10, 4), four threads started together, each with its own stream and family:
    ragged encode; mixed _verify; scrub, locate, heal, verify; fused encode + CRC-16.  Five rounds
    of fresh data per thread, checked after the thread's stream is drained."""
    torch, rsmi, gate = gpu
    with _leg("6"), rsmi.Codec(10, 4) as c:
        rng = np.random.default_rng(0x6)
        a = (torch, rsmi, c, rng)
        shapes = [(1025, 3, "aligned"), (4097, 5, "ua"), (16, 7, "aligned"), (4097, 2, "aligned"), (1025, 6, "ua")]
        families = [
            lambda S, nb, lay: [ragged_call(*a, S, nb, lay)],
            lambda S, nb, lay: [mixed_verify_call(*a, S, nb, lay)],
            lambda S, nb, lay: [scrub_call(*a, S, nb, lay), locate_call(*a, S, nb, lay), heal_call(*a, S, nb, lay),
                                verify_call(*a, S, nb, lay)],
            lambda S, nb, lay: [encode_call(torch, rsmi, c, S, nb, lay, rng, None, crc=True)],
        ]
        rounds = [[f(*shapes[(r + t) % 5]) for r in range(5)] for t, f in enumerate(families)]
        streams = [torch.cuda.Stream() for _ in families]
        assert len({s.cuda_stream for s in streams}) == 4
        for per in rounds:
            for calls in per:
                for x in calls:
                    for b in x.bufs:
                        b.dev.fill_(b.poison)
        torch.cuda.synchronize()
        barrier = threading.Barrier(4)
        snaps, errs = [[] for _ in families], []
        threads = [threading.Thread(target=_thread_rounds, args=(torch, streams[t], rounds[t], barrier, snaps[t], errs))
                   for t in range(4)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        torch.cuda.synchronize()
        assert not errs, errs
        for t in range(4):
            flat = [x for calls in rounds[t] for x in calls]
            assert len(flat) == len(snaps[t])
            for x, sn in zip(flat, snaps[t]):
                for i, b in enumerate(x.bufs):
                    b.check(sn[i].cpu().numpy(), (x.name, i, "thread %d" % t))
                    left = b.dev.cpu().numpy()
                    assert (left == (b.fillv & 0xFF if left.dtype == np.uint8 else b.fillv)).all(), \
                        (x.name, i, "written after the consumer's fill")


# ---------------------------------------------------------------- 7: seeded random interleave
SEEDS = (867, 573, 8151)   # found on the CPU by a search over 400 000 seeds, so that the test below holds
DRAWS = 40


def draw_specs(seed):
    """[(stream 0 or 1, builder, S, nb, layout, seed of the call's own choices)], device-free."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(DRAWS):
        out.append((int(rng.integers(2)), NAMES[int(rng.integers(len(NAMES)))], SIZES[int(rng.integers(3))],
                    int(rng.integers(1, 8)), LAYOUTS[int(rng.integers(2))], int(rng.integers(1 << 31))))
    return out


def successions(specs):
    """Ordered pairs of builders that follow one another on one stream: the calls that share that
    stream's scratch of every kind."""
    out = set()
    for st in (0, 1):
        own = [s[1] for s in specs if s[0] == st]
        out |= set(zip(own, own[1:]))
    return out


def test_seeds_cover_builders_and_neighbours():
    drawn, pairs = [], set()
    for seed in SEEDS:
        specs = draw_specs(seed)
        drawn += [s[1] for s in specs]
        pairs |= successions(specs)
    assert len(NAMES) == 17
    assert all(drawn.count(name) >= 2 for name in NAMES), {name: drawn.count(name) for name in NAMES}
    assert set(NEIGHBOURS) <= pairs, sorted(set(NEIGHBOURS) - pairs)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_random_interleave(gpu, seed):
    """Leg 7: 40 calls drawn uniformly from all builders with random size, blocks, layout, damage,
    erasure patterns and optional outputs, dealt over two streams of one Codec(10, 4), warm and then
    gated.  The library may block (nothing bounds the scratch here)."""
    torch, rsmi, gate = gpu
    specs = draw_specs(seed)
    with _leg("7"), rsmi.Codec(10, 4) as c:
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        plan = [(streams[st], BUILDERS[name](torch, rsmi, c, np.random.default_rng(sub), S, nb, layout))
                for st, name, S, nb, layout, sub in specs]
        try:
            run_plan(torch, gate, plan, gated=False)
            run_plan(torch, gate, plan, gated=True, must_not_wait=False)
        except BaseException:
            print("\nshared context: seed %d:" % seed)
            for i, s in enumerate(specs):
                print("  %2d stream %d %s S=%d nb=%d %s sub=%d" % ((i,) + s))
            raise


# ---------------------------------------------------------------- 8: the host paths
HOST_POISON = 0xA5A5A5A5
HOST_GUARD = 32


def guarded(content):
    """Pageable host bytes between guard bytes: (the whole buffer, the address of the content)."""
    buf = np.full(content.size + 2 * HOST_GUARD, 0xA7, dtype=np.uint8)
    buf[HOST_GUARD:HOST_GUARD + content.size] = content.reshape(-1)
    return buf, buf.ctypes.data + HOST_GUARD


def assert_guarded(buf, want, ctx):
    whole = np.full(buf.size, 0xA7, dtype=np.uint8)
    whole[HOST_GUARD:HOST_GUARD + want.size] = want.reshape(-1)
    if not np.array_equal(buf, whole):
        at = np.flatnonzero(buf != whole)
        raise AssertionError("%r: %d bytes differ, first at %d of %d" % (ctx, at.size, at[0] - HOST_GUARD, want.size))


def host_words(count):
    return np.full(count + 1, HOST_POISON, dtype=np.uint32)


def spare_host(w, ctx):
    assert w[-1] == HOST_POISON, (ctx, "the slot past the output was written")
    return w[:-1]


def assert_raw32(rsmi, raws, rows, ctx):
    """raws (..., ) uint32 against zlib.crc32 of rows (count, S)."""
    S = rows.shape[-1]
    for i, (x, row) in enumerate(zip(raws.reshape(-1), rows.reshape(-1, S))):
        assert rsmi.crc32_entry(b"", int(x), S) == zlib.crc32(row.tobytes()), (ctx, "R32", i)


def assert_raw16(rsmi, raws, rows, ctx):
    S = rows.shape[-1]
    for i, (x, row) in enumerate(zip(raws.reshape(-1), rows.reshape(-1, S))):
        assert int(x) >> 16 == 0 and rsmi.crc16_entry(b"", int(x), S) == orc.crc16_ibm(row.tobytes()), (ctx, "R", i)


def host_round(rsmi, c, rng, S, nb, ctx):
    """Every host entry point once over fresh pageable rows at pitch S, the families alternating:
    encode, verify, encode + both checksums, scrub, locate, mixed _verify, heal, ragged, the rows
    passes, encode.  Whole-buffer compares between guard bytes; outputs start as garbage."""
    k, m, n = c.k, c.m, c.n

    def fresh():
        return _full(k, m, _rows_data(rng, nb, k, S))

    def halves(sh):
        return guarded(np.ascontiguousarray(sh[:, :k])), guarded(np.ascontiguousarray(sh[:, k:]))

    def stripe(name, sh, image, verdicts=None, raws=False):
        (db, dp), (pb, pp) = halves(sh)
        bad = host_words(nb * m)
        args = (dp, k * S, pp, m * S, S, nb)
        if name == "verify":
            c.verify_batch_host_ptr(*args, bad.ctypes.data)
        elif name == "scrub":
            raw = host_words(nb * n)
            c.scrub_batch_host_ptr(*args, bad.ctypes.data, raw.ctypes.data)
            assert_raw16(rsmi, spare_host(raw, ctx), sh, ctx + (name,))
        else:
            out = np.full(nb + 1, 0x5EED, dtype=np.int32)
            getattr(c, name + "_batch_host_ptr")(*args, out.ctypes.data, bad.ctypes.data)
            assert out[-1] == 0x5EED and np.array_equal(out[:-1], verdicts), ctx + (name, out.tolist())
        got = spare_host(bad, ctx).reshape(nb, m) != 0
        assert np.array_equal(got, want_flags(k, m, sh)), ctx + (name, "flags")
        assert_guarded(db, np.ascontiguousarray(image[:, :k]), ctx + (name, "data"))
        assert_guarded(pb, np.ascontiguousarray(image[:, k:]), ctx + (name, "parity"))

    def encode(crcs):
        full = fresh()
        before = np.array(full)
        before[:, k:] = 0xEE
        (db, dp), (pb, pp) = halves(before)
        if crcs:
            r16, r32 = host_words(nb * n), host_words(nb * n)
            c.encode_batch_host_crcs_ptr(dp, k * S, pp, m * S, S, nb, r16.ctypes.data, r32.ctypes.data)
            assert_raw16(rsmi, spare_host(r16, ctx), full, ctx + ("encode crcs",))
            assert_raw32(rsmi, spare_host(r32, ctx), full, ctx + ("encode crcs",))
        else:
            c.encode_batch_host_ptr(dp, k * S, pp, m * S, S, nb)
        assert_guarded(db, np.ascontiguousarray(full[:, :k]), ctx + ("encode", crcs, "data"))
        assert_guarded(pb, np.ascontiguousarray(full[:, k:]), ctx + ("encode", crcs, "parity"))

    encode(False)
    sh = damaged(rng, fresh())
    stripe("verify", sh, sh)
    encode(True)
    sh = damaged(rng, fresh())
    stripe("scrub", sh, sh)
    sh = damaged(rng, fresh())
    stripe("locate", sh, sh, want_verdicts(k, m, sh))
    # the mixed reconstruct with R of the rows read and rebuilt, blocks of n rows at pitch S
    present = mr.present_of(n, random_losses(rng, n, m, nb))
    sh = mr.stored(fresh(), present)
    W = mr.wanted(k, present, None, False)
    want_status, image = mr.definition(k, m, sh, present, W)
    buf, ptr = guarded(sh)
    raw = host_words(nb * n)
    got = c.reconstruct_mixed_batch_host_verify_ptr(ptr, n * S, S, nb, mr.u8(present), None, False, raw.ctypes.data)
    assert got == want_status, ctx + ("mixed", got, want_status)
    assert_guarded(buf, image, ctx + ("mixed",))
    mv.assert_raws(rsmi, image, mv.touched(k, present, W, want_status), spare_host(raw, ctx).reshape(nb, n), ctx + ("mixed",))
    sh = damaged(rng, fresh())
    verdicts = want_verdicts(k, m, sh)
    stripe("heal", sh, test_heal.want_image(k, m, sh, verdicts), verdicts)
    # the ragged encode, sizes running through this module's from S
    # (past seven blocks every block has S bytes, so that the rows outgrow small_call_bytes as the
    # other families' do)
    b = Batch(k, m)
    for i in range(nb):
        b.place(S if nb > 7 else SIZES[(SIZES.index(S) + i) % 3], "a", v=int(rng.integers(1 << 30)), gap=i % 3,
                extra=i % 2)
    d_img, p_img, want = b.images()
    (db, dp), (pb, pp) = guarded(d_img), guarded(p_img)
    c.encode_ragged_batch_host_ptr(dp, pp, b.blocks())
    assert_guarded(db, d_img, ctx + ("ragged", "data"))
    assert_guarded(pb, want, ctx + ("ragged", "parity"))
    # both rows passes over 3 nb rows
    rows = _rows_data(rng, 1, 3 * nb, S)[0]
    buf, ptr = guarded(rows)
    r16, r32 = host_words(3 * nb), host_words(3 * nb)
    c.crc_rows_host_ptr(ptr, S, 3 * nb, S, r16.ctypes.data, r32.ctypes.data)
    assert_raw16(rsmi, spare_host(r16, ctx), rows, ctx + ("rows",))
    assert_raw32(rsmi, spare_host(r32, ctx), rows, ctx + ("rows",))
    assert_guarded(buf, rows, ctx + ("rows",))
    encode(False)


@pytest.mark.gpu
def test_host_paths_share_the_staging(gpu):
    """Leg 8: one Codec(10, 4), pageable memory, the host entry points of every family alternating
    over small, large (past small_call_bytes: the chunked upload) and small rows again, so that each
    staging area grows under one family and is reused by the next; then once more with
    small_call_bytes below one call's rows."""
    torch, rsmi, gate = gpu
    with _leg("8"), rsmi.Codec(10, 4) as c:
        rng = np.random.default_rng(0x8)
        assert 3 * 14 * 1025 < (2 << 20) < 40 * 14 * 4097   # the ragged call's 40 blocks of 14 rows at pitch 4112 too
        for S, nb in ((1025, 3), (4097, 40), (16, 5)):
            host_round(rsmi, c, rng, S, nb, ("default", S, nb))
        c.set_option("small_call_bytes", 40000)
        assert 3 * 14 * 4097 > 40000 and 5 * 14 * 1025 > 40000
        for S, nb in ((4097, 3), (1025, 5)):
            host_round(rsmi, c, rng, S, nb, ("small_call_bytes 40000", S, nb))
