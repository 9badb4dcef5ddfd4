"""rsmi_scrub on the GPU against the CPU oracles, exactly: Verify's flags and every shard's CRC-16
from one read of the rows.

Every expected value comes from the definition over the rows as stored:
  flags  want[b, j] = (oracle encode of block b's data rows)[j] != stored parity row j, in [0, S)
  raws   crc16_ibm(row) (the byte-serial oracle) == rsmi.crc16_entry(b"", raw, S), which at fixed S
         is a bijection of raw; rows of up to 2 KiB are also compared with test_crc16.raw_crc itself
and each test also states them from where it put the damage; the two must agree before the GPU's
answer is looked at.  There are no tolerances.  The cases are a few MB each.

  1  the sizes at which the kernel can go wrong, RS(10,4) and RS(4,2), both layouts; the padding trap
  2  the shapes of the accumulator pairing
  3  a sheet of aimed damage in one call, and damage that cancels in the syndrome
  4  UA: damage inside the overlapping last window (the shift correction)
  5  independent halves: each term of the alignment predicate broken alone
  6  stream order behind a delayed side stream; the scratch regrow, on two streams
  7  block strides past 2^32 on both halves
  8  shapes without an rs_scrub_mfma_kernel: the two passes
  9  host paths: page-locked in place, the small call, the pipeline past one chunk; Erasure.scrub
"""
import ctypes

import numpy as np
import pytest

import oracle_lib as orc
from test_crc16 import raw_crc
from test_verify import GAP, PAD_DATA, PAD_PARITY, Lay, assert_mds, stripes, want_flags

NB = 3
TILE = 1024   # 64 lanes x 16 bytes
UNIT = 4096   # 4 tiles: one workgroup
GUARD = 8     # words around each output
POISON_BAD, POISON_RAW, GUARD_WORD = 0x5EED, 0x7EA5, 0x6A6A


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    rsmi = pytest.importorskip("rsmi")
    if not torch.cuda.is_available() or rsmi.device_count() == 0:
        pytest.skip("no GPU")
    return torch, rsmi


def scrub_label(k, m, aligned):
    return "rs_scrub_mfma_kernel<K=%d,MT=%d>%s" % (k, m, "" if aligned else ",UA")


def want_entries(shards):
    """crc16_ibm of every row as stored: (nb, n)."""
    nb, n, _ = shards.shape
    return np.array([[orc.crc16_ibm(shards[b, r].tobytes()) for r in range(n)] for b in range(nb)], dtype=np.uint32)


def entries_of(rsmi, raws, S):
    """The checksum each raw finishes to (rsmi_crc16_entry with an empty header)."""
    return np.array([[rsmi.crc16_entry(b"", int(x), S) for x in row] for row in raws], dtype=np.uint32)


def assert_raws(rsmi, got_raws, shards, ctx):
    """got_raws (nb, n) against the rows as stored."""
    S = shards.shape[2]
    assert (got_raws >> 16 == 0).all(), ("R(shard) is 16 bits in a uint32", ctx)
    want = want_entries(shards)
    got = entries_of(rsmi, got_raws, S)
    if not np.array_equal(got, want):
        diff = np.argwhere(got != want)
        raise AssertionError("%r: %d checksums differ, first (block, row) = %r: got %#x, want %#x" %
                             (ctx, len(diff), tuple(diff[0]), got[tuple(diff[0])], want[tuple(diff[0])]))
    if S <= 2085:
        loop = np.array([[raw_crc(shards[b, r].tobytes()) for r in range(shards.shape[1])]
                         for b in range(shards.shape[0])], dtype=np.uint32)
        assert np.array_equal(got_raws, loop), ("raw_crc", ctx)


class Outputs:
    """The two device outputs, pre-filled with garbage (the call must zero what it accumulates
    into), each between guard words."""

    def __init__(self, torch, nb, k, m):
        self.nb, self.m, self.n = nb, m, k + m
        self.bad = torch.full((2 * GUARD + nb * m,), POISON_BAD, dtype=torch.int32, device="cuda")
        self.raw = torch.full((2 * GUARD + nb * (k + m),), POISON_RAW, dtype=torch.int32, device="cuda")
        for t in (self.bad, self.raw):
            t[:GUARD] = GUARD_WORD
            t[-GUARD:] = GUARD_WORD
        self.bad_ptr = self.bad.data_ptr() + 4 * GUARD
        self.raw_ptr = self.raw.data_ptr() + 4 * GUARD

    def read(self):
        bad, raw = self.bad.cpu().numpy(), self.raw.cpu().numpy()
        for a in (bad, raw):
            assert (a[:GUARD] == GUARD_WORD).all() and (a[-GUARD:] == GUARD_WORD).all(), "a guard word was written"
        return (bad[GUARD:-GUARD].reshape(self.nb, self.m) != 0,
                raw[GUARD:-GUARD].astype(np.uint32).reshape(self.nb, self.n))


def run_dev(torch, c, lay, host, label, stream=None):
    """rsmi_scrub_batch_dev over host's bytes: (flags (nb, m) bool, raws (nb, n) uint32).  The buffer
    must come back byte for byte, the guards untouched, the label as stated (a str, or a predicate)."""
    d = torch.from_numpy(host.copy()).cuda()
    assert d.data_ptr() % 256 == 0
    out = Outputs(torch, lay.nb, lay.k, lay.m)
    base = d.data_ptr() + lay.off
    torch.cuda.synchronize()
    st = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(st):
        c.scrub_batch_dev(base, lay.rs, lay.bs, base + lay.k * lay.rs, lay.rs, lay.bs, lay.S, lay.nb, out.bad_ptr,
                          out.raw_ptr, st.cuda_stream)
    st.synchronize()
    if callable(label):
        assert label(c.last_kernel()), c.last_kernel()
    else:
        assert c.last_kernel() == label, (c.last_kernel(), label)
    assert np.array_equal(d.cpu().numpy(), host), "scrub wrote to the shards"
    return out.read()


def check(torch, rsmi, c, lay, host, label, want, ctx, stream=None):
    """want (from the construction) must equal the oracle's flags over the rows as stored; then the
    GPU's flags must equal both and its raws the rows' checksums.  Returns the raws."""
    rows = lay.rows(host)
    assert np.array_equal(want_flags(lay.k, lay.m, rows), want), ("oracle", ctx)
    flags, raws = run_dev(torch, c, lay, host, label, stream)
    if not np.array_equal(flags, want):
        diff = np.argwhere(flags != want)
        raise AssertionError("%r: %d flags differ, first (block, row) = %r" % (ctx, len(diff), tuple(diff[0])))
    assert_raws(rsmi, raws, rows, ctx)
    return raws


def fill_padded(lay, shards):
    """Lay.fill, then every padding byte of row r of block b a sentinel of its own: non-zero and
    different from row to row."""
    host = lay.fill(shards)
    if lay.rs > lay.S:
        for b in range(lay.nb):
            for r in range(lay.n):
                o = lay.off + b * lay.bs + r * lay.rs
                host[o + lay.S:o + lay.rs] = 1 + (7 * r + 13 * b) % 255
    return host


# ---------------------------------------------------------------- 1: the sizes, the padding trap
SIZES = [1, 15, 16, 17, 1023, 1024, 1025, 2085, 4095, 4096, 4097, 5125, 26215, 32767, 32768, 40000]


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
@pytest.mark.parametrize("k,m", [(10, 4), (4, 2)])
def test_sizes(gpu, k, m, aligned):
    """Clean stripes, then one block with a damaged parity row and one with a damaged data row, at
    the smallest rows, the tile seam, a 5-byte last chunk, the unit seam (4 tiles), a last unit of
    two tiles, the headline row (7 units, the last of 2 tiles) and around the CRC's order (A^32767
    = I: the shift's exponent wraps).  Aligned: every padding byte a per-row sentinel, and the
    outputs do not change when the padding byte at S of every row is flipped."""
    torch, rsmi = gpu
    assert_mds(rsmi, k, m)
    label = scrub_label(k, m, aligned)
    with rsmi.Codec(k, m) as c:
        for S in SIZES:
            if not aligned and S < 16:
                continue  # unaligned rows shorter than a window: the two passes (test_fallback)
            lay = Lay(rsmi, k, m, S, NB, aligned)
            full = stripes(k, m, S)
            host = fill_padded(lay, full)
            raws = check(torch, rsmi, c, lay, host, label, np.zeros((NB, m), dtype=bool), (k, m, S, aligned, "clean"))
            if aligned and lay.rs > S:
                flipped = host.copy()
                for b in range(NB):
                    for r in range(k + m):
                        flipped[lay.off + b * lay.bs + r * lay.rs + S] ^= 0xFF
                f2, r2 = run_dev(torch, c, lay, flipped, label)
                assert not f2.any() and np.array_equal(r2, raws), (k, m, S, "padding byte at S")
            sh = full.copy()
            sh[1, k + m - 1, S - 1] ^= 0x80
            sh[2, 0, 0] ^= 0x01
            want = np.zeros((NB, m), dtype=bool)
            want[1, m - 1] = True
            want[2, :] = True
            r3 = check(torch, rsmi, c, lay, fill_padded(lay, sh), label, want, (k, m, S, aligned, "damaged"))
            changed = r3 != raws
            expect = np.zeros_like(changed)
            expect[1, k + m - 1] = expect[2, 0] = True
            assert np.array_equal(changed, expect), (k, m, S, aligned, np.argwhere(changed))


# ---------------------------------------------------------------- 2: the accumulator pairing
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
@pytest.mark.parametrize("k,m", [(2, 1), (3, 2), (1, 1), (6, 3), (16, 4)])
def test_accumulator_pairing(gpu, k, m, aligned):
    """Two shards share an f32 accumulator: odd shard counts (3, 5, 9), the smallest stripe, and 20
    shards in 10 accumulators.  Every row differs, so a count that lands in its neighbour's half
    (or in another accumulator) gives both rows a wrong checksum."""
    torch, rsmi = gpu
    assert_mds(rsmi, k, m)
    label = scrub_label(k, m, aligned)
    with rsmi.Codec(k, m) as c:
        for S in (17, 4097, 5125):
            lay = Lay(rsmi, k, m, S, NB, aligned)
            full = stripes(k, m, S)
            raws = check(torch, rsmi, c, lay, fill_padded(lay, full), label, np.zeros((NB, m), dtype=bool),
                         (k, m, S, "clean"))
            for r in sorted({0, k - 1, k, k + m - 1}):  # both halves of the first and last accumulators
                sh = full.copy()
                sh[1, r, S // 2] ^= 0x10
                want = np.zeros((NB, m), dtype=bool)
                if r < k:
                    want[1, :] = True
                else:
                    want[1, r - k] = True
                got = check(torch, rsmi, c, lay, fill_padded(lay, sh), label, want, (k, m, S, "row", r))
                expect = np.zeros((NB, k + m), dtype=bool)
                expect[1, r] = True
                assert np.array_equal(got != raws, expect), (k, m, S, r)


# ---------------------------------------------------------------- 3: a sheet of damage
SHEET_S = 5125   # 6 tiles = a unit of 4 and a unit of 2; 320 full chunks and a last chunk of 5 bytes
# one byte in each dword of a chunk; the tile seams; the unit seam; the last full chunk and the
# first and last byte of the partial chunk
SHEET_POS = [0, 5, 10, 15, 1023, 1024, 2047, 2048, 4095, 4096, 5119, 5120, 5124]


def sheet(rsmi, k, m, S, positions, aligned):
    """One call's worth of aimed damage, one block per damage and one clean block last: (lay, host,
    want flags, the rows whose raw differs from the clean stripe's, the clean shards).
    Parity row j alone, one bit flipped, at every position: exactly flag (b, j) and that row's raw.
    Data row 0 and data row k - 1, one bit: all m flags (the code is MDS) and that row's raw."""
    dmg = [("parity", j, p) for j in range(m) for p in positions]
    dmg += [("data", 0, positions[len(positions) // 2]), ("data", k - 1, positions[-1])]
    nb = len(dmg) + 1
    lay = Lay(rsmi, k, m, S, nb, aligned)
    full = stripes(k, m, S, nb)
    sh = full.copy()
    want = np.zeros((nb, m), dtype=bool)
    moved = np.zeros((nb, k + m), dtype=bool)
    for b, (kind, r, p) in enumerate(dmg):
        if kind == "parity":
            sh[b, k + r, p] ^= 1 << ((p + r) % 8)
            want[b, r] = True
            moved[b, k + r] = True
        else:
            sh[b, r, p] ^= 1 << (p % 8)
            want[b, :] = True
            moved[b, r] = True
    assert not want[nb - 1].any() and not moved[nb - 1].any()
    return lay, fill_padded(lay, sh), want, moved, full


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
@pytest.mark.parametrize("k,m", [(10, 4), (4, 2)])
def test_damage_sheet(gpu, k, m, aligned):
    torch, rsmi = gpu
    assert_mds(rsmi, k, m)
    with rsmi.Codec(k, m) as c:
        lay, host, want, moved, full = sheet(rsmi, k, m, SHEET_S, SHEET_POS, aligned)
        raws = check(torch, rsmi, c, lay, host, scrub_label(k, m, aligned), want, (k, m, aligned, "sheet"))
        clean = want_entries(full)
        assert np.array_equal(entries_of(rsmi, raws, SHEET_S) != clean, moved), "a raw moved that was not damaged"


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
@pytest.mark.parametrize("k,m", [(10, 4), (4, 2)])
def test_cancelling_damage(gpu, k, m, aligned):
    """A data row and all parity rows rewritten consistently: the syndrome is zero, so the flags are
    clean, and the raws are those of the new bytes (a checksum kept from the write would catch this;
    Verify cannot)."""
    torch, rsmi = gpu
    S = 4097
    lay = Lay(rsmi, k, m, S, NB, aligned)
    full = stripes(k, m, S)
    sh = full.copy()
    sh[1, k // 2, 4096] ^= 0x5A
    sh[1, k // 2, 77] ^= 0x01
    sh[1, k:] = orc.encode(k, m, np.ascontiguousarray(sh[1, :k]))
    moved = (sh != full).any(axis=2)
    assert moved[1, k // 2] and moved[1, k:].all() and moved.sum() == 1 + m
    with rsmi.Codec(k, m) as c:
        raws = check(torch, rsmi, c, lay, fill_padded(lay, sh), scrub_label(k, m, aligned),
                     np.zeros((NB, m), dtype=bool), (k, m, aligned, "cancel"))
        assert np.array_equal(entries_of(rsmi, raws, S) != want_entries(full), moved)


# ---------------------------------------------------------------- 4: UA, the overlapping last window
@pytest.mark.gpu
@pytest.mark.parametrize("S", [1025, 1032, 1039, 4097, 5128, 26215])
@pytest.mark.parametrize("k,m", [(10, 4), (4, 2)])
def test_ua_last_window(gpu, k, m, S):
    """Rows at pitch S from an odd base, S = 1, 8 and 15 mod 16 (26 215 = 7 mod 16: the headline):
    the row's last window [S - 16, S) overlaps the chunk before it.  The syndrome sees the
    overlapped bytes twice, the fold must see every byte once, at its place: one flipped bit at the
    window's first byte, on each side of the chunk boundary inside it, and at S - 1, in a data row
    and in a parity row."""
    torch, rsmi = gpu
    assert S % 16 in (1, 7, 8, 15)
    edge = (S - 1) // 16 * 16  # the last chunk's first byte
    pos = [S - 16, edge - 1, edge, S - 1]
    assert S - 16 <= edge - 1 < edge <= S - 1  # [S - 16, edge) is the overlap
    dmg = [(r, p) for r in (0, k - 1, k, k + m - 1) for p in pos]
    nb = len(dmg) + 1
    lay = Lay(rsmi, k, m, S, nb, False)
    assert lay.rs == S and lay.off % 2 == 1
    full = stripes(k, m, S, nb)
    sh = full.copy()
    want = np.zeros((nb, m), dtype=bool)
    moved = np.zeros((nb, k + m), dtype=bool)
    for b, (r, p) in enumerate(dmg):
        sh[b, r, p] ^= 1 << (b % 8)
        moved[b, r] = True
        if r < k:
            want[b, :] = True
        else:
            want[b, r - k] = True
    with rsmi.Codec(k, m) as c:
        raws = check(torch, rsmi, c, lay, lay.fill(sh), scrub_label(k, m, False), want, (k, m, S, "window"))
        assert np.array_equal(entries_of(rsmi, raws, S) != want_entries(full), moved)


# ---------------------------------------------------------------- 5: independent halves
def run_halves(torch, rsmi, c, shards, geo, label):
    """Data and parity rows in two allocations, each with its own byte phase, pitch and block
    stride (geo: d_off, d_rs, d_bs, p_off, p_rs, p_bs); everything that is not a row byte holds a
    sentinel.  Both allocations must come back whole."""
    nb, n, S = shards.shape
    k, m = c.k, c.m
    d_off, d_rs, d_bs, p_off, p_rs, p_bs = geo
    assert d_rs >= S and p_rs >= S and d_bs >= k * d_rs and p_bs >= m * p_rs
    hd = np.full(d_off + nb * d_bs + 64, PAD_DATA, dtype=np.uint8)
    hp = np.full(p_off + nb * p_bs + 64, PAD_PARITY, dtype=np.uint8)
    np.lib.stride_tricks.as_strided(hd[d_off:], shape=(nb, k, S), strides=(d_bs, d_rs, 1))[:] = shards[:, :k]
    np.lib.stride_tricks.as_strided(hp[p_off:], shape=(nb, m, S), strides=(p_bs, p_rs, 1))[:] = shards[:, k:]
    dd, dp = torch.from_numpy(hd.copy()).cuda(), torch.from_numpy(hp.copy()).cuda()
    assert dd.data_ptr() % 256 == 0 and dp.data_ptr() % 256 == 0
    out = Outputs(torch, nb, k, m)
    c.scrub_batch_dev(dd.data_ptr() + d_off, d_rs, d_bs, dp.data_ptr() + p_off, p_rs, p_bs, S, nb, out.bad_ptr,
                      out.raw_ptr, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert c.last_kernel() == label, (geo, c.last_kernel(), label)
    assert np.array_equal(dd.cpu().numpy(), hd) and np.array_equal(dp.cpu().numpy(), hp), "scrub wrote to a half"
    return out.read()


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", [(10, 4), (4, 2)])
def test_independent_halves(gpu, k, m):
    """The aligned kernel needs both bases, both pitches and both block strides on the 16-byte
    grid.  All six hold: the aligned label.  Each broken alone: the UA label.  The answers are the
    same whole way through, on clean stripes and on one with damage in each half."""
    torch, rsmi = gpu
    S = 1025
    full = stripes(k, m, S)
    sh = full.copy()
    sh[0, k + m - 1, S - 1] ^= 0x02
    sh[2, k - 1, 1024] ^= 0x40
    want = np.zeros((NB, m), dtype=bool)
    want[0, m - 1] = True
    want[2, :] = True
    assert np.array_equal(want_flags(k, m, sh), want)
    up = lambda x: (x + 15) // 16 * 16
    base = (0, 1088, k * 1088 + 64, 0, 1056, m * 1056 + 32)
    cases = [
        (base, True),
        ((5,) + base[1:], False),                                                # data base
        (base[:3] + (9,) + base[4:], False),                                     # parity base
        ((0, 1089, up(k * 1089)) + base[3:], False),                             # data pitch
        ((0, 1088, k * 1088 + 72) + base[3:], False),                            # data block stride
        (base[:3] + (0, 1057, up(m * 1057)), False),                             # parity pitch
        (base[:3] + (0, 1056, m * 1056 + 36), False),                            # parity block stride
    ]
    with rsmi.Codec(k, m) as c:
        for geo, aligned in cases:
            broken = [geo[0] % 16, geo[1] % 16, geo[2] % 16, geo[3] % 16, geo[4] % 16, geo[5] % 16]
            assert sum(1 for x in broken if x) == (0 if aligned else 1), geo
            for shards, w in ((full, np.zeros((NB, m), dtype=bool)), (sh, want)):
                flags, raws = run_halves(torch, rsmi, c, shards, geo, scrub_label(k, m, aligned))
                assert np.array_equal(flags, w), (geo, flags)
                assert_raws(rsmi, raws, shards, geo)


# ---------------------------------------------------------------- 6: stream order, scratch
@pytest.mark.gpu
def test_stream_order(gpu):
    """The call runs behind a delayed side stream with no host sync: the input arrives, and the
    outputs are poisoned, only in that stream's order, behind the delay; the outputs are cloned and
    overwritten in that stream right behind the call.  The delay has not ended when the call
    returns, and after the stream's event the clones hold the answers."""
    torch, rsmi = gpu
    from test_stream_order import Gate
    gate = Gate(torch)
    k, m, S, nb = 10, 4, 5125, 3
    lay = Lay(rsmi, k, m, S, nb, True)
    sh = stripes(k, m, S, nb).copy()
    sh[1, k + 2, 4096] ^= 0x08
    want = np.zeros((nb, m), dtype=bool)
    want[1, 2] = True
    assert np.array_equal(want_flags(k, m, sh), want)
    host = fill_padded(lay, sh)
    pinned = torch.from_numpy(host).pin_memory()
    st = torch.cuda.Stream()
    with rsmi.Codec(k, m) as c:
        for gated in (False, True):  # the first pass builds the plan, the tables and the scratch
            d = torch.full((lay.size,), 0xEE, dtype=torch.uint8, device="cuda")
            bad = torch.full((nb * m,), 0x0BAD, dtype=torch.int32, device="cuda")
            raw = torch.full((nb * (k + m),), 0x0BAD, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            e1, e2 = torch.cuda.Event(), torch.cuda.Event()
            with torch.cuda.stream(st):
                if gated:
                    gate()
                e1.record()
                d.copy_(pinned, non_blocking=True)
                bad.fill_(0x0BAD)
                raw.fill_(0x0BAD)
                base = d.data_ptr() + lay.off
                c.scrub_batch_dev(base, lay.rs, lay.bs, base + k * lay.rs, lay.rs, lay.bs, S, nb, bad.data_ptr(),
                                  raw.data_ptr(), st.cuda_stream)
                bad2, raw2 = bad.clone(), raw.clone()
                bad.fill_(-1)
                raw.fill_(-1)
                e2.record()
            if gated:
                assert not e1.query(), "the call waited for the stream"
            e2.synchronize()
            assert c.last_kernel() == scrub_label(k, m, True)
            assert np.array_equal(bad2.cpu().numpy().reshape(nb, m) != 0, want), gated
            assert_raws(rsmi, raw2.cpu().numpy().astype(np.uint32).reshape(nb, k + m), sh, ("stream order", gated))
            assert (bad.cpu().numpy() == -1).all() and (raw.cpu().numpy() == -1).all(), "a launch ran late"


@pytest.mark.gpu
def test_scratch_regrow_two_streams(gpu):
    """One context: a small call and then a larger one on one stream (the record scratch is freed
    and reallocated behind the first), then the same pair on a second stream, which has a scratch
    of its own; then the small call again in the larger scratch."""
    torch, rsmi = gpu
    k, m = 4, 2
    with rsmi.Codec(k, m) as c:
        for st in (torch.cuda.Stream(), torch.cuda.Stream()):
            for S, nb, (b, r, p) in ((1025, 2, (1, k + 1, 1024)), (40000, 9, (7, 1, 39999)), (1025, 2, (0, k, 0))):
                lay = Lay(rsmi, k, m, S, nb, True)
                sh = stripes(k, m, S, nb).copy()
                sh[b, r, p] ^= 0x20
                want = np.zeros((nb, m), dtype=bool)
                if r < k:
                    want[b, :] = True
                else:
                    want[b, r - k] = True
                check(torch, rsmi, c, lay, fill_padded(lay, sh), scrub_label(k, m, True), want, (S, nb), stream=st)


# ---------------------------------------------------------------- 7: offsets past 4 GiB
def _far_case(torch, rsmi, c, dd, dp, off, S, bs, aligned, seed):
    """RS(4,2), two blocks, rows written one by one into two allocations that are otherwise not
    filled; the second block lies past 2^32 in both.  A truncated offset reads the first block or
    bytes no row was written to."""
    k, m, nb = 4, 2, 2
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 256, size=(nb, k, S), dtype=np.uint8)
    sh = np.concatenate([data, np.stack([orc.encode(k, m, data[b]) for b in range(nb)])], axis=1)
    sh[0, k + 0, 1033] ^= 0x10
    sh[1, k + 1, 3] ^= 0x02
    want = np.zeros((nb, m), dtype=bool)
    want[0, 0] = want[1, 1] = True
    assert np.array_equal(want_flags(k, m, sh), want)
    for b in range(nb):
        for i in range(k):
            o = off + b * bs + i * S
            dd[o:o + S].copy_(torch.from_numpy(sh[b, i]))
        for j in range(m):
            o = off + b * bs + j * S
            dp[o:o + S].copy_(torch.from_numpy(sh[b, k + j]))
    out = Outputs(torch, nb, k, m)
    c.scrub_batch_dev(dd.data_ptr() + off, S, bs, dp.data_ptr() + off, S, bs, S, nb, out.bad_ptr, out.raw_ptr,
                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert c.last_kernel() == scrub_label(k, m, aligned), c.last_kernel()
    flags, raws = out.read()
    assert np.array_equal(flags, want), (off, flags)
    assert_raws(rsmi, raws, sh, ("far", off))
    for b in range(nb):  # nothing written
        o = off + b * bs
        assert np.array_equal(dd[o:o + k * S].cpu().numpy(), sh[b, :k].reshape(-1)), b
        assert np.array_equal(dp[o:o + m * S].cpu().numpy(), sh[b, k:].reshape(-1)), b


@pytest.mark.gpu
def test_offsets_past_4gib(gpu):
    """Two blocks at block_stride = 2^32 + 256 on both halves, aligned and shifted by one byte."""
    torch, rsmi = gpu
    if torch.cuda.mem_get_info()[0] < 12 << 30:
        pytest.skip("needs 12 GiB of free device memory")
    S, bs = 1040, 2 ** 32 + 256
    try:
        with rsmi.Codec(4, 2) as c:
            dd = torch.empty(2 ** 32 + 2 ** 20, dtype=torch.uint8, device="cuda")
            dp = torch.empty(2 ** 32 + 2 ** 20, dtype=torch.uint8, device="cuda")
            assert 1 + bs + 4 * S <= dd.numel()
            _far_case(torch, rsmi, c, dd, dp, 0, S, bs, True, 5001)
            _far_case(torch, rsmi, c, dd, dp, 1, S, bs, False, 5002)
            del dd, dp
    finally:
        torch.cuda.empty_cache()


# ---------------------------------------------------------------- 8: the two passes
@pytest.mark.gpu
@pytest.mark.parametrize("k,m,S,aligned", [(5, 5, 1040, True), (5, 5, 1040, False), (7, 2, 1025, True),
                                           (20, 4, 333, True), (4, 2, 9, False)],
                         ids=["5-5", "5-5-split", "7-2", "20-4", "4-2-S9-pitch9"])
def test_fallback(gpu, k, m, S, aligned):
    """m > 4 (two plan tiles), a K without an instantiation, K > 16, and unaligned rows shorter than
    16 bytes: Verify and the CRC-16 rows pass on the same stream.  The outputs equal the definition
    and the label is not the scrub kernel's."""
    torch, rsmi = gpu
    lay = Lay(rsmi, k, m, S, NB, aligned)
    assert aligned or lay.rs == S
    full = stripes(k, m, S)
    other = lambda s: bool(s) and not s.startswith("rs_scrub")
    with rsmi.Codec(k, m) as c:
        check(torch, rsmi, c, lay, fill_padded(lay, full), other, np.zeros((NB, m), dtype=bool), (k, m, S, "clean"))
        sh = full.copy()
        sh[1, k + m - 1, S - 1] ^= 0x10
        sh[2, k - 1, 0] ^= 0x01
        want = np.zeros((NB, m), dtype=bool)
        want[1, m - 1] = True
        want[2, :] = True
        check(torch, rsmi, c, lay, fill_padded(lay, sh), other, want, (k, m, S, "damaged"))


# ---------------------------------------------------------------- 9: host paths
def _host_scrub(c, data, dbs, parity, pbs, S, nb):
    bad = np.full(nb * c.m, POISON_BAD, dtype=np.uint32)
    raw = np.full(nb * c.n, POISON_RAW, dtype=np.uint32)
    c.scrub_batch_host_ptr(data, dbs, parity, pbs, S, nb, bad.ctypes.data, raw.ctypes.data)
    return bad.reshape(nb, c.m) != 0, raw.reshape(nb, c.n)


@pytest.mark.gpu
def test_host_page_locked_in_place(gpu):
    """Data and parity in one rsmi_host_alloc allocation: one kernel reads them in place at pitch S,
    the unaligned-window form, once."""
    torch, rsmi = gpu
    k, m, S, nb = 4, 2, 5125, 5
    full = stripes(k, m, S, nb)
    L = rsmi.lib()
    size = nb * (k + m) * S
    p = L.rsmi_host_alloc(size)
    assert p
    try:
        buf = np.ctypeslib.as_array((ctypes.c_uint8 * size).from_address(p))
        rows = buf.reshape(nb, k + m, S)
        with rsmi.Codec(k, m) as c:
            c.set_option("zero_copy", 1)
            bs = (k + m) * S
            for damage in (None, (3, k + 1, S - 1), (4, 0, 0)):
                rows[:] = full
                if damage:
                    rows[damage] ^= 0x20
                want = want_flags(k, m, rows)
                assert want.any() == (damage is not None)
                before = buf.copy()
                flags, raws = _host_scrub(c, p, bs, p + k * S, bs, S, nb)
                assert c.last_kernel() == scrub_label(k, m, False)
                assert np.array_equal(buf, before)
                assert np.array_equal(flags, want), (damage, flags)
                assert_raws(rsmi, raws, rows, damage)
    finally:
        L.rsmi_host_free(p)


@pytest.mark.gpu
def test_host_small_pageable_and_one_block(gpu):
    """A small pageable batch goes through the page-locked staging; rsmi_scrub of one block, clean
    and dirty."""
    torch, rsmi = gpu
    for k, m, S in ((2, 1, 2049), (10, 4, 4099)):
        nb = 3
        full = stripes(k, m, S, nb)
        assert nb * (k + m) * S * 2 <= (2 << 20)
        with rsmi.Codec(k, m) as c:
            sh = full.copy()
            sh[1, k, S - 1] ^= 0x04
            data, parity = np.ascontiguousarray(sh[:, :k]), np.ascontiguousarray(sh[:, k:])
            d0, p0 = data.copy(), parity.copy()
            flags, raws = _host_scrub(c, data.ctypes.data, k * S, parity.ctypes.data, m * S, S, nb)
            assert c.last_kernel() == scrub_label(k, m, False)
            assert np.array_equal(data, d0) and np.array_equal(parity, p0)
            want = np.zeros((nb, m), dtype=bool)
            want[1, 0] = True
            assert np.array_equal(want_flags(k, m, sh), want) and np.array_equal(flags, want)
            assert_raws(rsmi, raws, sh, (k, m, "small"))

            one = bytearray(full[0].tobytes())
            ok, raw = c.scrub(one, S)
            assert ok is True and bytes(one) == full[0].tobytes()
            assert_raws(rsmi, np.array([raw], dtype=np.uint32), full[:1], (k, m, "one clean"))
            one[(k + m - 1) * S + S - 1] ^= 0x01
            ok, raw2 = c.scrub(one, S)
            assert ok is False and raw2[:-1] == raw[:-1] and raw2[-1] != raw[-1]
            one[(k + m - 1) * S + S - 1] ^= 0x01
            one[0] ^= 0x80
            ok, raw3 = c.scrub(one, S)
            assert ok is False and raw3[1:] == raw[1:] and raw3[0] != raw[0]
            got = np.frombuffer(bytes(one), dtype=np.uint8).reshape(1, k + m, S)
            assert_raws(rsmi, np.array([raw3], dtype=np.uint32), got, (k, m, "one dirty"))


@pytest.mark.gpu
def test_host_pipeline_past_one_chunk(gpu):
    """RS(2,1), S = 65 537: one block more than a 64 MiB chunk of the upload pipeline holds, the
    data page-locked and the parity pageable (so nothing is read in place).  Damage in the first
    block, on each side of the chunk seam and in the last block; flags and raws whole."""
    torch, rsmi = gpu
    k, m, S = 2, 1, 65537
    chunk = max(1, (64 << 20) // (3 * rsmi.recommended_pitch(S)))
    nb = chunk + 2
    assert nb * 3 * S > (2 << 20)
    rng = np.random.default_rng(9)
    L = rsmi.lib()
    p = L.rsmi_host_alloc(nb * k * S)
    assert p
    try:
        data = np.ctypeslib.as_array((ctypes.c_uint8 * (nb * k * S)).from_address(p)).reshape(nb, k, S)
        data[:] = rng.integers(0, 256, size=(nb, k, S), dtype=np.uint8)
        parity = orc.encode_fast(k, m, data, threads=8)
        for b in (0, chunk, nb - 1):
            assert np.array_equal(orc.encode(k, m, data[b]), parity[b]), b
        want = np.zeros((nb, m), dtype=bool)
        for i, b in enumerate((0, chunk - 1, chunk, nb - 1)):
            parity[b, 0, (i * 21101) % S] ^= 1 << i
            want[b, 0] = True
        data[chunk + 1, 1, S - 1] ^= 0x01
        want[chunk + 1, 0] = True
        with rsmi.Codec(k, m) as c:
            d0, p0 = data.copy(), parity.copy()
            flags, raws = _host_scrub(c, p, k * S, parity.ctypes.data, m * S, S, nb)
            assert c.last_kernel() == scrub_label(k, m, True)
            assert np.array_equal(data, d0) and np.array_equal(parity, p0)
            assert np.array_equal(np.flatnonzero(flags[:, 0]), np.flatnonzero(want[:, 0]))
            assert_raws(rsmi, raws, np.concatenate([data, parity], axis=1), "pipeline")
    finally:
        L.rsmi_host_free(p)


@pytest.mark.gpu
def test_erasure_scrub_round_trip(gpu):
    """encode_data, then scrub: ok, and the raws encode_block_crc returns for the same block; a
    swapped pair of shards: not ok, and the two raws swap with them."""
    torch, rsmi = gpu
    for k, m, B in ((10, 4, 262144), (4, 2, 4099), (10, 4, 6)):
        block = orc.splitmix64_bytes(0x5C3B + B, B).tobytes()
        e = rsmi.NewErasure(k, m, B)
        shards = e.encode_data(block)
        ok, raws = e.scrub(shards)
        flat, want = e.encoder().encode_block_crc(block)
        assert flat == b"".join(shards)
        assert ok is True and raws == want, (k, m, B)
        if B > 6:
            sw = list(shards)
            sw[1], sw[k] = sw[k], sw[1]
            ok, r2 = e.scrub(sw)
            want2 = list(want)
            want2[1], want2[k] = want2[k], want2[1]
            assert ok is False and r2 == want2
        e._codec.close()
