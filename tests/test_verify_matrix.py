"""Every instantiated verify kernel, and the code around it, against the CPU oracle, exactly.

rs_verify_kernels.hip builds rs_verify_kernel<K, MT, UA> for K in VERIFY_KS x MT in 1..4 x both
layouts: 80 kernels, each its own unrolled code with its own ring geometry (P = min(K, MT <= 2 ?
16 : 6) rows in flight, parity row j in slot (K - P + j) % P, and with K < MT the parity rows
without a slot in xs[]).  This module runs every one of them on clean stripes and on a sheet of
aimed damage, proves by the launch label that the instantiation was reached, and then runs what
test_verify.py leaves out of launch_verify: the seams between launch tiles, offsets past 2^32, the
fallback's two grid-stride loops, its 64 MiB scratch chunks and the scratch regrow.  The host
paths are in test_verify_host.py.

Every expected flag is stated twice: from where the damage was put, and from the oracle's encode
of the data rows as stored (want_flags).  The two must agree before the GPU's answer is looked
at.  Everything is bit-exact: there are no tolerances.

  0  VERIFY_KS equals the dispatch table of the source (CPU)
  1  all 80 instantiations, clean and damaged
  2  plans of two and three launch tiles: flag[j] = out_row[j] across every seam
  3  block and shard strides past 2^32
  4  the fallback: rs_compare_rows_kernel's x and y loops, the scratch chunk seam, the regrow
"""
import os
import re
import time

import numpy as np
import pytest

import oracle_lib as orc
from test_verify import GAP, NB, PAD_DATA, PAD_PARITY, Lay, assert_mds, run_dev, stripes, want_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "filedag-storage_amd", "csrc")

# ---------------------------------------------------------------- the dispatch table, restated
VERIFY_KS = [1, 2, 3, 4, 5, 6, 8, 10, 12, 16]   # fill_verify_k<K>: fn and ua for MT = 1..4
MTS = [1, 2, 3, 4]                              # fill_verify_km<K, MT> inside fill_verify_k
COMPARE = "rs_compare_rows_kernel"


def verify_label(K, MT, aligned):
    return "rs_verify_kernel<K=%d,MT=%d>%s" % (K, MT, "" if aligned else ",UA")


def all_labels():
    return {verify_label(K, MT, a) for K in VERIFY_KS for MT in MTS for a in (True, False)}


# every instantiation a test of this module ran and asserted by its exact label
SEEN = set()
WALL = {}


# ---------------------------------------------------------------- leg 0: the table matches the source
def test_table_matches_source():
    """VERIFY_KS equals the arguments of fill_verify_k in rs_verify_kernels.hip and those of
    fill_k in rs_kernels.hip (the source says they are the same K), and fill_verify_km expands to
    MT = 1..4: a verify kernel added without extending this sweep fails the CPU suite."""
    with open(os.path.join(CSRC, "rs_verify_kernels.hip")) as f:
        src = f.read()
    with open(os.path.join(CSRC, "rs_kernels.hip")) as f:
        coding = f.read()
    assert [int(x) for x in re.findall(r"\bfill_verify_k<\s*(\d+)\s*>\s*\(", src)] == VERIFY_KS
    assert re.findall(r"\bfill_verify_km<K,\s*(\d+)>\(", src) == [str(m) for m in MTS]
    assert [int(x) for x in re.findall(r"\bfill_k<\s*(\d+)\s*>\s*\(", coding)] == VERIFY_KS
    # one fn and one ua entry per (K, MT), nothing else fills the table
    assert len(re.findall(r"&rs_verify_kernel<", src)) == 2
    assert re.search(r"t\.fn\[K\]\[MT\] = reinterpret_cast<void\*>\(&rs_verify_kernel<K, MT, false>\);", src)
    assert re.search(r"t\.ua\[K\]\[MT\] = reinterpret_cast<void\*>\(&rs_verify_kernel<K, MT, true>\);", src)
    assert len(all_labels()) == 2 * len(VERIFY_KS) * len(MTS) == 80


# ---------------------------------------------------------------- GPU plumbing
@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    rsmi = pytest.importorskip("rsmi")
    if not torch.cuda.is_available() or rsmi.device_count() == 0:
        pytest.skip("no GPU")
    yield torch, rsmi
    print("\nverify matrix: instantiations run and asserted by label: %d/%d" % (len(SEEN & all_labels()), 80))
    print("verify matrix: wall seconds per leg:", ", ".join("%s %.2f" % kv for kv in sorted(WALL.items())))


class _leg:
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.t0 = time.perf_counter()

    def __exit__(self, *a):
        WALL[self.name] = WALL.get(self.name, 0.0) + time.perf_counter() - self.t0


def _check(torch, c, lay, host, label, want, ctx):
    """want (from the construction) must equal the oracle's answer over the rows as stored; then
    the GPU's flags must equal both.  run_dev pins the label and the buffer byte for byte."""
    assert np.array_equal(want_flags(lay.k, lay.m, lay.rows(host)), want), ("oracle", ctx)
    got = run_dev(torch, c, lay, host, label)
    if not np.array_equal(got, want):
        diff = np.argwhere(got != want)
        raise AssertionError("%r: %d flags differ, first (block, row) = %r: got %r, want %r" %
                             (ctx, len(diff), tuple(diff[0]), got[tuple(diff[0])], want[tuple(diff[0])]))


# ---------------------------------------------------------------- leg 1: all 80 instantiations
CLEAN_S = [16, 17, 1008, 1025, 2085]
SHEET_S = 2085   # 3 tiles; 130 full chunks and a last chunk of 5 bytes
# one byte in each dword of a chunk (acc[j][w] / mk[w]); the tile seams; the last full chunk and
# the first and last byte of the partial chunk
SHEET_POS = [0, 5, 10, 15, 1023, 1024, 2047, 2048, 2079, 2080, 2084]
SMALL_S = 17     # aligned: a second chunk of one byte; split: two windows, only the second has byte 16
SMALL_POS = [0, 16]


def _sheet(rsmi, k, mt, S, positions, aligned, with_data):
    """One call's worth of aimed damage, one block per damage and one untouched block at the end.
    Parity row j alone, one bit flipped, at every position: exactly flag (block, j).  with_data:
    data row 0 and data row k - 1: all mt flags of the block; aligned: byte S (the first padding
    byte) of a data row and of a parity row: no flag."""
    dmg = [("parity", j, p) for j in range(mt) for p in positions]
    if with_data:
        dmg += [("data", 0, positions[len(positions) // 2]), ("data", k - 1, positions[-1])]
        if aligned:
            dmg += [("pad", k - 1, S), ("pad", k + mt - 1, S)]
    nb = len(dmg) + 1
    lay = Lay(rsmi, k, mt, S, nb, aligned)
    sh = stripes(k, mt, S, nb).copy()
    want = np.zeros((nb, mt), dtype=bool)
    for b, (kind, r, p) in enumerate(dmg):
        if kind == "parity":
            sh[b, k + r, p] ^= 1 << ((p + r) % 8)
            want[b, r] = True
        elif kind == "data":
            sh[b, r, p] ^= 1 << (p % 8)
            want[b, :] = True
    host = lay.fill(sh)
    for b, (kind, r, p) in enumerate(dmg):
        if kind == "pad":
            assert lay.rs > S
            o = lay.off + b * lay.bs + r * lay.rs + p
            assert host[o] == (PAD_DATA if r < k else PAD_PARITY)
            host[o] ^= 0xFF
    assert not want[nb - 1].any() and want.sum() == mt * len(positions) + (2 * mt if with_data else 0)
    return lay, host, want


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
@pytest.mark.parametrize("K", VERIFY_KS)
def test_every_instantiation(gpu, K, aligned):
    """rs_verify_kernel<K, MT> for MT = 1..4 through Codec(K, MT), a plan of one tile: clean
    stripes at five sizes with sentinels in every padding and gap byte, then the damage sheets."""
    torch, rsmi = gpu
    mine = set()
    with _leg("leg1"):
        for MT in MTS:
            assert_mds(rsmi, K, MT)
            label = verify_label(K, MT, aligned)
            with rsmi.Codec(K, MT) as c:
                for S in CLEAN_S:
                    lay = Lay(rsmi, K, MT, S, NB, aligned)
                    host = lay.fill(stripes(K, MT, S))
                    if aligned and lay.rs > S:
                        assert host[lay.off + S] == PAD_DATA and host[lay.off + K * lay.rs + S] == PAD_PARITY
                    assert host[(lay.off + lay.bs - 1) if aligned else 0] == GAP
                    assert lay.label() == label
                    _check(torch, c, lay, host, label, np.zeros((NB, MT), dtype=bool), (K, MT, S, aligned, "clean"))
                lay, host, want = _sheet(rsmi, K, MT, SHEET_S, SHEET_POS, aligned, True)
                _check(torch, c, lay, host, label, want, (K, MT, SHEET_S, aligned, "sheet"))
                lay, host, want = _sheet(rsmi, K, MT, SMALL_S, SMALL_POS, aligned, False)
                _check(torch, c, lay, host, label, want, (K, MT, SMALL_S, aligned, "small sheet"))
            mine.add(label)
    assert mine == {verify_label(K, MT, aligned) for MT in MTS} and len(mine) == 4
    SEEN.update(mine)


# ---------------------------------------------------------------- leg 2: seams between launch tiles
@pytest.mark.gpu
@pytest.mark.parametrize("m", [5, 6, 7, 8, 9])
@pytest.mark.parametrize("K", [3, 10])
def test_launch_tile_seams(gpu, K, m):
    """Codec(K, m) with m in 5..9: plans of two and three tiles of up to four parity rows (with
    K = 3 the full tiles are K < MT).  Block j has parity row j alone damaged, for every j: exactly
    flag (j, j), so a tile that reports into another tile's rows shows.  The label is the last
    tile's."""
    torch, rsmi = gpu
    S = 1040
    last_mt = m - 4 * ((m - 1) // 4)
    assert 1 <= last_mt <= 4 and (m - last_mt) % 4 == 0
    with _leg("leg2"), rsmi.Codec(K, m) as c:
        for aligned in (True, False):
            label = verify_label(K, last_mt, aligned)
            lay = Lay(rsmi, K, m, S, m, aligned)
            full = stripes(K, m, S, m)
            _check(torch, c, lay, lay.fill(full), label, np.zeros((m, m), dtype=bool), (K, m, aligned, "clean"))
            sh = full.copy()
            for j in range(m):
                sh[j, K + j, (1039, 1024, 0, 1023)[j % 4] if j < 4 else (j * 131 + 7) % S] ^= 1 << (j % 8)
            _check(torch, c, lay, lay.fill(sh), label, np.eye(m, dtype=bool), (K, m, aligned, "diagonal"))
            SEEN.add(label)


# ---------------------------------------------------------------- leg 3: offsets past 2^32
def _far_case(torch, rsmi, c, d, off, rs, bs, S, nb, aligned, seed):
    """RS(4,2) rows written one by one into an allocation that is otherwise not filled.  First
    call: block 0 carries damage in parity row 0 and the last block (the same block when nb = 1)
    in parity row 1; second call: every block clean."""
    k, m = 4, 2
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 256, size=(nb, k, S), dtype=np.uint8)
    full = np.concatenate([data, np.stack([orc.encode(k, m, data[b]) for b in range(nb)])], axis=1)

    def row(b, i):
        o = off + b * bs + i * rs
        return d[o:o + S]

    def put(sh):
        for b in range(nb):
            for i in range(k + m):
                row(b, i).copy_(torch.from_numpy(sh[b, i]))

    def call(want):
        bad = torch.full((nb * m,), 0x5EED, dtype=torch.int32, device="cuda")
        base = d.data_ptr() + off
        c.verify_batch_dev(base, rs, bs, base + k * rs, rs, bs, S, nb, bad.data_ptr(),
                           torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert c.last_kernel() == verify_label(k, m, aligned), c.last_kernel()
        got = bad.cpu().numpy().reshape(nb, m) != 0
        assert np.array_equal(got, want), (off, rs, bs, nb, got, want)

    sh = full.copy()
    sh[0, k + 0, 1033] ^= 0x10
    sh[nb - 1, k + 1, 3] ^= 0x02
    want = np.zeros((nb, m), dtype=bool)
    want[0, 0] = want[nb - 1, 1] = True
    assert np.array_equal(want_flags(k, m, sh), want)
    put(sh)
    call(want)
    for b in range(nb):  # verify wrote nothing
        for i in range(k + m):
            assert np.array_equal(row(b, i).cpu().numpy(), sh[b, i]), (b, i)
    assert not want_flags(k, m, full).any()
    put(full)
    call(np.zeros((nb, m), dtype=bool))


@pytest.mark.gpu
def test_offsets_past_4gib(gpu):
    """Two blocks at block_stride = 2^32 + 256, and one block with rows at shard_stride = 2^30 + 16
    (row 4 and the parity rows past 2^32), aligned and shifted by one byte (the UA kernel).  An
    offset truncated to 32 bits lands inside the allocation: it reads the other block or bytes no
    row was written to, and changes one of the two answers."""
    torch, rsmi = gpu
    if torch.cuda.mem_get_info()[0] < 8 << 30:
        pytest.skip("needs 8 GiB of free device memory")
    S = 1040
    with _leg("leg3"):
        try:
            with rsmi.Codec(4, 2) as c:
                d = torch.empty(2 ** 32 + 2 ** 20, dtype=torch.uint8, device="cuda")
                bs = 2 ** 32 + 256
                assert 1 + bs + 6 * S <= d.numel()
                _far_case(torch, rsmi, c, d, 0, S, bs, S, 2, True, 3001)
                _far_case(torch, rsmi, c, d, 1, S, bs, S, 2, False, 3002)
                del d
                torch.cuda.empty_cache()
                rs = 2 ** 30 + 16
                d = torch.empty(5 * rs + S + 64, dtype=torch.uint8, device="cuda")
                assert 4 * rs >= 2 ** 32 and 1 + 5 * rs + S <= d.numel()
                _far_case(torch, rsmi, c, d, 0, rs, 6 * rs, S, 1, True, 3003)
                _far_case(torch, rsmi, c, d, 1, rs, 6 * rs, S, 1, False, 3004)
                del d
        finally:
            torch.cuda.empty_cache()


# ---------------------------------------------------------------- leg 4: the fallback
def _stored_vs(full, sh, k):
    """The flags of shards sh whose data rows are those of full (the oracle's clean stripes):
    the oracle's parity against the stored parity, without encoding the same rows again."""
    assert np.array_equal(sh[:, :k], full[:, :k])
    return (sh[:, k:] != full[:, k:]).any(axis=2)


@pytest.mark.gpu
def test_fallback_long_row(gpu):
    """(a) RS(7,1), one block, contiguous rows of 4 * 256 * 4096 + 5 bytes: longer than the capped
    x grid of rs_compare_rows_kernel covers in one pass, with a partial last group.  Byte S - 1 is
    reached only by the second pass of the x loop."""
    torch, rsmi = gpu
    k, m, S = 7, 1, 4 * 256 * 4096 + 5
    assert (S + 3) // 4 > 4096 * 256 and S % 4 == 1
    with _leg("leg4a"), rsmi.Codec(k, m) as c:
        lay = Lay(rsmi, k, m, S, 1, False)
        assert lay.rs == S
        full = stripes(k, m, S, 1)
        for pos in (None, 0, S - 1):
            sh = full.copy()
            want = np.zeros((1, m), dtype=bool)
            if pos is not None:
                sh[0, k, pos] ^= 0x08
                want[0, 0] = True
            assert np.array_equal(_stored_vs(full, sh, k), want)
            got = run_dev(torch, c, lay, lay.fill(sh), COMPARE)
            assert np.array_equal(got, want), (pos, got)


SEAM_HIT = [0, 65534, 65535, 65536, 2 ** 20 - 1, 2 ** 20, 2 ** 20 + 1, 2 ** 20 + 2]
_SEAM = []


def seam_stripes(rsmi):
    """The layout of (b), shared with test_locate_matrix.py: (lay, full, fill).  RS(1,4), S = 15,
    2^20 + 3 blocks of clean stripes from the SIMD oracle (spot-checked against the scalar one),
    computed once and never written; fill(sh) is the byte buffer of lay that holds sh."""
    k, m, S = 1, 4, 15
    nb = 2 ** 20 + 3
    assert m * ((S + 15) // 16 * 16) == 64 and (64 << 20) // 64 == 2 ** 20 < nb and SEAM_HIT[-1] == nb - 1
    lay = Lay(rsmi, k, m, S, nb, False)
    assert lay.rs == S and lay.bs == (k + m) * S and lay.off % 2 == 1
    if not _SEAM:
        rng = np.random.default_rng(4002)
        data = rng.integers(0, 256, size=(nb, k, S), dtype=np.uint8)
        par = orc.encode_fast(k, m, data)
        for b in SEAM_HIT + [1, 77777, 2 ** 20 + 2]:  # the SIMD oracle against the scalar one
            assert np.array_equal(orc.encode(k, m, data[b]), par[b]), b
        full = np.concatenate([data, par], axis=1)
        full.setflags(write=False)
        _SEAM.append(full)

    def fill(sh):  # Lay.fill without its per-row loop: this layout has no padding and no gaps
        host = np.full(lay.size, GAP, dtype=np.uint8)
        host[lay.off:lay.off + nb * lay.bs] = sh.reshape(-1)
        assert np.array_equal(lay.rows(host)[nb - 1], sh[nb - 1])
        return host

    return lay, _SEAM[0], fill


@pytest.mark.gpu
def test_fallback_chunk_seam_and_y_loop(gpu):
    """(b) RS(1,4), S = 15, rows back to back at pitch 15 from an odd base, 2^20 + 3 blocks:
    unaligned rows shorter than 16 bytes; m * round_up(S, 16) = 64, so a 64 MiB scratch chunk is
    exactly 2^20 blocks and the second chunk starts at block 2^20; each chunk's compare grid is
    capped at y = 65535, so its y loop strides 16 times.  One damaged parity byte on each side of
    the y grid's first wrap, of the chunk seam, and at both ends."""
    torch, rsmi = gpu
    k, m, S = 1, 4, 15
    nb = 2 ** 20 + 3
    with _leg("leg4b"):
        lay, full, fill = seam_stripes(rsmi)
        hit = SEAM_HIT
        sh = full.copy()
        want = np.zeros((nb, m), dtype=bool)
        for i, b in enumerate(hit):
            sh[b, k + i % m, (i * 7) % S] ^= 1 << (i % 8)
            want[b, i % m] = True
        assert np.array_equal(_stored_vs(full, sh, k), want)
        with rsmi.Codec(k, m) as c:
            got = run_dev(torch, c, lay, fill(sh), COMPARE)
            assert np.array_equal(np.argwhere(got), np.argwhere(want)), (np.argwhere(got)[:16], np.argwhere(want))
            assert np.array_equal(got, want)
            assert not run_dev(torch, c, lay, fill(full), COMPARE).any()


@pytest.mark.gpu
def test_fallback_scratch_regrow(gpu):
    """(c) One context, one stream: a fallback call of 3 blocks of RS(7,2) at S = 1025, one of 40
    blocks at S = 65541 (the scratch is freed and reallocated behind the first call), then the
    first again in the larger scratch at its own, smaller row pitch."""
    torch, rsmi = gpu
    k, m = 7, 2
    with _leg("leg4c"), rsmi.Codec(k, m) as c:
        for S, nb, (b, j, pos) in ((1025, 3, (1, 1, 1024)), (65541, 40, (38, 0, 65540)), (1025, 3, (2, 0, 0))):
            lay = Lay(rsmi, k, m, S, nb, True)
            full = stripes(k, m, S, nb)
            sh = full.copy()
            sh[b, k + j, pos] ^= 0x20
            want = np.zeros((nb, m), dtype=bool)
            want[b, j] = True
            assert np.array_equal(_stored_vs(full, sh, k), want)
            got = run_dev(torch, c, lay, lay.fill(sh), COMPARE)
            assert np.array_equal(got, want), (S, nb, np.argwhere(got))
