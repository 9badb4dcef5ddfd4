"""Every instantiated locate kernel, and the fallback's loops, against the definition, exactly.

rs_locate_kernels.hip builds rs_locate_kernel<K, MT, UA> for K in LOCATE_KS x MT in 2..4 x both
layouts: 60 kernels, each its own unrolled code with the ring geometry of the verify kernel of its
shape and a locate_tile whose j loops are unrolled per MT and whose ratio tables are indexed by the
MT-dependent dword of a plan table.  This module runs every one of them on clean stripes and on a
sheet of aimed damage, proves by the launch label that the instantiation was reached, and then
runs what test_locate.py leaves out of launch_locate: independent data and parity layouts, the
x loop and the y loop of rs_locate_rows_kernel, the 64 MiB scratch chunk seam with locate's own
offsets, the scratch regrow and the eviction of the per-stream scratch.

Every expected verdict is stated twice: from where the damage was put, and from the definition
computed with the CPU oracle (test_locate.want_verdict: replace shard x by its reconstruction,
re-encode, compare).  The two must agree before the GPU's answer is looked at.  The one exception
is two damaged shards under m = 2, where the distance promises nothing: there the definition alone
decides.  Everything is bit-exact: there are no tolerances.

  0  LOCATE_KS x LOCATE_MTS equals the dispatch table of the source (CPU)
  1  all 60 instantiations, clean and damaged; m = 1 for every K
  2  data and parity at independent pitches and block strides, parity at an odd address
  3  rs_locate_rows_kernel's x loop
  4  the scratch chunk seam and the y loop of the locate fallback; no flags pointer
  5  the scratch regrow
  6  more streams than scratch entries
"""
import ctypes
import itertools
import os
import re
import time

import numpy as np
import pytest

from test_locate import CLEAN, ROWS, UNKNOWN, check, label, run_dev, want_verdict, want_verdicts
from test_stream_order import _hip_runtime
from test_verify import GAP, NB, PAD_DATA, PAD_PARITY, Lay, assert_mds, stripes, want_flags
from test_verify_matrix import CLEAN_S, SEAM_HIT, SHEET_POS, SHEET_S, VERIFY_KS, seam_stripes, verify_label

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "filedag-storage_amd", "csrc")

# ---------------------------------------------------------------- the dispatch table, restated
LOCATE_KS = [1, 2, 3, 4, 5, 6, 8, 10, 12, 16]   # fill_locate_k<K>: fn and ua for MT = 2..4
LOCATE_MTS = [2, 3, 4]                          # fill_locate_km<K, MT> inside fill_locate_k
KEPT_STREAMS = 32                               # stream_scratch() evicts at map.size() >= 32


def locate_label(K, MT, aligned):
    return "rs_locate_kernel<K=%d,MT=%d>%s" % (K, MT, "" if aligned else ",UA")


def all_labels():
    return {locate_label(K, MT, a) for K in LOCATE_KS for MT in LOCATE_MTS for a in (True, False)}


# every instantiation a test of this module ran and asserted by its exact label
SEEN = set()
WALL = {}


# ---------------------------------------------------------------- leg 0: the table matches the source
def test_table_matches_source():
    """LOCATE_KS equals the arguments of fill_locate_k in rs_locate_kernels.hip and those of
    fill_verify_k in rs_verify_kernels.hip (the source says they are the same K), and
    fill_locate_km expands to MT = 2..4: a locate kernel added without extending this sweep fails
    the CPU suite.  stream_scratch() keeps 32 streams, which leg 6 relies on."""
    with open(os.path.join(CSRC, "rs_locate_kernels.hip")) as f:
        src = f.read()
    with open(os.path.join(CSRC, "rs_verify_kernels.hip")) as f:
        verify = f.read()
    with open(os.path.join(CSRC, "rsmi_verify.cpp")) as f:
        host = f.read()
    assert [int(x) for x in re.findall(r"\bfill_locate_k<\s*(\d+)\s*>\s*\(", src)] == LOCATE_KS
    assert re.findall(r"\bfill_locate_km<K,\s*(\d+)>\(", src) == [str(m) for m in LOCATE_MTS] == ["2", "3", "4"]
    assert [int(x) for x in re.findall(r"\bfill_verify_k<\s*(\d+)\s*>\s*\(", verify)] == LOCATE_KS == VERIFY_KS
    # one fn and one ua entry per (K, MT), nothing else fills the table
    assert len(re.findall(r"&rs_locate_kernel<", src)) == 2
    assert re.search(r"t\.fn\[K\]\[MT\] = reinterpret_cast<void\*>\(&rs_locate_kernel<K, MT, false>\);", src)
    assert re.search(r"t\.ua\[K\]\[MT\] = reinterpret_cast<void\*>\(&rs_locate_kernel<K, MT, true>\);", src)
    assert len(all_labels()) == 2 * len(LOCATE_KS) * len(LOCATE_MTS) == 60
    body = host[host.index("VerifyScratch& stream_scratch("):host.index("int launch_stripe_tiles(")]
    assert re.findall(r"map\.size\(\)\s*>=\s*(\d+)", body) == [str(KEPT_STREAMS)]
    assert "hipDeviceSynchronize" in body and "map.clear()" in body
    assert N_STREAMS > KEPT_STREAMS + 1


# ---------------------------------------------------------------- GPU plumbing
@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    rsmi = pytest.importorskip("rsmi")
    if not torch.cuda.is_available() or rsmi.device_count() == 0:
        pytest.skip("no GPU")
    assert (rsmi.LocateClean, rsmi.LocateUnknown) == (CLEAN, UNKNOWN)
    yield torch, rsmi
    print("\nlocate matrix: instantiations run and asserted by label: %d/%d" % (len(SEEN & all_labels()), 60))
    print("locate matrix: wall seconds per leg:", ", ".join("%s %.2f" % kv for kv in sorted(WALL.items())))


class _leg:
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.t0 = time.perf_counter()

    def __exit__(self, *a):
        WALL[self.name] = WALL.get(self.name, 0.0) + time.perf_counter() - self.t0


def _agree(want, defn, ctx, free=()):
    """The verdicts from the construction equal the definition's, except at the blocks in free,
    where the construction promises nothing and the definition alone decides."""
    want = np.array(want, dtype=np.int32)
    for b in free:
        want[b] = defn[b]
    assert np.array_equal(want, defn), (ctx, want.tolist(), defn.tolist())
    return want


# ---------------------------------------------------------------- leg 1: all 60 instantiations
SMALL_SIZES = [17, 16]   # 17: aligned, a second chunk of one byte; split, two overlapping windows
DP_POS = [1023, 1024, 2084, 5]                               # data shard + parity row j*, per j*
DP_ERR, PP_ERR = (0x5A, 0x21), (0x11, 0x80)                  # the error bytes of the two-shard cases
_SHEETS = {}   # (K, MT, tag) -> (shards, want, flags): the definition, shared by aligned and split


def _sheet(K, MT):
    """The damage sheet of RS(K, MT) at S = SHEET_S, one block per damage and one untouched block
    at the end: (shards, verdicts, flags, pad), the verdicts stated from the construction and
    agreed with the definition.  pad = (block, data row, parity row): the block whose padding the
    aligned run damages as well, and the rows whose padding it is."""
    n, S = K + MT, SHEET_S
    pairs = list(itertools.combinations(range(MT), 2))
    nb = 2 * n + MT + len(pairs) + 2
    x_pad = 0 if K >= 2 else n - 1
    pad = (nb - 2, K - 1, K)
    assert x_pad not in pad[1:]
    if (K, MT, "sheet") not in _SHEETS:
        rng = np.random.default_rng(7000 + 31 * K + MT)
        sh = stripes(K, MT, S, nb).copy()
        want, free = [], []
        for x in range(n):            # a stale shard: every error value in every byte column
            err = rng.integers(1, 256, size=S, dtype=np.uint8)
            err[rng.permutation(S)[:255]] = np.arange(1, 256, dtype=np.uint8)
            assert len(np.unique(err)) == 255 and err.min() == 1
            sh[len(want), x] ^= err
            want.append(x)
        for x in range(n):            # a single bit
            p = SHEET_POS[x % len(SHEET_POS)]
            sh[len(want), x, p] ^= 1 << ((p + x) % 8)
            want.append(x)
        for js in range(MT):          # a data shard and parity row j* in one byte column
            b, c, p = len(want), (K - 1 - js) % K, DP_POS[js]
            sh[b, c, p] ^= DP_ERR[0]
            sh[b, K + js, p] ^= DP_ERR[1]
            if MT == 2:
                free.append(b)
            want.append(UNKNOWN)
        for i, j in pairs:            # two parity rows in one byte column
            b, p = len(want), SHEET_POS[(4 * i + j) % len(SHEET_POS)]
            sh[b, K + i, p] ^= PP_ERR[0]
            sh[b, K + j, p] ^= PP_ERR[1]
            if MT == 2:
                free.append(b)
            want.append(UNKNOWN)
        assert len(want) == pad[0]    # the block whose padding is damaged too
        sh[pad[0], x_pad, 2079] ^= 0x04
        want += [x_pad, CLEAN]
        assert len(want) == nb
        defn = want_verdicts(K, MT, sh)
        assert defn[:2 * n].tolist() == 2 * list(range(n)), (K, MT, defn)
        sh.setflags(write=False)
        _SHEETS[K, MT, "sheet"] = (sh, _agree(want, defn, (K, MT, "sheet"), free), want_flags(K, MT, sh))
    return _SHEETS[K, MT, "sheet"] + (pad,)


def _small_sheet(K, MT, S):
    """Every shard as the culprit at byte 0 and at byte S - 1, and a clean block."""
    n = K + MT
    if (K, MT, S) not in _SHEETS:
        sh = stripes(K, MT, S, 2 * n + 1).copy()
        want = []
        for x in range(n):
            sh[2 * x, x, 0] ^= 1 << (x % 8)
            sh[2 * x + 1, x, S - 1] ^= 0x80 >> (x % 8)
            want += [x, x]
        want.append(CLEAN)
        sh.setflags(write=False)
        _SHEETS[K, MT, S] = (sh, _agree(want, want_verdicts(K, MT, sh), (K, MT, S)), want_flags(K, MT, sh))
    return _SHEETS[K, MT, S]


def _m1_sheet(K, S):
    """m = 1: a damaged data row, a damaged parity row and a clean block.  Every shard explains
    any damage, so dirty is -2."""
    if (K, 1, S) not in _SHEETS:
        sh = stripes(K, 1, S, NB).copy()
        sh[0, K - 1, S - 1] ^= 0x01
        sh[1, K, 1024] ^= 0x80
        sh.setflags(write=False)
        want = _agree([UNKNOWN, UNKNOWN, CLEAN], want_verdicts(K, 1, sh), (K, 1, S))
        _SHEETS[K, 1, S] = (sh, want, want_flags(K, 1, sh))
    return _SHEETS[K, 1, S]


def _run_sheet(torch, c, lay, host, lab, want, flags, ctx):
    got, bad = run_dev(torch, c, lay, host, lab)
    if not np.array_equal(got, want):
        b = int(np.flatnonzero(got != want)[0])
        raise AssertionError("%r: %d verdicts differ, first at block %d: got %d, want %d" %
                             (ctx, (got != want).sum(), b, got[b], want[b]))
    assert np.array_equal(bad, flags), (ctx, np.argwhere(bad != flags)[:8])


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
@pytest.mark.parametrize("K", LOCATE_KS)
def test_every_instantiation(gpu, K, aligned):
    """rs_locate_kernel<K, MT> for MT = 2..4 through Codec(K, MT): clean stripes at five sizes with
    sentinels in every padding and gap byte, then the damage sheets.  On the sheet every shard is
    the culprit as a stale row (all 255 error values through every column's ratio product for
    every j, and the AND across three tiles) and as a single bit; a data shard together with each
    parity row j* (j* >= 1 disturbs exactly the one row a lax data test could skip) and every pair
    of parity rows (a parity test that skipped row i would name j) are -2 for MT >= 3 by the
    distance and the definition's for MT = 2; damage in the padding beside real damage leaves the
    verdict alone.  Then rs_verify_kernel<K, MT=1> as locate's launch for m = 1."""
    torch, rsmi = gpu
    mine = set()
    with _leg("leg1"):
        for MT in LOCATE_MTS:
            assert_mds(rsmi, K, MT)
            lab = locate_label(K, MT, aligned)
            n = K + MT
            with rsmi.Codec(K, MT) as c:
                for S in CLEAN_S:
                    lay = Lay(rsmi, K, MT, S, NB, aligned)
                    assert label(lay) == lab
                    full = stripes(K, MT, S)
                    host = lay.fill(full)
                    if aligned and lay.rs > S:
                        assert host[lay.off + S] == PAD_DATA and host[lay.off + K * lay.rs + S] == PAD_PARITY
                    assert host[(lay.off + lay.bs - 1) if aligned else 0] == GAP
                    assert not want_flags(K, MT, full).any()
                    got = check(torch, c, lay, full, lab)   # the definition and the oracle's flags
                    assert (got == CLEAN).all(), (K, MT, S, aligned, got)
                # the sheet
                sh, want, flags, (pb, pd, pp) = _sheet(K, MT)
                assert want[-1] == CLEAN and (want[:-1] != CLEAN).all() and flags[:-1].any(axis=1).all()
                assert MT == 2 or (want[2 * n:pb] == UNKNOWN).all()
                lay = Lay(rsmi, K, MT, SHEET_S, sh.shape[0], aligned)
                host = lay.fill(sh)
                if aligned:   # byte S, the first padding byte, of another data row and of a parity row
                    assert lay.rs > SHEET_S
                    for r in (pd, pp):
                        o = lay.off + pb * lay.bs + r * lay.rs + SHEET_S
                        assert host[o] == (PAD_DATA if r < K else PAD_PARITY)
                        host[o] ^= 0xFF
                else:         # the byte before the first row and the byte after the last
                    for o in (lay.off - 1, lay.off + lay.nb * lay.bs):
                        assert host[o] == GAP
                        host[o] ^= 0xFF
                assert np.array_equal(lay.rows(host), sh)
                _run_sheet(torch, c, lay, host, lab, want, flags, (K, MT, SHEET_S, aligned, "sheet"))
                # the small sheets
                for S in SMALL_SIZES:
                    sh, want, flags = _small_sheet(K, MT, S)
                    lay = Lay(rsmi, K, MT, S, sh.shape[0], aligned)
                    _run_sheet(torch, c, lay, lay.fill(sh), lab, want, flags, (K, MT, S, aligned, "small sheet"))
            mine.add(lab)
        # m = 1: Verify's kernel, no candidates, the verdict kernel
        with rsmi.Codec(K, 1) as c:
            sh, want, flags = _m1_sheet(K, 1025)
            lay = Lay(rsmi, K, 1, 1025, NB, aligned)
            assert label(lay) == verify_label(K, 1, aligned)
            assert want.tolist() == [UNKNOWN, UNKNOWN, CLEAN]
            _run_sheet(torch, c, lay, lay.fill(sh), verify_label(K, 1, aligned), want, flags, (K, 1, aligned))
    assert mine == {locate_label(K, MT, aligned) for MT in LOCATE_MTS} and len(mine) == 3
    SEEN.update(mine)


# ---------------------------------------------------------------- leg 2: independent layouts
@pytest.mark.gpu
@pytest.mark.parametrize("k,m,lab", [(6, 3, "rs_locate_kernel<K=6,MT=3>,UA"), (7, 2, ROWS)], ids=["fused", "fallback"])
def test_independent_data_and_parity_layouts(gpu, k, m, lab):
    """Data and parity in one allocation at their own pitches and block strides: data rows
    16-byte aligned, parity rows from an odd address at an odd pitch, which must select the UA
    kernel (and, in the fallback, compare scratch rows against stored rows at parity's own
    strides).  A data culprit, a parity culprit, two damaged shards and a clean block; the buffer
    comes back byte for byte, the sentinels between the rows included."""
    torch, rsmi = gpu
    S, nb, n = 1025, 4, k + m
    drs, prs = 1072, S + 9
    dbs, pbs = k * drs + 64, m * prs + 5
    doff = 256
    poff = doff + nb * dbs + 33
    assert drs % 16 == 0 and dbs % 16 == 0 and poff % 2 == 1 and prs % 2 == 0 and pbs % 2 == 1
    with _leg("leg2"):
        sh = stripes(k, m, S, nb).copy()
        sh[0, 2, S - 1] ^= 0x10
        sh[1, n - 1, 0] ^= 0x01
        sh[2, 0, S // 2] ^= 0x33
        sh[2, k, S // 2] ^= 0x44
        free = [2] if m == 2 else []   # m = 2, two damaged shards: the definition alone decides
        want = _agree([2, n - 1, UNKNOWN, CLEAN], want_verdicts(k, m, sh), (k, m), free)
        flags = want_flags(k, m, sh)
        host = np.full(poff + nb * pbs + 64, GAP, dtype=np.uint8)
        for b in range(nb):
            for r in range(k):
                o = doff + b * dbs + r * drs
                host[o:o + drs] = PAD_DATA
                host[o:o + S] = sh[b, r]
            for j in range(m):
                o = poff + b * pbs + j * prs
                host[o:o + prs] = PAD_PARITY
                host[o:o + S] = sh[b, k + j]
        d = torch.from_numpy(host.copy()).cuda()
        assert d.data_ptr() % 256 == 0
        with rsmi.Codec(k, m) as c:
            for with_flags in (True, False):
                cul = torch.full((nb + 2,), 0x5EED, dtype=torch.int32, device="cuda")
                bad = torch.full((nb * m + 2,), 0x5EED, dtype=torch.int32, device="cuda")
                c.locate_batch_dev(d.data_ptr() + doff, drs, dbs, d.data_ptr() + poff, prs, pbs, S, nb, cul.data_ptr(),
                                   bad.data_ptr() if with_flags else 0, torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                assert c.last_kernel() == lab, c.last_kernel()
                assert np.array_equal(d.cpu().numpy(), host), "locate wrote to the shards"
                cul, bad = cul.cpu().numpy(), bad.cpu().numpy()
                assert (cul[nb:] == 0x5EED).all() and (bad[nb * m:] == 0x5EED).all()
                assert np.array_equal(cul[:nb], want), (with_flags, cul[:nb], want)
                if with_flags:
                    assert np.array_equal(bad[:nb * m].reshape(nb, m) != 0, flags)
                else:
                    assert (bad == 0x5EED).all()
    if lab != ROWS:
        SEEN.add(lab)


# ---------------------------------------------------------------- leg 3: the rows kernel's x loop
LONG_S = 256 * 4096 + 5
_LONG = {}


def _long_cases(k, m):
    """(name, shards (1, n, S), verdict) for one block of rows of LONG_S bytes; the definition
    costs about a second per dirty block at this size, so each is computed once."""
    if (k, m) not in _LONG:
        S = LONG_S
        full = stripes(k, m, S, 1)
        cases = []
        for name, dmg, want in (("clean", [], CLEAN), ("data-last", [(4, S - 1)], 4),
                                ("parity", [(k + m - 1, S - 2)], k + m - 1),
                                ("two-passes-disagree", [(2, 100), (5, S - 1)], UNKNOWN),
                                ("two-passes-agree", [(2, 100), (2, S - 1)], 2)):
            sh = full.copy()
            for x, p in dmg:
                sh[0, x, p] ^= 0x08
            # shard 2 in the first pass and shard 5 in the second: two data shards, -2 under the
            # definition for both codes (for m = 2 not by the distance, so asserted as computed)
            assert want_verdict(k, m, sh[0]) == want, (k, m, name)
            cases.append((name, sh, want))
        _LONG[k, m] = cases
    return _LONG[k, m]


@pytest.mark.gpu
@pytest.mark.parametrize("m", [2, 3])
def test_rows_kernel_x_loop(gpu, m):
    """RS(7,m), one block, rows of 256 * 4096 + 5 bytes at pitch S: more byte columns than the
    capped x grid of rs_locate_rows_kernel covers in one pass, so the last 5 bytes are reached only
    by the second pass.  Damage there alone, damage in both passes that names different shards
    (the first pass alone would say 2) and the same shard."""
    torch, rsmi = gpu
    k, S = 7, LONG_S
    assert (S + 255) // 256 > 4096 and S - 256 * 4096 == 5
    with _leg("leg3"), rsmi.Codec(k, m) as c:
        lay = Lay(rsmi, k, m, S, 1, False)
        assert lay.rs == S
        for name, sh, want in _long_cases(k, m):
            got = check(torch, c, lay, sh, ROWS, np.array([want], dtype=np.int32))
            assert got.tolist() == [want], (name, got)


# ---------------------------------------------------------------- leg 4: chunk seam and y loop
@pytest.mark.gpu
def test_fallback_chunk_seam_and_y_loop(gpu):
    """RS(1,4), S = 15, rows back to back from an odd base, 2^20 + 3 blocks (the layout of
    test_verify_matrix.py 4b): launch_locate's scratch chunk is exactly 2^20 blocks, so the second
    chunk's flags, candidates and parity start at bad + 2^20 * m, cand + 2^20 * words and
    parity + 2^20 * parity_bs, and each chunk's rs_locate_rows_kernel grid wraps y 16 times.  One
    damaged byte on each side of the y grid's first wrap, of the chunk seam and at both ends, the
    damaged shard rotating over all five.  Then the same call with no flags pointer: the flags
    live in the stream's scratch behind the candidate words."""
    torch, rsmi = gpu
    k, m, S = 1, 4, 15
    with _leg("leg4"):
        lay, full, fill = seam_stripes(rsmi)
        nb = lay.nb
        sh = full.copy()
        want = np.full(nb, CLEAN, dtype=np.int32)      # clean by construction from encode_fast
        flags = np.zeros((nb, m), dtype=bool)
        for i, b in enumerate(SEAM_HIT):
            x = i % (k + m)
            sh[b, x, (i * 7) % S] ^= 1 << (i % 8)
            want[b] = x
            flags[b] = True if x < k else np.arange(m) == x - k
            assert want_verdict(k, m, sh[b]) == x, (b, x)
            assert np.array_equal(want_flags(k, m, sh[b:b + 1])[0], flags[b]), b
        assert want[SEAM_HIT].tolist() == [0, 1, 2, 3, 4, 0, 1, 2]
        for b in (1, 65533, 2 ** 20 - 2):              # a sample of the rest under the definition
            assert want_verdict(k, m, sh[b]) == CLEAN
        host = fill(sh)
        with rsmi.Codec(k, m) as c:
            got, bad = run_dev(torch, c, lay, host, ROWS)
            assert np.array_equal(np.flatnonzero(got != CLEAN), np.array(SEAM_HIT)), np.flatnonzero(got != CLEAN)[:16]
            assert np.array_equal(got, want), (got[SEAM_HIT], want[SEAM_HIT])
            assert np.array_equal(np.flatnonzero(bad.any(axis=1)), np.array(SEAM_HIT))
            assert np.array_equal(bad, flags)
            got2, none = run_dev(torch, c, lay, host, ROWS, flags=False)
            assert none is None and np.array_equal(got2, got)


# ---------------------------------------------------------------- leg 5: scratch regrow
@pytest.mark.gpu
@pytest.mark.parametrize("k,m,fused", [(5, 3, True), (7, 2, False)], ids=["fused", "fallback"])
def test_scratch_regrow(gpu, k, m, fused):
    """One context, one stream: 3 blocks at S = 1025, 40 blocks at S = 65541 (locate_scratch, and
    for RS(7,2) verify_scratch too, is freed and reallocated behind the first call), then 3 blocks
    again in the larger scratch, with no flags pointer, so the flags lie behind 3 candidate words
    in a scratch that held 40.  One culprit per call, at a different block and position."""
    torch, rsmi = gpu
    with _leg("leg5"), rsmi.Codec(k, m) as c:
        for S, nb, (b, x, pos), with_flags in ((1025, 3, (1, k + 1, 1024), True), (65541, 40, (38, 3, 65540), True),
                                               (1025, 3, (2, 0, 0), False)):
            lay = Lay(rsmi, k, m, S, nb, True)
            sh = stripes(k, m, S, nb).copy()
            sh[b, x, pos] ^= 0x20
            want = np.full(nb, CLEAN, dtype=np.int32)
            want[b] = x
            assert np.array_equal(want_verdicts(k, m, sh), want)
            got, bad = run_dev(torch, c, lay, lay.fill(sh), label(lay) if fused else ROWS, flags=with_flags)
            assert np.array_equal(got, want), (S, nb, got)
            if with_flags:
                assert np.array_equal(bad, want_flags(k, m, sh))
    if fused:
        SEEN.add(locate_label(k, m, True))


# ---------------------------------------------------------------- leg 6: more streams than scratch entries
N_STREAMS = 34


@pytest.mark.gpu
@pytest.mark.parametrize("k,m,fused", [(4, 3, True), (7, 2, False)], ids=["fused", "fallback"])
def test_more_streams_than_scratch_entries(gpu, k, m, fused):
    """One context, locate on 34 distinct streams in turn, each with its own culprit: the 33rd
    stream makes stream_scratch() drain the device, free every stream's scratch and start the map
    again.  Then the first stream once more, whose scratch was freed, and a verify on the same
    context.  The outputs are poisoned on the stream of the call; every verdict is the
    definition's.  35 small calls: the evict-and-reallocate path, not a stress loop."""
    torch, rsmi = gpu
    S, nb, n = 1025, 3, k + m
    hip = _hip_runtime()
    hip.hipStreamCreateWithFlags.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
    hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
    own = []
    with _leg("leg6"):
        try:
            for _ in range(N_STREAMS):
                h = ctypes.c_void_p()
                assert hip.hipStreamCreateWithFlags(ctypes.byref(h), 1) == 0  # hipStreamNonBlocking
                own.append(h)
            streams = [torch.cuda.ExternalStream(h.value) for h in own]
            assert len({s.cuda_stream for s in streams}) == N_STREAMS > KEPT_STREAMS + 1
            lay = Lay(rsmi, k, m, S, nb, True)
            lab = label(lay) if fused else ROWS
            full = stripes(k, m, S, nb)
            wants = {}

            def call(c, i, st):
                x, b = i % n, i % nb
                sh = full.copy()
                sh[b, x, (i * 37) % S] ^= 1 << (i % 8)
                if (x, b) not in wants:
                    wants[x, b] = want_verdicts(k, m, sh)
                    assert wants[x, b][b] == x and (np.delete(wants[x, b], b) == CLEAN).all()
                d = torch.from_numpy(lay.fill(sh)).cuda()
                cul = torch.empty(nb, dtype=torch.int32, device="cuda")
                bad = torch.empty(nb * m, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                with torch.cuda.stream(st):
                    cul.fill_(0x0BAD)
                    bad.fill_(0x0BAD)
                    c.locate_batch_dev(d.data_ptr(), lay.rs, lay.bs, d.data_ptr() + k * lay.rs, lay.rs, lay.bs, S, nb,
                                       cul.data_ptr(), bad.data_ptr() if i % 2 else 0, st.cuda_stream)
                st.synchronize()
                assert c.last_kernel() == lab
                assert np.array_equal(cul.cpu().numpy(), wants[x, b]), (i, cul.cpu().numpy())
                if i % 2:
                    assert np.array_equal(bad.cpu().numpy().reshape(nb, m) != 0, want_flags(k, m, sh)), i
                else:
                    assert (bad.cpu().numpy() == 0x0BAD).all(), i
                return d, sh

            with rsmi.Codec(k, m) as c:
                for i, st in enumerate(streams):
                    call(c, i, st)
                d, sh = call(c, N_STREAMS + 1, streams[0])   # its scratch went with the eviction
                bad = torch.full((nb * m,), 0x5EED, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                c.verify_batch_dev(d.data_ptr(), lay.rs, lay.bs, d.data_ptr() + k * lay.rs, lay.rs, lay.bs, S, nb,
                                   bad.data_ptr(), streams[0].cuda_stream)
                streams[0].synchronize()
                assert np.array_equal(bad.cpu().numpy().reshape(nb, m) != 0, want_flags(k, m, sh))
        finally:
            torch.cuda.synchronize()
            for h in own:
                hip.hipStreamDestroy(h)
    if fused:
        SEEN.add(locate_label(k, m, True))
