"""Every instantiated heal kernel, and the fallback kernel's x loop, against the definition, exactly.

rs_heal_kernels.hip builds rs_heal_kernel<K, MT, UA> for the shapes of rs_locate_kernel: K in
HEAL_KS x MT in 2..4 x both layouts, 60 kernels, each its own unrolled code: the ring geometry of
its shape decides where a parity culprit's chunk is found after the column loop (a ring slot, or,
for K < MT, a register loaded ahead of it), the column loop's unrolled capture decides which data
chunk is kept, and the inverse coefficient is read from the MT-dependent dword of a table column
chosen at run time.  This module runs every one of them on a batch with a data culprit, a parity
culprit, a clean block and a block of two damaged shards, compares the whole buffer with the
definition's image (test_heal.check) and proves by the launch label that the instantiation was
reached.  Then rs_heal_rows_kernel's x loop, on rows longer than its capped grid covers at once.

  0  HEAL_KS x HEAL_MTS equals the dispatch tables of the source (CPU)
  1  all 60 instantiations
  2  rs_heal_rows_kernel's x loop
"""
import os
import re

import numpy as np
import pytest

from test_heal import ROWS, check
from test_locate import CLEAN, UNKNOWN, want_verdicts
from test_locate_matrix import LOCATE_KS, LOCATE_MTS, LONG_S, _long_cases
from test_verify import Lay, stripes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "filedag-storage_amd", "csrc")

HEAL_KS = [1, 2, 3, 4, 5, 6, 8, 10, 12, 16]   # fill_heal_k<K>: fn and ua for MT = 2..4
HEAL_MTS = [2, 3, 4]                          # fill_heal_km<K, MT> inside fill_heal_k
SHEET_S = 1040                                # two tiles, the second of one chunk


def heal_label(K, MT, aligned):
    return "rs_heal_kernel<K=%d,MT=%d>%s" % (K, MT, "" if aligned else ",UA")


def all_labels():
    return {heal_label(K, MT, a) for K in HEAL_KS for MT in HEAL_MTS for a in (True, False)}


SEEN = set()


def test_table_matches_source():
    """HEAL_KS x HEAL_MTS is what rs_heal_kernels.hip fills, and it is the locate kernels' set:
    every verdict rs_locate_kernel can give has an rs_heal_kernel to act on it."""
    with open(os.path.join(CSRC, "rs_heal_kernels.hip")) as f:
        src = f.read()
    assert [int(x) for x in re.findall(r"\bfill_heal_k<\s*(\d+)\s*>\s*\(", src)] == HEAL_KS == LOCATE_KS
    assert re.findall(r"\bfill_heal_km<K,\s*(\d+)>\(", src) == [str(m) for m in HEAL_MTS]
    assert HEAL_MTS == LOCATE_MTS
    assert len(re.findall(r"&rs_heal_kernel<", src)) == 2
    assert re.search(r"t\.fn\[K\]\[MT\] = reinterpret_cast<void\*>\(&rs_heal_kernel<K, MT, false>\);", src)
    assert re.search(r"t\.ua\[K\]\[MT\] = reinterpret_cast<void\*>\(&rs_heal_kernel<K, MT, true>\);", src)
    assert len(all_labels()) == 2 * len(HEAL_KS) * len(HEAL_MTS) == 60


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    rsmi = pytest.importorskip("rsmi")
    if not torch.cuda.is_available() or rsmi.device_count() == 0:
        pytest.skip("no GPU")
    yield torch, rsmi
    print("\nheal matrix: instantiations run and asserted by label: %d/%d" % (len(SEEN & all_labels()), 60))


_SHEETS = {}


def _sheet(K, MT):
    """(shards, verdicts) of RS(K, MT) at SHEET_S: every data shard and every parity shard once
    as the culprit (a burst across the tile seam for the first of each kind, single bytes at the
    chunk edges for the rest), a block of two damaged shards and a clean block.  The verdicts are
    the definition's; for MT >= 3 the distance says what they are, for MT = 2 the definition alone
    decides the two-shard block."""
    if (K, MT) not in _SHEETS:
        n, S = K + MT, SHEET_S
        nb = n + 2
        rng = np.random.default_rng(9000 + 31 * K + MT)
        sh = stripes(K, MT, S, nb).copy()
        for x in range(n):
            if x in (0, K):
                sh[x, x, 1000:1040] ^= rng.integers(1, 256, size=40, dtype=np.uint8)
            else:
                sh[x, x, (0, 15, 16, 1023, 1024, 1039)[x % 6]] ^= 1 << (x % 8)
        sh[n, K - 1, 1030] ^= 0x5A           # a data shard and a parity shard, one byte column
        sh[n, n - 1, 1030] ^= 0x21
        want = want_verdicts(K, MT, sh)
        assert want[:n].tolist() == list(range(n)) and want[n + 1] == CLEAN, (K, MT, want)
        assert MT == 2 or want[n] == UNKNOWN
        sh.setflags(write=False)
        _SHEETS[K, MT] = (sh, want)
    return _SHEETS[K, MT]


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
@pytest.mark.parametrize("K", HEAL_KS)
def test_every_instantiation(gpu, K, aligned):
    torch, rsmi = gpu
    mine = set()
    for MT in HEAL_MTS:
        lab = heal_label(K, MT, aligned)
        sh, want = _sheet(K, MT)
        lay = Lay(rsmi, K, MT, SHEET_S, sh.shape[0], aligned)
        with rsmi.Codec(K, MT) as c:
            _, image = check(torch, c, lay, sh, lab, want)
            n = K + MT
            assert np.array_equal(image[:n], stripes(K, MT, SHEET_S, n + 2)[:n])  # one shard: the original
            # what was healed is clean now, and a second heal finds nothing to write
            again = want_verdicts(K, MT, image)
            assert (again[:n] == CLEAN).all() and again[n + 1] == CLEAN
            check(torch, c, lay, image, lab, again)
        mine.add(lab)
    assert len(mine) == 3
    SEEN.update(mine)


@pytest.mark.gpu
def test_rows_kernel_x_loop(gpu):
    """RS(7,2), one block, rows of 256 * 4096 + 5 bytes at pitch S (test_locate_matrix's long
    cases, whose verdicts are the definition's): more byte columns than the capped x grid of
    rs_heal_rows_kernel covers in one pass, so the last 5 bytes are healed only by the second
    pass.  A data culprit damaged in both passes, one damaged in the second alone, a parity
    culprit, and two shards that disagree across the passes (UNKNOWN: untouched)."""
    torch, rsmi = gpu
    k, m, S = 7, 2, LONG_S
    assert (S + 255) // 256 > 4096 and S - 256 * 4096 == 5
    with rsmi.Codec(k, m) as c:
        lay = Lay(rsmi, k, m, S, 1, False)
        full = stripes(k, m, S, 1)
        for name, sh, want in _long_cases(k, m):
            got, image = check(torch, c, lay, sh, ROWS, np.array([want], dtype=np.int32))
            assert got.tolist() == [want], (name, got)
            assert np.array_equal(image, sh if want == UNKNOWN else full), name
