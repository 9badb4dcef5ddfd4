"""Every instantiated rs_mixed_kernel, reached by its label and compared with the oracle.

rs_mixed_kernels.hip builds rs_mixed_kernel<K, MT, UA> for K in {1..6, 8, 10, 12, 16} and MT in
1..4, aligned and unaligned-window: 80 kernels, the verify family's count.  The CPU leg pins that
grid to the source.  Each GPU case is one call of three blocks that lose MT rows each, three
different patterns, so the plan differs between the blocks of one class and is found through the
list, not only picked by the class.  S = 1030 (two tiles a row, the last chunk partial), the data
rows hold every byte value, the whole buffer is compared."""
import itertools
import os
import re

import numpy as np
import pytest

import oracle_lib as orc
from test_mixed_reconstruct import check, layout, mixed_label, present_of, stored
from test_verify_matrix import VERIFY_KS

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "filedag-storage_amd", "csrc")
MIXED_KS = [1, 2, 3, 4, 5, 6, 8, 10, 12, 16]   # fill_mixed_k<K>: fn and ua for MT = 1..4
MIXED_MTS = [1, 2, 3, 4]                        # fill_mixed_km<K, MT> inside fill_mixed_k
S = 1030


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    rsmi = pytest.importorskip("rsmi")
    if not torch.cuda.is_available() or rsmi.device_count() == 0:
        pytest.skip("no GPU")
    return torch, rsmi


def test_kernel_table_matches_source():
    """MIXED_KS x MIXED_MTS is what rs_mixed_kernels.hip fills, both layouts per entry, and the K
    are the verify kernels': 80 kernels."""
    with open(os.path.join(CSRC, "rs_mixed_kernels.hip")) as f:
        src = f.read()
    assert [int(x) for x in re.findall(r"\bfill_mixed_k<\s*(\d+)\s*>\s*\(", src)] == MIXED_KS == VERIFY_KS
    assert re.findall(r"\bfill_mixed_km<K,\s*(\d+)>\(", src) == [str(mt) for mt in MIXED_MTS]
    body = src[src.index("static void fill_mixed_km("):src.index("static void fill_mixed_k(")]
    assert re.findall(r"t\.(fn|ua)\[K\]\[MT\] = reinterpret_cast<void\*>\(&rs_mixed_kernel<K, MT, (false|true)>\);",
                      body) == [("fn", "false"), ("ua", "true")]
    assert 2 * len(MIXED_KS) * len(MIXED_MTS) == 80
    # the kernel has no workgroup barrier: its waves stage their own tables
    kernel = src[src.index("__global__"):src.index("static void fill_mixed_km(")]
    assert "__syncthreads" not in kernel and "s_barrier" not in kernel


def ramp_stripes(k, m, nb):
    """(nb, k + m, S): every data row holds every byte value, no two rows alike."""
    x = np.arange(S, dtype=np.int64)
    data = np.stack([np.stack([(x * (2 * (c % 3) + 1) + 37 * c + 11 * b) & 0xFF for c in range(k)])
                     for b in range(nb)]).astype(np.uint8)
    for b in range(nb):
        for c in range(k):
            assert np.unique(data[b, c]).size == 256
    par = np.stack([orc.encode(k, m, data[b]) for b in range(nb)])
    return np.concatenate([data, par], axis=1)


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "ua"])
@pytest.mark.parametrize("K", MIXED_KS)
def test_every_mixed_kernel(gpu, K, aligned):
    torch, rsmi = gpu
    m = 4
    n = K + m
    full = ramp_stripes(K, m, 3)
    with rsmi.Codec(K, m) as c:
        for MT in MIXED_MTS:
            combos = list(itertools.combinations(range(n), MT))
            losses = [combos[0], combos[len(combos) // 2], combos[-1]]
            assert len(set(losses)) == 3
            present = present_of(n, losses)
            lay = layout(rsmi, K, m, S, 3, aligned)
            check(torch, c, lay, stored(full, present), present, None, False, mixed_label(K, MT, aligned))
