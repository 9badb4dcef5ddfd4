"""Every instantiated rs_ragged_kernel, reached by its label and compared with the oracle.

rs_ragged_kernels.hip builds rs_ragged_kernel<K, MT, UA> for K in {1..6, 8, 10, 12, 16} and MT in
1..4, aligned and unaligned-window: 80 kernels, the mixed family's count.  The CPU leg pins that
grid to the source.  Each GPU case is RS(K, MT) (one plan tile of MT rows) with an all-aligned call
and an all-UA call over blocks of 17 * 16 and 1 025 bytes among others: 1 025 bytes give two tiles
with the last one a single chunk of one byte, 2 049 three tiles with the last one partial; the whole
buffers are compared."""
import os
import re

import pytest

from test_mixed_matrix import MIXED_KS
from test_ragged_encode import ALIGNED, UA, ragged_label, run_dev, seam_batch

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "filedag-storage_amd", "csrc")
RAGGED_KS = [1, 2, 3, 4, 5, 6, 8, 10, 12, 16]   # fill_ragged_k<K>: fn and ua for MT = 1..4
RAGGED_MTS = [1, 2, 3, 4]                        # fill_ragged_km<K, MT> inside fill_ragged_k
SIZES = [17 * 16, 1025, 2049]


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    rsmi = pytest.importorskip("rsmi")
    if not torch.cuda.is_available() or rsmi.device_count() == 0:
        pytest.skip("no GPU")
    return torch, rsmi


def test_kernel_table_matches_source():
    """RAGGED_KS x RAGGED_MTS is what rs_ragged_kernels.hip fills, both layouts per entry, the K are
    the mixed kernels' and the host's ragged_shape: 80 kernels."""
    with open(os.path.join(CSRC, "rs_ragged_kernels.hip")) as f:
        src = f.read()
    assert [int(x) for x in re.findall(r"\bfill_ragged_k<\s*(\d+)\s*>\s*\(", src)] == RAGGED_KS == MIXED_KS
    assert re.findall(r"\bfill_ragged_km<K,\s*(\d+)>\(", src) == [str(mt) for mt in RAGGED_MTS]
    body = src[src.index("static void fill_ragged_km("):src.index("static void fill_ragged_k(")]
    assert re.findall(r"t\.(fn|ua)\[K\]\[MT\] = reinterpret_cast<void\*>\(&rs_ragged_kernel<K, MT, (false|true)>\);",
                      body) == [("fn", "false"), ("ua", "true")]
    assert 2 * len(RAGGED_KS) * len(RAGGED_MTS) == 80
    # the host classes by ragged_shape, which names the same K
    with open(os.path.join(CSRC, "rs_plan.hpp")) as f:
        plan = f.read()
    m = re.search(r"constexpr bool ragged_shape\(int K\) \{ return K >= 1 && \(K <= 6((?: \|\| K == \d+)*)\); \}", plan)
    assert m and [1, 2, 3, 4, 5, 6] + [int(x) for x in re.findall(r"\d+", m.group(1))] == RAGGED_KS
    # the tables are staged once per workgroup: one barrier, ahead of the unit loop
    kernel = src[src.index("__global__"):src.index("static void fill_ragged_km(")]
    assert kernel.count("__syncthreads()") == 1 and kernel.index("__syncthreads()") < kernel.index("for (uint32_t u =")
    with open(os.path.join(os.path.dirname(CSRC), "Makefile")) as f:
        mk = f.read()
    assert "csrc/rs_ragged_kernels.hip" in mk and "csrc/rsmi_ragged.cpp" in mk


@pytest.mark.gpu
@pytest.mark.parametrize("ua", [False, True], ids=["aligned", "ua"])
@pytest.mark.parametrize("K", RAGGED_KS)
def test_every_ragged_kernel(gpu, K, ua):
    torch, rsmi = gpu
    for MT in RAGGED_MTS:
        with rsmi.Codec(K, MT) as c:
            b = seam_batch(K, MT, "ua" if ua else "aligned", SIZES)
            run_dev(torch, c, b, (K, MT, ua), label=ragged_label(K, MT, ua), classes={UA if ua else ALIGNED})
