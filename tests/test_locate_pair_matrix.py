"""Every instantiated rs_locate_pair_kernel, reached by its label: K in {1..6, 8, 10, 12, 16},
MT = m in {3, 4}, aligned and unaligned-window rows, 40 kernels.  Each runs one call that holds a
data-data pair, a data-parity-0 pair, a data-parity-(m-1) pair and the parity-parity pair {k, k+1}
(K = 1 has no data-data pair: a second data-parity pair stands in), a single culprit and a clean
block, against the definition computed with the CPU oracle."""
import numpy as np
import pytest

from test_locate_pair import CLEAN, PAIR_KS, UNKNOWN, check, pair_label, want_pairs
from test_verify import Lay, stripes

SEEN = set()
_SHEETS = {}


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    rsmi = pytest.importorskip("rsmi")
    if not torch.cuda.is_available() or rsmi.device_count() == 0:
        pytest.skip("no GPU")
    yield torch, rsmi
    print("\nlocate pair matrix: instantiations run and asserted by label: %d/40" % len(SEEN))


def sheet(K, MT):
    """(shards, want): S = 1041 (two tiles; split: an overlapping last window), every pair damaged
    in three byte columns spread over both tiles so that m = 3 names it too; the definition must
    confirm each pair on the CPU."""
    if (K, MT) not in _SHEETS:
        S = 1041
        pairs = [(0, K - 1) if K > 1 else (0, K + 1), (K - 1, K), (0, K + MT - 1), (K, K + 1)]
        sh = stripes(K, MT, S, len(pairs) + 2).copy()
        for b, (x, y) in enumerate(pairs):
            for i, (ex, ey) in enumerate(((0x21, 0x9C), (0x47, 0x0B), (0xD3, 0x65))):
                sh[b, x, (b * 37 + 5 + i * 509) % S] ^= ex
                sh[b, y, (b * 37 + 5 + i * 509) % S if i else 1040 - b] ^= ey
        sh[len(pairs), K // 2, 1024] ^= 0x04
        want = want_pairs(K, MT, sh)
        assert want.tolist() == [list(p) for p in pairs] + [[K // 2, CLEAN], [CLEAN, CLEAN]], (K, MT, want.tolist())
        _SHEETS[K, MT] = (sh, want)
    return _SHEETS[K, MT]


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
@pytest.mark.parametrize("MT", [3, 4])
@pytest.mark.parametrize("K", PAIR_KS)
def test_every_instantiation(gpu, K, MT, aligned):
    torch, rsmi = gpu
    sh, want = sheet(K, MT)
    lay = Lay(rsmi, K, MT, 1041, sh.shape[0], aligned)
    lab = pair_label(lay)
    assert lab == "rs_locate_pair_kernel<K=%d,MT=%d>%s" % (K, MT, "" if aligned else ",UA")
    with rsmi.Codec(K, MT) as c:
        got = check(torch, c, lay, sh, lab, want)
    assert (got != UNKNOWN).all()
    SEEN.add(lab)
