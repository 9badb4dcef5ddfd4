"""Every instantiated rs_heal_pair_kernel, reached by its label: K in {1..6, 8, 10, 12, 16},
MT = m in {3, 4}, aligned and unaligned-window rows, 40 kernels.  Each runs one call that holds a
data-data pair, a data-parity-0 pair, a data-parity-(m-1) pair and the parity-parity pair {k, k+1}
(K = 1 has no data-data pair: a second data-parity pair stands in), a single culprit and a clean
block, against the definition computed with the CPU oracle: the verdicts, the flags and the whole
buffer.  S = 1025, the smallest row with two tiles and a partial last chunk."""
import numpy as np
import pytest

from test_heal_pair import check, label, want_image
from test_locate_pair import CLEAN, PAIR_KS, want_pairs
from test_verify import Lay, stripes

SEEN = set()
_SHEETS = {}
S = 1025


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    rsmi = pytest.importorskip("rsmi")
    if not torch.cuda.is_available() or rsmi.device_count() == 0:
        pytest.skip("no GPU")
    yield torch, rsmi
    print("\nheal pair matrix: instantiations run and asserted by label: %d/40" % len(SEEN))


def sheet(K, MT):
    """(shards, want): x damaged alone in a column of tile 0, y alone in byte 1024 (tile 1, the
    partial chunk), so the pair is the only explanation at m = 3 too, and both in one column of
    tile 0, which takes both rows of D.  The definition must confirm each pair on the CPU, and the
    image must be the original."""
    if (K, MT) not in _SHEETS:
        pairs = [(0, K - 1) if K > 1 else (0, K + 1), (K - 1, K), (0, K + MT - 1), (K, K + 1)]
        full = stripes(K, MT, S, len(pairs) + 2)
        sh = full.copy()
        for b, (x, y) in enumerate(pairs):
            sh[b, x, b * 37 + 5] ^= 0x21 + b
            sh[b, y, 1024] ^= 0x9C - b
            sh[b, x, 600 + b] ^= 0x47
            sh[b, y, 600 + b] ^= 0x0B + 16 * b
        sh[len(pairs), K // 2, 1024] ^= 0x04
        want = want_pairs(K, MT, sh)
        assert want.tolist() == [list(p) for p in pairs] + [[K // 2, CLEAN], [CLEAN, CLEAN]], (K, MT, want.tolist())
        assert np.array_equal(want_image(K, MT, sh, want), full)
        _SHEETS[K, MT] = (sh, want)
    return _SHEETS[K, MT]


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
@pytest.mark.parametrize("MT", [3, 4])
@pytest.mark.parametrize("K", PAIR_KS)
def test_every_instantiation(gpu, K, MT, aligned):
    torch, rsmi = gpu
    sh, want = sheet(K, MT)
    lay = Lay(rsmi, K, MT, S, sh.shape[0], aligned)
    lab = label(lay)
    assert lab == "rs_heal_pair_kernel<K=%d,MT=%d>%s" % (K, MT, "" if aligned else ",UA")
    with rsmi.Codec(K, MT) as c:
        check(torch, c, lay, sh, lab, want)
    SEEN.add(lab)
