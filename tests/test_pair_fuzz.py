"""rsmi_locate_pair under seeded random damage, against the definition computed with the CPU oracle.

Each of 24 seeds draws a shape, a row size, a layout and, per block, 0 to 3 damaged shards with
random extents.  The number of damaged shards per block is not drawn but dealt: of 12 blocks two
are clean, two carry one damaged shard, seven carry two and one carries three, in a seeded order.
With m >= 4 the distance names every two-shard block, so 7 of the 10 dirty blocks (at least half)
carry a pair verdict by the definition alone, which the test asserts for every such seed."""
import numpy as np
import pytest

from test_locate_pair import CLEAN, ROWS, check, pair_label, want_pairs
from test_verify import Lay, stripes

SHAPES = [(10, 4), (16, 4), (8, 4), (12, 4), (6, 3), (5, 3), (4, 4), (3, 3), (4, 2), (20, 4), (7, 3), (2, 4)]
FALLBACK = {(20, 4), (7, 3)}
SIZES = [16, 48, 1023, 1041, 2049, 4099]
DEAL = [0, 0, 1, 1, 2, 2, 2, 2, 2, 2, 2, 3]


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    rsmi = pytest.importorskip("rsmi")
    if not torch.cuda.is_available() or rsmi.device_count() == 0:
        pytest.skip("no GPU")
    return torch, rsmi


def draw(seed):
    rng = np.random.default_rng(0xFA12 + seed)
    k, m = SHAPES[seed % len(SHAPES)]
    S = SIZES[int(rng.integers(len(SIZES)))]
    aligned = bool(seed // len(SHAPES) % 2) ^ bool(seed % 2)
    deal = rng.permutation(DEAL)
    sh = stripes(k, m, S, len(deal)).copy()
    for b, nd in enumerate(deal):
        for x in rng.choice(k + m, size=int(nd), replace=False):
            lo = int(rng.integers(S))
            ext = int(min(S - lo, rng.choice([1, 1, 2, 17, 1100, S])))
            sh[b, x, lo:lo + ext] ^= rng.integers(1, 256, size=ext, dtype=np.uint8)
    return k, m, S, aligned, deal, sh


def pair_share(k, m, deal, want):
    """The definition's verdicts against the deal: the share of dirty blocks with a pair verdict."""
    dirty = want[:, 0] != CLEAN
    assert np.array_equal(dirty, deal > 0)
    assert (want[deal == 1, 1] == CLEAN).all() or m < 2
    pairs = int((want[:, 1] >= 0).sum())
    if m >= 4:
        assert (want[deal == 2, 1] >= 0).all(), "the distance names two damaged shards"
        assert 2 * pairs >= int(dirty.sum())
    return pairs, int(dirty.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(24))
def test_fuzz(gpu, seed):
    torch, rsmi = gpu
    k, m, S, aligned, deal, sh = draw(seed)
    want = want_pairs(k, m, sh)
    pair_share(k, m, deal, want)
    lay = Lay(rsmi, k, m, S, sh.shape[0], aligned)
    lab = ROWS if (k, m) in FALLBACK else pair_label(lay)
    with rsmi.Codec(k, m) as c:
        check(torch, c, lay, sh, lab, want)
