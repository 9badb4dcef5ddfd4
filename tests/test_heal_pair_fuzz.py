"""rsmi_heal_pair under seeded random damage, against the definition computed with the CPU oracle.

Each of 16 seeds takes a shape of RS(10,4), RS(6,3), RS(16,4), RS(7,3) (the last has no
rs_heal_pair_kernel: the fallback) and a layout in turn, draws a row size and, per block, 0 to 3
damaged shards with random extents.  The number of damaged shards per block is not drawn but
dealt: of 12 blocks two are clean, two carry one damaged shard, six carry two and two carry three,
in a seeded order.  The wanted verdicts are the definition's, the wanted image is the input with
the rows a verdict names replaced by the oracle's reconstruct with those rows absent; the oracle
defines both for every block, so no draw is left out."""
import numpy as np
import pytest

from test_heal_pair import ROWS, check, label, want_image
from test_locate_pair import CLEAN, UNKNOWN, want_pairs
from test_verify import Lay, stripes

SHAPES = [(10, 4), (6, 3), (16, 4), (7, 3)]
FALLBACK = {(7, 3)}
SIZES = [16, 48, 1023, 1041, 2049, 4099]
DEAL = [0, 0, 1, 1, 2, 2, 2, 2, 2, 2, 3, 3]


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    rsmi = pytest.importorskip("rsmi")
    if not torch.cuda.is_available() or rsmi.device_count() == 0:
        pytest.skip("no GPU")
    return torch, rsmi


def draw(seed):
    rng = np.random.default_rng(0x4EA1 + seed)
    k, m = SHAPES[seed % len(SHAPES)]
    S = SIZES[int(rng.integers(len(SIZES)))]
    aligned = bool(seed // len(SHAPES) % 2)
    deal = rng.permutation(DEAL)
    sh = stripes(k, m, S, len(deal)).copy()
    for b, nd in enumerate(deal):
        for x in rng.choice(k + m, size=int(nd), replace=False):
            lo = int(rng.integers(S))
            ext = int(min(S - lo, rng.choice([1, 1, 2, 17, 1100, S])))
            sh[b, x, lo:lo + ext] ^= rng.integers(1, 256, size=ext, dtype=np.uint8)
    return k, m, S, aligned, deal, sh


def check_deal(k, m, S, deal, sh, want, image):
    """What the distance promises of the definition's verdicts and image, whatever the draw."""
    full = stripes(k, m, S, len(deal))
    assert np.array_equal(want[:, 0] != CLEAN, deal > 0)
    assert (want[deal == 1, 1] == CLEAN).all() and (want[deal == 1, 0] >= 0).all()
    if m >= 4:
        assert (want[deal == 2, 1] >= 0).all(), "the distance names two damaged shards"
    for b in range(len(deal)):
        if deal[b] <= (2 if m >= 4 else 1):
            assert np.array_equal(image[b], full[b]), b  # within the distance: the original bytes
        if want[b, 0] == UNKNOWN:
            assert np.array_equal(image[b], sh[b]), b


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(16))
def test_fuzz(gpu, seed):
    torch, rsmi = gpu
    k, m, S, aligned, deal, sh = draw(seed)
    want = want_pairs(k, m, sh)
    image = want_image(k, m, sh, want)
    check_deal(k, m, S, deal, sh, want, image)
    lay = Lay(rsmi, k, m, S, sh.shape[0], aligned)
    lab = ROWS if (k, m) in FALLBACK else label(lay)
    with rsmi.Codec(k, m) as c:
        _, got_image = check(torch, c, lay, sh, lab, want)
    assert np.array_equal(got_image, image)
