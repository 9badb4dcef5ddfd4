"""Seeded random ragged encodes against the oracle, through the device call and the three host legs.

Each case draws (k, m) from the shipped shapes, 1-200 blocks, every block's S from 1 to 70 000 with
a bias to the seams (16, the 1 024-byte tile, the 4 096-byte unit), and per block the form of each
half: aligned with a random stride surplus, or at a random byte phase with a random pitch >= S; the
two halves are drawn independently, blocks leave random gaps.  Both images are compared whole
against the sentinel-filled expectation (test_ragged_encode.py).  No case is skipped: a draw is
shaped to fit, never rejected."""
import numpy as np
import pytest

from test_ragged_encode import Batch, round16, run_dev, run_host

SHAPES = [(10, 4), (4, 2), (16, 4), (2, 1), (5, 5), (7, 2), (12, 3)]
SEAM_SIZES = [1, 2, 15, 16, 17, 31, 32, 33, 1008, 1023, 1024, 1025, 1040, 2047, 2048, 2049, 4095, 4096, 4097, 4112,
              8191, 8192, 8193]
BUDGET = 6 << 20   # bytes of data rows per case: keeps a case within seconds


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    rsmi = pytest.importorskip("rsmi")
    if not torch.cuda.is_available() or rsmi.device_count() == 0:
        pytest.skip("no GPU")
    return torch, rsmi


def draw(seed):
    rng = np.random.default_rng(seed)
    k, m = SHAPES[seed % len(SHAPES)]
    nb = int(rng.integers(1, 201))
    b = Batch(k, m, int(rng.integers(0, 16)), int(rng.integers(0, 16)))
    spent = 0
    for i in range(nb):
        r = rng.random()
        if r < 0.5:
            S = int(rng.choice(SEAM_SIZES)) + int(rng.integers(-1, 2)) * int(rng.random() < 0.3)
        elif r < 0.9:
            S = int(rng.integers(1, 6000))
        else:
            S = int(rng.integers(6000, 70001))
        S = max(1, S)
        if spent + k * S > BUDGET:   # shaped to fit: the large sizes come early or not at all
            S = int(rng.choice(SEAM_SIZES))
        spent += k * S
        v = int(rng.integers(0, 3))
        gap = int(rng.integers(0, 3))
        # each half on its own: aligned with a surplus, or any phase and pitch
        if rng.random() < 0.5:
            doff, ds = round16(b.dcur) + 16 * gap, round16(S) + 16 * int(rng.integers(0, 4))
        else:
            doff, ds = b.dcur + int(rng.integers(0, 40)), S + int(rng.integers(0, 20))
        if rng.random() < 0.5:
            poff, ps = round16(b.pcur) + 16 * gap, round16(S) + 16 * int(rng.integers(0, 4))
        else:
            poff, ps = b.pcur + int(rng.integers(0, 40)), S + int(rng.integers(0, 20))
        b.add(S, doff, ds, poff, ps, v)
    return b


def test_draws_are_well_formed():
    """CPU: every seed gives a batch whose parity rows overlap nothing, within the budget, and the
    seeds together reach every class and both seams."""
    classes, sizes = set(), set()
    for seed in range(14):
        b = draw(seed)
        assert 1 <= len(b.rows) <= 200
        cover = np.zeros(b.pcur, dtype=np.uint8)
        for S, doff, ds, poff, ps in b.rows:
            assert S >= 1 and ds >= S and ps >= S
            for j in range(b.m):
                cover[poff + j * ps:poff + j * ps + S] += 1
        assert cover.max() == 1, seed
        classes |= set(b.classes(0, 0))
        sizes |= {r[0] for r in b.rows}
    assert classes == {0, 1, 2}
    assert {1023, 1024, 1025, 4096, 4097} <= sizes and max(sizes) > 6000 and min(sizes) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(14))
def test_ragged_fuzz(gpu, seed):
    torch, rsmi = gpu
    b = draw(seed)
    with rsmi.Codec(b.k, b.m) as c:
        run_dev(torch, c, b, ("fuzz", seed, "device"))
        if seed % 2:
            c.set_option("small_call_bytes", 300000)   # several chunks on the staged legs
        run_host(torch, rsmi, c, b, True, True, ("fuzz", seed, "page-locked in place"))
        run_host(torch, rsmi, c, b, False, False, ("fuzz", seed, "pageable"))
        run_host(torch, rsmi, c, b, bool(seed & 2), not (seed & 2), ("fuzz", seed, "one half page-locked"))
