"""rsmi_reconstruct_mixed_batch_*_verify, seeded fuzz: (k, m) from the shipped shapes, S up to
40 000, a random layout, random present and required masks with too-few and intact blocks among
them, over the device call, the three host paths and the strided walk (waves_per_cu = 1).  Every case
is checked as test_mixed_verify checks: bytes against the definition and the plain mixed call, R of
every row read or written against the oracle, 0 elsewhere.  No case is skipped; at least half the
blocks of every case have something to rebuild, by construction.  About 300 blocks in all."""
import ctypes

import numpy as np
import pytest

from test_mixed_reconstruct import present_of, stored, wanted, layout
from test_mixed_verify import check_dev, gpu, host_case  # noqa: F401
from test_verify import stripes

SHIPPED = [(2, 1), (4, 2), (10, 4), (16, 4), (5, 5)]
SEEDS = list(range(20))
PATHS = ["dev", "strided", "pinned", "small", "upload"]


def draw(seed):
    """(k, m, S, aligned, present, required or None, data_only) of a case: 12-18 blocks."""
    rng = np.random.default_rng(9000 + seed)
    k, m = SHIPPED[seed % len(SHIPPED)]
    n = k + m
    S = int(rng.choice([int(rng.integers(1, 40001)), int(rng.integers(1, 3000)), 16 * int(rng.integers(1, 600))]))
    nb = int(rng.integers(12, 19))
    losses = []
    for b in range(nb):
        if b % 2 == 0:
            nlost = int(rng.integers(1, m + 1))          # has work: this half by construction
        else:
            nlost = int(rng.choice([0, int(rng.integers(0, m + 1)), int(rng.integers(m + 1, n + 1))]))
        losses.append(tuple(sorted(rng.choice(n, size=nlost, replace=False).tolist())))
    present = present_of(n, losses)
    required = None
    data_only = bool(rng.integers(0, 2))
    if rng.integers(0, 2):
        required = rng.integers(0, 3, size=(nb, n)) != 0
    W = wanted(k, present, required, data_only)
    for b in range(0, nb, 2):                            # ... whatever the masks drew
        if not W[b].any():
            if required is not None:
                required[b, losses[b][0]] = True
            else:
                data_only = False
    W = wanted(k, present, required, data_only)
    work = sum(1 for b in range(nb) if W[b].any() and present[b].sum() >= k)
    assert 2 * work >= nb, (seed, work, nb)
    return k, m, S, bool(rng.integers(0, 2)), present, required, data_only


def test_cases_cover_the_ground():
    cases = [draw(s) for s in SEEDS]
    assert 200 <= sum(c[4].shape[0] for c in cases) <= 400
    assert {(c[0], c[1]) for c in cases} == set(SHIPPED)
    assert any(c[5] is None for c in cases) and any(c[5] is not None for c in cases)
    assert any((c[4].sum(axis=1) < c[0]).any() for c in cases) and any(c[4].all(axis=1).any() for c in cases)
    assert any(c[3] for c in cases) and not all(c[3] for c in cases)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_fuzz(gpu, seed):
    torch, rsmi = gpu
    k, m, S, aligned, present, required, data_only = draw(seed)
    nb = present.shape[0]
    sh = stored(stripes(k, m, S, nb), present)
    path = PATHS[(seed // len(SHIPPED) + seed) % len(PATHS)]
    L = rsmi.lib()
    held = []

    def pinned(nbytes):
        p = L.rsmi_host_alloc(nbytes)
        assert p
        held.append(p)
        return np.ctypeslib.as_array((ctypes.c_uint8 * nbytes).from_address(p))

    def pageable(nbytes):
        return np.empty(nbytes, dtype=np.uint8)

    try:
        with rsmi.Codec(k, m) as c:
            if path in ("dev", "strided"):
                if path == "strided":
                    c.set_option("waves_per_cu", 1)
                check_dev(torch, rsmi, c, layout(rsmi, k, m, S, nb, aligned), sh, present, required, data_only)
            else:
                c.set_option("small_call_bytes", 0 if path == "upload" else 1 << 30)
                bs = (k + m) * S + (0 if aligned else 5)
                host_case(rsmi, c, pinned if path == "pinned" else pageable, k, m, S, sh, present, required, data_only, bs=bs)
    finally:
        for p in held:
            L.rsmi_host_free(p)
