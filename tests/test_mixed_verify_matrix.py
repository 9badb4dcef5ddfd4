"""Every instantiated rs_mixed_fused_kernel<K, MT> on both layouts, reached by its rsmi_last_kernel
label through rsmi_reconstruct_mixed_batch_dev_verify and checked as test_mixed_verify checks: the
whole buffer against the definition and against rsmi_reconstruct_mixed_batch_dev on a copy, R of
every row read or written against the oracle, 0 elsewhere.  S = 4097: two units a block, the last
holding one tile of one byte; three blocks with distinct patterns that rebuild MT rows each.  The
list of shapes is held equal to the fill_ calls of the source."""
import itertools

import numpy as np
import pytest

from test_mixed_reconstruct import layout, present_of, stored
from test_mixed_verify import check_dev, fused_label, gpu  # noqa: F401
from test_mixed_verify_abi import SHAPES_K, instantiated
from test_verify import stripes

SHAPES = [(K, MT) for K in SHAPES_K for MT in (1, 2, 3, 4)]
S = 4097


def test_shapes_match_source():
    assert instantiated() == SHAPES and len(SHAPES) == 40


def patterns(K, m, MT):
    """Three distinct patterns of RS(K, m) that lose MT rows: data rows first where K has them, then
    across data and parity, then parity only (all their survivors data rows)."""
    n = K + m
    all_ = list(itertools.combinations(range(n), MT))
    picks = [all_[0], all_[len(all_) // 2], all_[-1]]
    assert len(set(picks)) == 3
    return picks


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "ua"])
@pytest.mark.parametrize("K,MT", SHAPES)
def test_every_kernel(gpu, K, MT, aligned):
    torch, rsmi = gpu
    m = 4
    losses = patterns(K, m, MT)
    present = present_of(K + m, losses)
    sh = stored(stripes(K, m, S, len(losses)), present)
    with rsmi.Codec(K, m) as c:
        lay = layout(rsmi, K, m, S, len(losses), aligned)
        _, raw = check_dev(torch, rsmi, c, lay, sh, present, None, False, fused_label(K, MT, aligned))
    assert raw.any(axis=1).all() and (np.count_nonzero(raw, axis=1) <= K + MT).all()
