"""Every instantiated scrub kernel against the CPU oracles, exactly.

rs_scrub_kernels.hip builds rs_scrub_mfma_kernel<K, MT, WPS, UA> for K in SCRUB_KS x MT in 1..4 x
both layouts: 80 kernels, each its own unrolled code with its own ring geometry (rs_verify_kernel's)
and its own pairing of the K + MT shards into (K + MT + 1) / 2 accumulators.  This module runs every
one of them on clean stripes at six sizes and on a sheet of aimed damage, and proves by the launch
label that the instantiation was reached.  The expected values are test_scrub.py's: flags from the
oracle's encode of the data rows as stored and from where the damage was put, raws from the
byte-serial CRC of every row as stored.  There are no tolerances.
"""
import time

import numpy as np
import pytest

from test_scrub import NB, check, entries_of, fill_padded, sheet, want_entries
from test_scrub_abi import MTS, SCRUB_KS, all_labels, scrub_label
from test_verify import GAP, Lay, assert_mds, stripes

# every instantiation a test of this module ran and asserted by its exact label
SEEN = set()
WALL = {}

CLEAN_S = [16, 17, 1008, 1025, 4097, 5125]
SHEET_S = 2085   # 3 tiles of one unit; 130 full chunks and a last chunk of 5 bytes
# one byte in each dword of a chunk; the tile seams; the last full chunk and the first and last
# byte of the partial chunk
SHEET_POS = [0, 5, 10, 15, 1023, 1024, 2047, 2048, 2079, 2080, 2084]


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    rsmi = pytest.importorskip("rsmi")
    if not torch.cuda.is_available() or rsmi.device_count() == 0:
        pytest.skip("no GPU")
    yield torch, rsmi
    print("\nscrub matrix: instantiations run and asserted by label: %d/%d" % (len(SEEN & all_labels()), 80))
    print("scrub matrix: wall seconds:", ", ".join("%s %.2f" % kv for kv in sorted(WALL.items())))


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
@pytest.mark.parametrize("K", SCRUB_KS)
def test_every_instantiation(gpu, K, aligned):
    """rs_scrub_mfma_kernel<K, MT> for MT = 1..4 through Codec(K, MT), a plan of one tile: clean
    stripes at six sizes with a sentinel in every padding and gap byte, then the damage sheet."""
    torch, rsmi = gpu
    t0 = time.perf_counter()
    mine = set()
    for MT in MTS:
        assert_mds(rsmi, K, MT)
        label = scrub_label(K, MT, aligned)
        with rsmi.Codec(K, MT) as c:
            for S in CLEAN_S:
                lay = Lay(rsmi, K, MT, S, NB, aligned)
                host = fill_padded(lay, stripes(K, MT, S))
                assert host[(lay.off + lay.bs - 1) if aligned else 0] == GAP
                check(torch, rsmi, c, lay, host, label, np.zeros((NB, MT), dtype=bool), (K, MT, S, aligned, "clean"))
            lay, host, want, moved, full = sheet(rsmi, K, MT, SHEET_S, SHEET_POS, aligned)
            raws = check(torch, rsmi, c, lay, host, label, want, (K, MT, SHEET_S, aligned, "sheet"))
            assert np.array_equal(entries_of(rsmi, raws, SHEET_S) != want_entries(full), moved), (K, MT, aligned)
        mine.add(label)
    assert mine == {scrub_label(K, MT, aligned) for MT in MTS} and len(mine) == 4
    SEEN.update(mine)
    WALL["K=%d,%s" % (K, "aligned" if aligned else "split")] = time.perf_counter() - t0
