"""The store path of the headline kernels (store_policy, csrc/rs_plan.hpp).

RS(10,4) rows of at most 32 KiB, the rows that take the grouped tile order, run their plain aligned
encode on a kernel of its own: how it stores the parity rows (three nontemporal, the last one
plain) is a template parameter that the launch label does not print.  The one-row
reconstruct keeps its kernel; the 2 KiB wave tile tried for it was not kept, so every
launch here has 1 KiB tiles.  No choice of store instruction may change a byte.

GPU: RS(10,4) encode, then ReconstructData of shard 0 in place, rows at rsmi_recommended_pitch(S)
in a buffer with guard bytes before and after.  After each launch the whole buffer, guards and row
padding included, is compared with the oracle's rows, so a byte written at or past S of a row, or
outside the blocks, fails the case; the launch label must be what (K, MT) always gave.
  Rows: 17 (a second chunk of one byte), 1025 and 2049 (one byte past one and two 1 KiB tiles),
2048 (two exact tiles), 26215 (the headline's: 26 tiles, a 7-byte last chunk).
  Blocks: 1, 3 and 11 of every row.  At 26215 bytes 3 blocks are 20 workgroups: past the
multiple-of-8 head (16 grouped, 4 plain) with a block boundary inside a workgroup; 11 blocks are 72
workgroups, which option waves_per_cu = 1 (64 workgroups on an MI355X) turns into the strided loop
with head = 0.
  Neighbour: RS(10,4) rows of 104858 bytes (the 1 MiB block) are past the grouped rows and keep the
kernel of their cache policy; result and label stay.
"""
import numpy as np
import pytest

import oracle_lib as orc

K, M, N = 10, 4, 14
S_HEAD = 26215
LABEL_ENC = "rs_fast_kernel<K=10,MT=4,NT=1>"
LABEL_REC = "rs_fast_kernel<K=10,MT=1,NT=2>"


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    rsmi = pytest.importorskip("rsmi")
    if not torch.cuda.is_available() or rsmi.device_count() == 0:
        pytest.skip("no GPU")
    return torch, rsmi


def workgroups(S, nb):
    """Workgroups of a one-tile-per-wave launch (1 KiB of a row per wave, four waves)."""
    tpb = ((S + 15) // 16 + 63) // 64
    return (nb * tpb + 3) // 4


_FULL = {}


def full_blocks(S, nb):
    """nb blocks of K random rows with the oracle's parity, computed once per shape and left
    unchanged; the oracle also rebuilds shard 0 of every block from the survivors."""
    key = (S, nb)
    if key not in _FULL:
        data = np.random.default_rng(77 * S + nb).integers(0, 256, size=(nb, K, S), dtype=np.uint8)
        full = np.concatenate([data, orc.encode_fast(K, M, data, threads=4)], axis=1)
        present = [i != 0 for i in range(N)]
        for b in range(nb):
            erased = full[b].copy()
            erased[0] = 0xEE
            rc, sh = orc.reconstruct(K, M, erased, present, True)
            assert rc == 0 and np.array_equal(sh, full[b])
        full.setflags(write=False)
        _FULL[key] = full
    return _FULL[key]


def _case(torch, rsmi, S, nb, waves_per_cu):
    rs, off = rsmi.recommended_pitch(S), 64
    assert rs % 16 == 0 and rs >= S
    bs = N * rs
    full = full_blocks(S, nb)
    host = np.full(off + nb * bs + 64, 0x5A, dtype=np.uint8)

    def rows(buf):
        return np.lib.stride_tricks.as_strided(buf[off:], shape=(nb, N, S), strides=(bs, rs, 1))

    rows(host)[:, :K] = full[:, :K]
    expect = host.copy()
    rows(expect)[:] = full
    stream = torch.cuda.current_stream().cuda_stream
    with rsmi.Codec(K, M) as c:
        if waves_per_cu:
            c.set_option("waves_per_cu", waves_per_cu)
        d = torch.from_numpy(host.copy()).cuda()
        base = d.data_ptr() + off
        c.encode_batch_dev(base, rs, bs, base + K * rs, rs, bs, S, nb, stream)
        torch.cuda.synchronize()
        assert c.last_kernel() == LABEL_ENC, c.last_kernel()
        assert np.array_equal(d.cpu().numpy(), expect), (S, nb, waves_per_cu, "encode")
        erased = expect.copy()
        rows(erased)[:, 0] = 0xEE
        d.copy_(torch.from_numpy(erased))
        c.reconstruct_batch_dev(base, rs, bs, S, nb, [i != 0 for i in range(N)], True, stream)
        torch.cuda.synchronize()
        assert c.last_kernel() == LABEL_REC, c.last_kernel()
        assert np.array_equal(d.cpu().numpy(), expect), (S, nb, waves_per_cu, "reconstruct")


# (row bytes, blocks, waves_per_cu)
CASES = [(S, nb, 0) for S in (17, 1025, 2048, 2049, S_HEAD) for nb in (1, 3, 11)]
CASES += [(S, 11, 1) for S in (17, 1025, 2048, 2049, S_HEAD)]


def test_grids_cross_the_boundaries():
    """The grids the docstring names."""
    assert [workgroups(S_HEAD, nb) for nb in (1, 3, 11)] == [7, 20, 72]
    assert workgroups(2048, 1) == 1 and workgroups(2049, 3) == 3 and workgroups(17, 11) == 3


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=["S%d_nb%d_wpc%d" % c for c in CASES])
def test_store_path_launches(gpu, case):
    torch, rsmi = gpu
    _case(torch, rsmi, *case)


@pytest.mark.gpu
def test_neighbour_rows_keep_their_kernel(gpu):
    """RS(10,4) rows of 104858 bytes (one 1 MiB block): the same (K, MT), but past the rows of
    the grouped order, so the launches run the kernels the cache policy gives."""
    torch, rsmi = gpu
    _case(torch, rsmi, 104858, 1, 0)
