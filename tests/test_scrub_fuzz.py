"""rsmi_scrub_batch_dev on seeded random shapes, exactly: k, m, S, the layouts of the two halves
and the block count are drawn per seed, and every block takes random damage in data and parity
(or none).  The expected flags are the oracle's encode of the data rows as stored against the
stored parity, the expected raws the byte-serial CRC of every row as stored; where the draw has a
scrub kernel the label must say so, with the layout the two halves add up to.  Each seed is a few
hundred KB at most."""
import numpy as np
import pytest

import oracle_lib as orc
from test_scrub import Outputs, assert_raws
from test_scrub_abi import SCRUB_KS, scrub_label
from test_verify import PAD_DATA, PAD_PARITY, want_flags

SEEDS = list(range(36))


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    rsmi = pytest.importorskip("rsmi")
    if not torch.cuda.is_available() or rsmi.device_count() == 0:
        pytest.skip("no GPU")
    return torch, rsmi


def draw_half(rng, rows, S, aligned):
    """(byte phase, pitch, block stride) of one half: on the 16-byte grid, or rows at a pitch of
    S .. S + 5 from any phase."""
    if aligned:
        rs = (S + 15) // 16 * 16 + 16 * int(rng.integers(0, 3))
        return 0, rs, rows * rs + 16 * int(rng.integers(0, 4))
    rs = S + int(rng.integers(0, 6))
    return int(rng.integers(0, 16)), rs, rows * rs + int(rng.integers(0, 9))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_random_shape(gpu, seed):
    torch, rsmi = gpu
    rng = np.random.default_rng(0x5C2B00 + seed)
    k = int(rng.choice(SCRUB_KS + [7, 9, 11])) if seed % 6 else int(rng.integers(1, 21))
    m = int(rng.integers(1, 5)) if seed % 9 else int(rng.integers(1, 7))
    S = int(rng.choice([int(rng.integers(1, 64)), int(rng.integers(64, 2100)), int(rng.integers(2100, 9000)),
                        int(rng.choice([1024, 4096, 4095, 4097, 8192]))]))
    nb = int(rng.integers(1, 6))
    da, pa = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
    d_off, d_rs, d_bs = draw_half(rng, k, S, da)
    p_off, p_rs, p_bs = draw_half(rng, m, S, pa)

    data = rng.integers(0, 256, size=(nb, k, S), dtype=np.uint8)
    sh = np.concatenate([data, np.stack([orc.encode(k, m, data[b]) for b in range(nb)])], axis=1)
    for b in range(nb):  # no damage, or one to three flipped bits anywhere in the block
        for _ in range(int(rng.integers(0, 4))):
            sh[b, int(rng.integers(0, k + m)), int(rng.integers(0, S))] ^= 1 << int(rng.integers(0, 8))
    want = want_flags(k, m, sh)

    hd = np.full(d_off + nb * d_bs + 64, PAD_DATA, dtype=np.uint8)
    hp = np.full(p_off + nb * p_bs + 64, PAD_PARITY, dtype=np.uint8)
    np.lib.stride_tricks.as_strided(hd[d_off:], shape=(nb, k, S), strides=(d_bs, d_rs, 1))[:] = sh[:, :k]
    np.lib.stride_tricks.as_strided(hp[p_off:], shape=(nb, m, S), strides=(p_bs, p_rs, 1))[:] = sh[:, k:]
    dd, dp = torch.from_numpy(hd.copy()).cuda(), torch.from_numpy(hp.copy()).cuda()
    out = Outputs(torch, nb, k, m)
    with rsmi.Codec(k, m) as c:
        c.scrub_batch_dev(dd.data_ptr() + d_off, d_rs, d_bs, dp.data_ptr() + p_off, p_rs, p_bs, S, nb, out.bad_ptr,
                          out.raw_ptr, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        label = c.last_kernel()
    ctx = (seed, k, m, S, nb, (d_off, d_rs, d_bs), (p_off, p_rs, p_bs), label)
    grid = all(x % 16 == 0 for x in (dd.data_ptr() + d_off, d_rs, d_bs, dp.data_ptr() + p_off, p_rs, p_bs))
    if k in SCRUB_KS and m <= 4 and (grid or S >= 16):
        assert label == scrub_label(k, m, grid), ctx
    else:
        assert label and not label.startswith("rs_scrub"), ctx
    assert np.array_equal(dd.cpu().numpy(), hd) and np.array_equal(dp.cpu().numpy(), hp), ctx
    flags, raws = out.read()
    assert np.array_equal(flags, want), ctx
    assert_raws(rsmi, raws, sh, ctx)
