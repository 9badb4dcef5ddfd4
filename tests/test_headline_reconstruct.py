"""The headline's one-row reconstruct on its own kernel (store_policy, waves_cap, csrc/rs_plan.hpp).

RS(10,4) rows of at most 32 KiB, the rows that take the grouped tile order, run their plain aligned
one-row reconstruct on a kernel of its own: it writes the rebuilt row through the L2 (buffer stores
bounded by a descriptor of the row's S bytes) and is capped at 4 waves per SIMD.
Neither choice shows in the launch label, and neither may change a byte.

CPU: a host program of static_asserts over rs_plan.hpp: the (10, 4) encode and the (10, 1)
reconstruct are the only shapes with a kernel of their own on the grouped rows, and what each is.
(That tile_group stays a bijection is tests/test_tile_order.py's check, unchanged.)

GPU: rsmi_reconstruct_batch_dev of every single lost data row, and of row 0 with data_only, in
place, rows at rsmi_recommended_pitch(S) in a buffer with guard bytes before and after.  After every
launch the whole buffer, guards and row padding included, is compared with the oracle's rebuilt
rows, so a byte written at or past S of a row, or outside the blocks, fails the case; the launch
label must be what (K, MT) always gave.
  Rows: 16 (one whole chunk), 17 (a second chunk of one byte), 1031 (a second tile of one 7-byte
chunk), 26215 (the headline's: 26 tiles, a 7-byte last chunk) and 32768 (32 exact tiles, the
longest row of the new kernel); 32784 (one chunk more) is past the grouped rows and keeps the
kernel of its cache policy.
  Blocks: 1, 3 and 41 of every row.  At 26215 bytes these are 7 workgroups (below 8: head 0), 20
(16 grouped and 4 plain, a block boundary inside a workgroup) and 267 (XCD ranges of 33 with 3
left over).
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_lib as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "filedag-storage_amd", "csrc")

K, M, N = 10, 4, 14
LABEL_REC = "rs_fast_kernel<K=10,MT=1,NT=2>"
ROWS = (16, 17, 1031, 26215, 32768, 32784)
BLOCKS = (1, 3, 41)

PLAN_PROGRAM = r"""
#include "rs_plan.hpp"
using namespace rsmi;
constexpr int nt(int K, int MT) { return K >= 4 * MT ? 2 : 1; }
constexpr int own_kernels() {
    int n = 0;
    for (int K = 1; K <= 16; K++)
        for (int MT = 1; MT <= kMaxMT; MT++) n += grouped_kernel_shape(K, MT, nt(K, MT));
    return n;
}
static_assert(own_kernels() == 2, "the headline's encode and one-row reconstruct alone");
static_assert(grouped_kernel_shape(10, 4, 1) && store_policy(10, 4, 1) == 2 && waves_cap(10, 4) == 0, "encode");
static_assert(grouped_kernel_shape(10, 1, 2) && store_policy(10, 1, 2) == kStoreWriteThrough, "reconstruct");
static_assert(waves_cap(10, 1) >= kMinWavesPerSimd && waves_cap(10, 1) <= 8, "a cap at or above the floor");
static_assert(store_policy(10, 2, 2) == 0 && store_policy(4, 2, 1) == 1 && waves_cap(16, 1) == 0, "the others");
static_assert(kGroupedRowMax == 32768u, "rows of at most 32 KiB");
int main() { return 0; }
"""


# ---------------------------------------------------------------- CPU
def test_plan_constants(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "needs a host C++ compiler"
    src = tmp_path / "plan.cpp"
    src.write_text(PLAN_PROGRAM)
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", CSRC, str(src)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr


def workgroups(S, nb):
    """Workgroups of a one-tile-per-wave launch (1 KiB of a row per wave, four waves)."""
    tpb = ((S + 15) // 16 + 63) // 64
    return (nb * tpb + 3) // 4


def test_grids_cross_the_boundaries():
    """The grids the docstring names."""
    assert [workgroups(26215, nb) for nb in BLOCKS] == [7, 20, 267]
    assert workgroups(16, 1) == 1 and workgroups(1031, 3) == 2 and workgroups(32768, 41) == 328
    assert workgroups(32784, 1) == 9


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    rsmi = pytest.importorskip("rsmi")
    if not torch.cuda.is_available() or rsmi.device_count() == 0:
        pytest.skip("no GPU")
    return torch, rsmi


_FULL = {}


def full_blocks(S, nb):
    """nb blocks of K random rows with the oracle's parity, computed once per shape and left
    unchanged."""
    key = (S, nb)
    if key not in _FULL:
        data = np.random.default_rng(131 * S + nb).integers(0, 256, size=(nb, K, S), dtype=np.uint8)
        full = np.concatenate([data, orc.encode_fast(K, M, data, threads=4)], axis=1)
        full.setflags(write=False)
        _FULL[key] = full
    return _FULL[key]


def oracle_rebuild(full, lost, data_only):
    """The oracle's ReconstructData / Reconstruct of every block with row `lost` erased."""
    nb, _, S = full.shape
    sh = np.ascontiguousarray(full).copy()
    sh[:, lost] = 0xEE
    present = np.array([0 if i == lost else 1 for i in range(N)], dtype=np.uint8)
    rc = orc.lib().rs_cpu_reconstruct_batch(K, M, orc.ptr(sh), N * S, S, nb, orc.ptr(present), 1 if data_only else 0, 4)
    assert rc == 0, rc
    return sh


CASES = [(S, nb) for S in ROWS for nb in BLOCKS]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=["S%d_nb%d" % c for c in CASES])
def test_one_row_reconstruct(gpu, case):
    torch, rsmi = gpu
    S, nb = case
    rs, off = rsmi.recommended_pitch(S), 64
    assert rs % 16 == 0 and rs >= S
    bs = N * rs
    full = full_blocks(S, nb)
    host = np.full(off + nb * bs + 64, 0x5A, dtype=np.uint8)

    def rows(buf):
        return np.lib.stride_tricks.as_strided(buf[off:], shape=(nb, N, S), strides=(bs, rs, 1))

    rows(host)[:] = full
    stream = torch.cuda.current_stream().cuda_stream
    with rsmi.Codec(K, M) as c:
        d = torch.empty(host.size, dtype=torch.uint8, device="cuda")
        # every single lost data row, then row 0 once more through ReconstructData
        for lost, data_only in [(i, False) for i in range(K)] + [(0, True)]:
            expect = host.copy()
            rows(expect)[:] = oracle_rebuild(full, lost, data_only)
            erased = host.copy()
            rows(erased)[:, lost] = 0xEE
            d.copy_(torch.from_numpy(erased))
            c.reconstruct_batch_dev(d.data_ptr() + off, rs, bs, S, nb, [i != lost for i in range(N)], data_only,
                                    stream)
            torch.cuda.synchronize()
            assert c.last_kernel() == LABEL_REC, (c.last_kernel(), lost, data_only)
            assert np.array_equal(d.cpu().numpy(), expect), (S, nb, lost, data_only)
