"""The coding kernels' workgroup -> tile order (tile_group / launch_head, csrc/rs_plan.hpp).

A coding launch renumbers its first `head` workgroups so that each XCD sweeps one contiguous range
of tiles; the rest keep the plain order.  The mapping is for speed only, so
whatever it is the result must stay bit-exact.

CPU: tests/cpp/test_tile_order.cpp (own main, includes only rs_plan.hpp) is compiled and run plain
and with -fsanitize=address,undefined: tile_group is a permutation of [0, grid) for every grid up
to 4 200 and every multiple of 8 head <= grid, one XCD's workgroups take a contiguous range,
head = 0 is the identity, and launch_head is a multiple of 8 and <= grid.

GPU: launches whose grids cross the head / tail boundary, the multiple-of-8 boundary and a block
boundary inside a workgroup, at the shipped share, each also with option waves_per_cu set; the
whole buffer (guards and padding included) is compared with the oracle and the launch label must
be what it was.  waves_per_cu = 1 caps a grid at num_cu / 4 workgroups (64 on an MI355X), which
none of the small cases reaches, so one more case of 11 blocks (72 workgroups) runs the strided
loop, which keeps head = 0.  The library arms a completion flag on a table launch of
rs_fast_kernel only for a lone block, so case h is two launches: a 3-block table launch (20
workgroups, head 16) and a one-block launch of 8 workgroups (head 8) with its flag armed, whose
return shows that every workgroup was counted exactly once.
"""
import ctypes
import os
import shutil
import subprocess
import threading

import numpy as np
import pytest

import oracle_lib as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "filedag-storage_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "test_tile_order.cpp")


# ---------------------------------------------------------------- CPU: the mapping on the host
@pytest.mark.parametrize("flags", [["-O2"], ["-O2", "-g", "-fsanitize=address,undefined",
                                             "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "asan_ubsan"])
def test_tile_group_host_program(tmp_path, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "needs a host C++ compiler"
    exe = str(tmp_path / "test_tile_order")
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", CSRC, SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "ok", r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    rsmi = pytest.importorskip("rsmi")
    if not torch.cuda.is_available() or rsmi.device_count() == 0:
        pytest.skip("no GPU")
    return torch, rsmi


def nt_of(K, MT):
    return 2 if K >= 4 * MT else 1


def label(K, MT, ua=False, tb=False):
    return "rs_fast_kernel<K=%d,MT=%d,NT=%d>" % (K, MT, nt_of(K, MT)) + (",UA" if ua else "") + (",TB" if tb else "")


def workgroups(S, nb):
    tpb = ((S + 15) // 16 + 63) // 64
    return (nb * tpb + 3) // 4


_FULL = {}


def full_blocks(k, m, S, nb):
    """nb blocks of k random rows with their parity from the oracle, computed once per shape."""
    key = (k, m, S, nb)
    if key not in _FULL:
        data = np.random.default_rng(1000 * k + 10 * m + S + nb).integers(0, 256, size=(nb, k, S), dtype=np.uint8)
        full = np.concatenate([data, orc.encode_fast(k, m, data, threads=4)], axis=1)
        full.setflags(write=False)
        _FULL[key] = full
    return _FULL[key]


class Layout:
    """nb blocks of n rows in one byte buffer with guard bytes before and after; rows at pitch rs
    from byte offset off (aligned layouts: the padding at and past S of each row is guard too)."""

    def __init__(self, n, S, nb, rs, off):
        self.n, self.S, self.nb, self.rs, self.off = n, S, nb, rs, off
        self.bs = n * rs
        self.size = off + nb * self.bs + 64

    def buffer(self, fill):
        return np.full(self.size, fill, dtype=np.uint8)

    def rows(self, host):
        return np.lib.stride_tricks.as_strided(host[self.off:], shape=(self.nb, self.n, self.S),
                                               strides=(self.bs, self.rs, 1))


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _dev_case(torch, rsmi, k, m, S, nb, ua, lost, waves_per_cu):
    """Encode into a guarded device buffer, then (lost given) rebuild those rows in place.  Every
    byte of the buffer is compared with the oracle's."""
    n = k + m
    rs, off = (S + 3, 7) if ua else (rsmi.recommended_pitch(S), 64)
    lay = Layout(n, S, nb, rs, off)
    full = full_blocks(k, m, S, nb)
    host = lay.buffer(0x5A)
    lay.rows(host)[:, :k] = full[:, :k]
    expect = host.copy()
    lay.rows(expect)[:] = full
    with rsmi.Codec(k, m) as c:
        if waves_per_cu:
            c.set_option("waves_per_cu", waves_per_cu)
        d = torch.from_numpy(host.copy()).cuda()
        base = d.data_ptr() + lay.off
        c.encode_batch_dev(base, lay.rs, lay.bs, base + k * lay.rs, lay.rs, lay.bs, S, nb, _stream(torch))
        torch.cuda.synchronize()
        assert c.last_kernel() == label(k, m, ua=ua), c.last_kernel()
        assert np.array_equal(d.cpu().numpy(), expect), (k, m, S, nb, ua, "encode")
        if lost:
            erased = expect.copy()
            lay.rows(erased)[:, lost] = 0xEE
            d.copy_(torch.from_numpy(erased))
            present = [i not in lost for i in range(n)]
            c.reconstruct_batch_dev(base, lay.rs, lay.bs, S, nb, present, True, _stream(torch))
            torch.cuda.synchronize()
            assert c.last_kernel() == label(k, len(lost), ua=ua), c.last_kernel()
            for b in range(nb):  # the oracle rebuilds the same rows from the same survivors
                rc, sh = orc.reconstruct(k, m, np.ascontiguousarray(lay.rows(erased)[b]), present, True)
                assert rc == 0 and np.array_equal(sh, full[b])
            assert np.array_equal(d.cpu().numpy(), expect), (k, m, S, nb, ua, lost, "reconstruct")


S_HEAD = 26215  # the headline's row: 26 tiles, the last of 39 lanes

# (id, k, m, S, blocks, ua, lost rows, workgroups)
DEV_CASES = [
    ("a_head16_tail4", 10, 4, S_HEAD, 3, False, None, 20),
    ("b_grid33", 10, 4, S_HEAD, 5, False, None, 33),
    ("c_grid7_head0", 10, 4, S_HEAD, 1, False, None, 7),
    ("d_reconstruct_shard0", 10, 4, S_HEAD, 3, False, [0], 20),
    ("e_two_tiles_a_block", 16, 4, 1040, 37, False, None, 19),
    ("f_policy1_rs2_1", 2, 1, 4096, 16, False, None, 16),
    ("g_unaligned", 10, 4, S_HEAD, 3, True, None, 20),
    ("strided_72_workgroups", 10, 4, S_HEAD, 11, False, [0], 72),
]


@pytest.mark.gpu
@pytest.mark.parametrize("waves_per_cu", [0, 1], ids=["one_tile_per_wave", "waves_per_cu_1"])
@pytest.mark.parametrize("case", DEV_CASES, ids=[c[0] for c in DEV_CASES])
def test_device_launches(gpu, case, waves_per_cu):
    torch, rsmi = gpu
    _, k, m, S, nb, ua, lost, wgs = case
    assert workgroups(S, nb) == wgs
    _dev_case(torch, rsmi, k, m, S, nb, ua, lost, waves_per_cu)


def _host_rows(rsmi, nbytes):
    p = rsmi.lib().rsmi_host_alloc(nbytes)
    assert p
    return p, np.ctypeslib.as_array((ctypes.c_uint8 * nbytes).from_address(p))


@pytest.mark.gpu
def test_table_launch_three_blocks(gpu):
    """Case h, first half: three callers' page-locked blocks rebuilt by one table launch of 78
    tiles (20 workgroups, head 16); each buffer's guard bytes stay."""
    torch, rsmi = gpu
    k, m, S, T = 10, 4, 26208, 3
    n = k + m
    assert workgroups(S, T) == 20
    L = rsmi.lib()
    full = full_blocks(k, m, S, T)
    with rsmi.Codec(k, m) as c:
        c.set_option("coalesce_lanes", 1)
        c.set_option("coalesce_us", 100000)
        c.set_option("coalesce_max", T)
        bufs = [_host_rows(rsmi, n * S + 64) for _ in range(T)]
        try:
            present = (ctypes.c_uint8 * n)(*[0 if i == 0 else 1 for i in range(n)])
            for t, (p, flat) in enumerate(bufs):
                flat[:] = 0x5A
                flat[:n * S].reshape(n, S)[:] = full[t]
                flat[:S] = 0xEE
            rcs = [None] * T

            def rec(t):
                rcs[t] = L.rsmi_reconstruct_coalesced(c._h, bufs[t][0], S, present, 1)

            th = [threading.Thread(target=rec, args=(t,)) for t in range(T)]
            for x in th:
                x.start()
            for x in th:
                x.join()
            assert rcs == [0] * T
            assert c.last_kernel() == label(k, 1, tb=True), c.last_kernel()
            for t, (p, flat) in enumerate(bufs):
                assert np.array_equal(flat[:n * S].reshape(n, S), full[t]), t
                assert (flat[n * S:] == 0x5A).all(), t
        finally:
            for p, flat in bufs:
                del flat
            for p, _ in bufs:
                L.rsmi_host_free(p)


@pytest.mark.gpu
def test_table_launch_flag_armed(gpu):
    """Case h, second half: a lone page-locked block of 32 tiles a row (8 workgroups, head 8, a
    last tile of 63 lanes) rebuilt in place by a table launch with its completion flag armed.
    The call returns once the launch's last workgroup releases the flag: a workgroup counted twice
    would release it before the rows are whole, one not counted never.  Three calls reuse the
    counter the last workgroup resets."""
    torch, rsmi = gpu
    k, m, S = 10, 4, 32752
    n = k + m
    assert workgroups(S, 1) == 8
    full = full_blocks(k, m, S, 1)[0]
    with rsmi.Codec(k, m) as c:
        c.set_option("coalesce_flag", 1)
        p, flat = _host_rows(rsmi, n * S + 64)
        try:
            for lost in (0, 3, 9):
                flat[:] = 0x5A
                flat[:n * S].reshape(n, S)[:] = full
                flat[lost * S:(lost + 1) * S] = 0xEE
                c.reconstruct_batch_host_ptr(p, n * S, S, 1, [i != lost for i in range(n)], True)
                assert c.last_kernel() == label(k, 1, tb=True), c.last_kernel()
                assert np.array_equal(flat[:n * S].reshape(n, S), full), lost
                assert (flat[n * S:] == 0x5A).all()
        finally:
            del flat
            rsmi.lib().rsmi_host_free(p)
