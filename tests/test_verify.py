"""Encoder.Verify on the GPU against the CPU oracle, exactly.

Every expected flag is  want[b, j] = (oracle encode of block b's data rows)[j] != stored parity
row j of block b, anywhere in [0, S).  There are no tolerances.  The cases are a few MB each.

  1  clean stripes with every padding byte a sentinel (the padding trap), both layouts
  2  one flipped byte at the tile and chunk edges, in a parity row, a data row, a padding byte
  3  damage that one parity row cancels: per-row attribution and the coefficient tables
  4  m > 4: two launch tiles, the flag index is the parity row across the seam
  5  shapes without an rs_verify_kernel: encode into scratch + rs_compare_rows_kernel
  6  waves_per_cu = 1: the grid-stride loop
  7  stream order, with no host sync between the steps
  8  host paths: the chunked pipeline, page-locked rows in place, the small call, Erasure.verify
  9  no side effects on the encode and reconstruct of the same context
"""
import ctypes
import os

import numpy as np
import pytest

import oracle_lib as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NB = 3
TILE = 1024                    # 64 lanes x 16 bytes
PAD_DATA, PAD_PARITY, GAP = 0xA5, 0x3C, 0x77   # sentinels: data padding, parity padding, between blocks


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    rsmi = pytest.importorskip("rsmi")
    if not torch.cuda.is_available() or rsmi.device_count() == 0:
        pytest.skip("no GPU")
    return torch, rsmi


_ORACLE = {}


def stripes(k, m, S, nb=NB):
    """(nb, k + m, S) clean shards from the oracle, computed once per shape and never written."""
    key = (k, m, S, nb)
    if key not in _ORACLE:
        rng = np.random.default_rng(1000003 * k + 10007 * m + 31 * S + nb)
        data = rng.integers(0, 256, size=(nb, k, S), dtype=np.uint8)
        par = np.stack([orc.encode(k, m, data[b]) for b in range(nb)])
        full = np.concatenate([data, par], axis=1)
        full.setflags(write=False)
        _ORACLE[key] = full
    return _ORACLE[key]


def want_flags(k, m, shards):
    """The definition, from the oracle: shards (nb, k + m, S) as stored."""
    nb = shards.shape[0]
    out = np.zeros((nb, m), dtype=bool)
    for b in range(nb):
        enc = orc.encode(k, m, np.ascontiguousarray(shards[b, :k]))
        out[b] = (enc != shards[b, k:]).any(axis=1)
    return out


class Lay:
    """nb blocks of n rows of S bytes in one byte buffer.  aligned: rows at
    rsmi_recommended_pitch(S) from a 256-byte-aligned base, a gap of 48 bytes after every block;
    split: rows back to back at pitch S from an odd base offset.  Everything that is not a row
    byte holds a sentinel: data-row padding, parity-row padding and the gaps differ."""

    def __init__(self, rsmi, k, m, S, nb, aligned, rs=None):
        self.k, self.m, self.n, self.S, self.nb, self.aligned = k, m, k + m, S, nb, aligned
        self.rs = rs if rs is not None else (rsmi.recommended_pitch(S) if aligned else S)
        self.off = 0 if aligned else 3
        self.bs = self.n * self.rs + (48 if aligned else 0)
        self.size = self.off + nb * self.bs + 64

    def fill(self, shards):
        host = np.full(self.size, GAP, dtype=np.uint8)
        for b in range(self.nb):
            for r in range(self.n):
                o = self.off + b * self.bs + r * self.rs
                host[o:o + self.rs] = PAD_DATA if r < self.k else PAD_PARITY
        self.rows(host)[:] = shards
        return host

    def rows(self, host):
        return np.lib.stride_tricks.as_strided(host[self.off:], shape=(self.nb, self.n, self.S),
                                               strides=(self.bs, self.rs, 1))

    def label(self):
        return "rs_verify_kernel<K=%d,MT=%d>%s" % (self.k, min(self.m, 4), "" if self.aligned else ",UA")


def run_dev(torch, c, lay, host, label):
    """rsmi_verify_batch_dev over host's bytes: the flags (nb, m) as bool.  The flags tensor starts
    poisoned (the call zeroes it), the buffer must come back byte for byte, the label must match."""
    d = torch.from_numpy(host.copy()).cuda()
    assert d.data_ptr() % 256 == 0
    bad = torch.full((lay.nb * lay.m,), 0x5EED, dtype=torch.int32, device="cuda")
    base = d.data_ptr() + lay.off
    c.verify_batch_dev(base, lay.rs, lay.bs, base + lay.k * lay.rs, lay.rs, lay.bs, lay.S, lay.nb, bad.data_ptr(),
                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert c.last_kernel() == label, (c.last_kernel(), label)
    assert np.array_equal(d.cpu().numpy(), host), "verify wrote to the shards"
    return bad.cpu().numpy().reshape(lay.nb, lay.m) != 0


# ---------------------------------------------------------------- 1: clean stripes, the padding trap
SHAPES_1 = [(2, 1), (4, 2), (10, 4), (16, 4)]
SIZES_1 = [16, 17, 31, 1008, 1024, 1025, 1040, 4099]


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
@pytest.mark.parametrize("k,m", SHAPES_1)
def test_clean_stripes_and_padding(gpu, k, m, aligned):
    torch, rsmi = gpu
    with rsmi.Codec(k, m) as c:
        for S in SIZES_1:
            lay = Lay(rsmi, k, m, S, NB, aligned)
            full = stripes(k, m, S)
            host = lay.fill(full)
            if aligned and lay.rs > S:  # the sentinels are really there, and differ
                assert host[lay.off + S] == PAD_DATA and host[lay.off + k * lay.rs + S] == PAD_PARITY
            assert not want_flags(k, m, full).any()
            got = run_dev(torch, c, lay, host, lay.label())
            assert not got.any(), (k, m, S, aligned, got)


# ---------------------------------------------------------------- 2: one flipped byte
def flip_positions(S):
    return sorted({0, TILE - 1, TILE, S - 1, S - 16})


def assert_mds(rsmi, k, m):
    """Every parity coefficient is non-zero, so one damaged data byte changes every parity row."""
    with rsmi.Codec(k, m) as c:
        M = np.frombuffer(c.encode_matrix(), dtype=np.uint8).reshape(k + m, k)
    assert (M[k:] != 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
@pytest.mark.parametrize("S", [1025, 4099])
@pytest.mark.parametrize("k,m", [(10, 4), (4, 2)])
def test_one_flipped_byte(gpu, k, m, S, aligned):
    torch, rsmi = gpu
    assert_mds(rsmi, k, m)
    lay = Lay(rsmi, k, m, S, NB, aligned)
    full = stripes(k, m, S)
    clean = lay.fill(full)
    with rsmi.Codec(k, m) as c:
        for pos in flip_positions(S):
            for j in range(m):  # parity row j of block 1: exactly flag (1, j)
                host = clean.copy()
                lay.rows(host)[1, k + j, pos] ^= 0x40
                want = np.zeros((NB, m), dtype=bool)
                want[1, j] = True
                assert np.array_equal(want_flags(k, m, lay.rows(host)), want)
                got = run_dev(torch, c, lay, host, lay.label())
                assert np.array_equal(got, want), ("parity", pos, j, got)
            for r in (0, k - 1):  # a data row: all m flags of the block
                host = clean.copy()
                lay.rows(host)[1, r, pos] ^= 0x01
                want = np.zeros((NB, m), dtype=bool)
                want[1, :] = True
                assert np.array_equal(want_flags(k, m, lay.rows(host)), want)
                got = run_dev(torch, c, lay, host, lay.label())
                assert np.array_equal(got, want), ("data", pos, r, got)
        if aligned:  # a padding byte at offset S, data row and parity row: still clean
            assert lay.rs > S
            for r in (0, k, k + m - 1):
                host = clean.copy()
                o = lay.off + 1 * lay.bs + r * lay.rs + S
                host[o] ^= 0xFF
                got = run_dev(torch, c, lay, host, lay.label())
                assert not got.any(), ("padding", r, got)


# ---------------------------------------------------------------- 3: cancelling damage
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
@pytest.mark.parametrize("k,m", [(10, 4), (4, 2)])
def test_cancelling_damage(gpu, k, m, aligned):
    """One data byte corrupted and parity row j alone replaced by the oracle's parity of the
    corrupted data: flag j is clear and every other flag of the block is set."""
    torch, rsmi = gpu
    assert_mds(rsmi, k, m)
    S = 1025
    lay = Lay(rsmi, k, m, S, NB, aligned)
    full = stripes(k, m, S)
    with rsmi.Codec(k, m) as c:
        for j in range(m):
            sh = full.copy()
            sh[1, j % k, 517] ^= 0x5A
            sh[1, k + j] = orc.encode(k, m, np.ascontiguousarray(sh[1, :k]))[j]
            want = np.zeros((NB, m), dtype=bool)
            want[1, :] = True
            want[1, j] = False
            assert np.array_equal(want_flags(k, m, sh), want)
            got = run_dev(torch, c, lay, lay.fill(sh), lay.label())
            assert np.array_equal(got, want), (j, got)


# ---------------------------------------------------------------- 4: m > 4, two launch tiles
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
def test_two_launch_tiles(gpu, aligned):
    """RS(5,5): parity rows 0..3 in the first tile, row 4 in the second (MT = 1, the last label)."""
    torch, rsmi = gpu
    k, m, S = 5, 5, 1040
    lay = Lay(rsmi, k, m, S, NB, aligned)
    full = stripes(k, m, S)
    label = "rs_verify_kernel<K=5,MT=1>" + ("" if aligned else ",UA")
    with rsmi.Codec(k, m) as c:
        assert not run_dev(torch, c, lay, lay.fill(full), label).any()
        for j in (3, 4, 0):
            sh = full.copy()
            sh[2, k + j, 1033] ^= 0x80
            want = np.zeros((NB, m), dtype=bool)
            want[2, j] = True
            assert np.array_equal(want_flags(k, m, sh), want)
            got = run_dev(torch, c, lay, lay.fill(sh), label)
            assert np.array_equal(got, want), (j, got)
        sh = full.copy()  # a data byte: all five flags, both tiles
        sh[0, 2, 7] ^= 0x02
        want = want_flags(k, m, sh)
        assert want[0].all() and not want[1:].any()
        assert np.array_equal(run_dev(torch, c, lay, lay.fill(sh), label), want)


# ---------------------------------------------------------------- 5: fallback shapes
@pytest.mark.gpu
@pytest.mark.parametrize("k,m,S,aligned", [(7, 2, 1025, True), (20, 4, 333, True), (4, 2, 5, False)],
                         ids=["7-2", "20-4", "4-2-S5-pitch5"])
def test_fallback_shapes(gpu, k, m, S, aligned):
    """K without an instantiation, K > 16, and unaligned rows shorter than 16 bytes: the encode
    into scratch and rs_compare_rows_kernel."""
    torch, rsmi = gpu
    lay = Lay(rsmi, k, m, S, NB, aligned)
    assert aligned or lay.rs == S == 5
    full = stripes(k, m, S)
    label = "rs_compare_rows_kernel"
    with rsmi.Codec(k, m) as c:
        assert not run_dev(torch, c, lay, lay.fill(full), label).any()
        sh = full.copy()
        sh[1, k + m - 1, S - 1] ^= 0x10
        want = np.zeros((NB, m), dtype=bool)
        want[1, m - 1] = True
        assert np.array_equal(want_flags(k, m, sh), want)
        assert np.array_equal(run_dev(torch, c, lay, lay.fill(sh), label), want)
        sh = full.copy()
        sh[2, k - 1, 0] ^= 0x01
        want = want_flags(k, m, sh)
        assert want[2].all() and not want[:2].any()
        assert np.array_equal(run_dev(torch, c, lay, lay.fill(sh), label), want)


# ---------------------------------------------------------------- 6: waves_per_cu = 1
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
@pytest.mark.parametrize("many", [False, True], ids=["9-blocks", "past-the-grid"])
def test_waves_per_cu_1(gpu, many, aligned):
    """RS(10,4), S = 4099 (5 tiles per block) with option waves_per_cu = 1, one damaged block among
    the rest.  9 blocks are 45 tiles, fewer than the capped grid's waves (num_cu / 4 workgroups of
    4 waves: 256 on an MI355X), so that case only pins the capped launch; the second case has more
    tiles than the capped grid has waves, so every wave of it strides to a second tile, and the
    damage sits in a block only the second pass reaches."""
    torch, rsmi = gpu
    k, m, S = 10, 4, 4099
    tpb = ((S + 15) // 16 + 63) // 64
    waves = max(1, torch.cuda.get_device_properties(0).multi_processor_count // 4) * 4
    nb = waves // tpb + 8 if many else 9
    assert (nb * tpb > waves) == many
    lay = Lay(rsmi, k, m, S, nb, aligned)
    full = stripes(k, m, S, nb)
    with rsmi.Codec(k, m) as c:
        c.set_option("waves_per_cu", 1)
        assert not run_dev(torch, c, lay, lay.fill(full), lay.label()).any()
        sh = full.copy()
        sh[nb - 2, k + 2, 4098] ^= 0x04
        want = np.zeros((nb, m), dtype=bool)
        want[nb - 2, 2] = True
        assert np.array_equal(want_flags(k, m, sh), want)
        assert np.array_equal(run_dev(torch, c, lay, lay.fill(sh), lay.label()), want)
        sh = full.copy()
        sh[nb - 1, 3, 4097] ^= 0x04
        want = want_flags(k, m, sh)
        assert want[nb - 1].all() and not want[:nb - 1].any()
        assert np.array_equal(run_dev(torch, c, lay, lay.fill(sh), lay.label()), want)


# ---------------------------------------------------------------- 7: stream order
@pytest.mark.gpu
def test_stream_order(gpu):
    """encode, verify, a torch op that flips one parity byte, verify again, all on one side stream
    with no host sync in between: the first flags are all zero and the second hold exactly that
    flag.  Both flag tensors start poisoned on that stream, so a memset or a kernel issued on
    another stream shows."""
    torch, rsmi = gpu
    k, m, S, nb = 10, 4, 4099, 3
    rs = rsmi.recommended_pitch(S)
    bs = (k + m) * rs
    full = stripes(k, m, S, nb)
    host = np.full(nb * bs, 0x11, dtype=np.uint8)
    rows = np.lib.stride_tricks.as_strided(host, shape=(nb, k + m, S), strides=(bs, rs, 1))
    rows[:, :k] = full[:, :k]
    pinned = torch.from_numpy(host).pin_memory()
    st = torch.cuda.Stream()
    with rsmi.Codec(k, m) as c:
        for warm in (True, False):  # the first pass builds the plan; the second is the test
            d = torch.empty(nb * bs, dtype=torch.uint8, device="cuda")
            bad1 = torch.empty(nb * m, dtype=torch.int32, device="cuda")
            bad2 = torch.empty(nb * m, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                h = st.cuda_stream
                d.copy_(pinned, non_blocking=True)
                bad1.fill_(0x0BAD)
                bad2.fill_(0x0BAD)
                c.encode_batch_dev(d.data_ptr(), rs, bs, d.data_ptr() + k * rs, rs, bs, S, nb, h)
                c.verify_batch_dev(d.data_ptr(), rs, bs, d.data_ptr() + k * rs, rs, bs, S, nb, bad1.data_ptr(), h)
                d[1 * bs + (k + 2) * rs + 1024] ^= 0x08
                c.verify_batch_dev(d.data_ptr(), rs, bs, d.data_ptr() + k * rs, rs, bs, S, nb, bad2.data_ptr(), h)
            st.synchronize()
            got = d.cpu().numpy()
            grow = np.lib.stride_tricks.as_strided(got, shape=(nb, k + m, S), strides=(bs, rs, 1))
            want2 = np.zeros((nb, m), dtype=bool)
            want2[1, 2] = True
            assert np.array_equal(want_flags(k, m, grow), want2)  # the encode ran, then the flip
            assert not bad1.cpu().numpy().any(), warm
            assert np.array_equal(bad2.cpu().numpy().reshape(nb, m) != 0, want2), warm


# ---------------------------------------------------------------- 8: host paths
def _host_flags(c, data, dbs, parity, pbs, S, nb):
    bad = np.full(nb * c.m, 0x5EED, dtype=np.uint32)
    c.verify_batch_host_ptr(data, dbs, parity, pbs, S, nb, bad.ctypes.data)
    return bad.reshape(nb, c.m) != 0


@pytest.mark.gpu
def test_host_pipeline_pageable(gpu):
    """RS(2,1), S = 2049, pageable buffers, more than two chunks of the upload pipeline: one
    damaged parity byte in the first block, the last block and the two blocks on each side of
    every chunk seam; the flags are exactly those."""
    torch, rsmi = gpu
    k, m, S = 2, 1, 2049
    chunk = max(1, (64 << 20) // (3 * rsmi.recommended_pitch(S)))
    nb = 2 * chunk + 3
    assert nb * 3 * S > (2 << 20)  # not a small call
    rng = np.random.default_rng(8)
    data = rng.integers(0, 256, size=(nb, k, S), dtype=np.uint8)
    parity = orc.encode_fast(k, m, data, threads=8)
    hit = sorted({0, nb - 1, chunk - 2, chunk - 1, chunk, chunk + 1, 2 * chunk - 2, 2 * chunk - 1, 2 * chunk,
                  2 * chunk + 1})
    for i, b in enumerate(hit):
        parity[b, 0, (i * 211) % S] ^= 1 << (i % 8)
    want = np.zeros((nb, m), dtype=bool)
    want[hit, 0] = True
    with rsmi.Codec(k, m) as c:
        d0, p0 = data.copy(), parity.copy()
        got = _host_flags(c, data.ctypes.data, k * S, parity.ctypes.data, m * S, S, nb)
        assert c.last_kernel() == "rs_verify_kernel<K=2,MT=1>"
        assert np.array_equal(data, d0) and np.array_equal(parity, p0)
        assert np.array_equal(np.flatnonzero(got[:, 0]), np.array(hit)), np.flatnonzero(got[:, 0])
        assert np.array_equal(got, want)


@pytest.mark.gpu
def test_host_page_locked_in_place(gpu):
    """Data and parity in one rsmi_host_alloc allocation, zero_copy 1: one kernel reads them in
    place over PCIe at pitch S, the unaligned-window form."""
    torch, rsmi = gpu
    k, m, S, nb = 2, 1, 2049, 5
    full = stripes(k, m, S, nb)
    L = rsmi.lib()
    size = nb * (k + m) * S
    p = L.rsmi_host_alloc(size)
    assert p
    try:
        buf = np.ctypeslib.as_array((ctypes.c_uint8 * size).from_address(p))
        rows = buf.reshape(nb, k + m, S)
        with rsmi.Codec(k, m) as c:
            c.set_option("zero_copy", 1)
            bs = (k + m) * S
            for damage in (None, (3, 2, 2048), (4, 0, 0)):
                rows[:] = full
                if damage:
                    rows[damage] ^= 0x20
                want = want_flags(k, m, rows)
                assert want.any() == (damage is not None)
                before = buf.copy()
                got = _host_flags(c, p, bs, p + k * S, bs, S, nb)
                assert c.last_kernel() == "rs_verify_kernel<K=2,MT=1>,UA"
                assert np.array_equal(buf, before)
                assert np.array_equal(got, want), (damage, got)
    finally:
        L.rsmi_host_free(p)


@pytest.mark.gpu
def test_small_call_one_block(gpu):
    """rsmi_verify of one pageable block goes through the page-locked staging (small call)."""
    torch, rsmi = gpu
    for k, m, S in ((2, 1, 2049), (10, 4, 4099)):
        full = stripes(k, m, S)
        with rsmi.Codec(k, m) as c:
            sh = bytearray(full[0].tobytes())
            assert (k + m) * S * 2 <= (2 << 20)
            assert c.verify(sh, S) is True
            assert c.last_kernel() == "rs_verify_kernel<K=%d,MT=%d>,UA" % (k, m)
            assert bytes(sh) == full[0].tobytes()
            sh[(k + m - 1) * S + S - 1] ^= 0x01
            assert c.verify(sh, S) is False
            sh[(k + m - 1) * S + S - 1] ^= 0x01
            sh[0] ^= 0x80
            assert c.verify(sh, S) is False
            sh[0] ^= 0x80
            assert c.verify(sh, S) is True


@pytest.mark.gpu
def test_erasure_verify_golden(gpu):
    """Erasure.verify on the golden RS(10,4) vectors: True; with two shards swapped: False."""
    torch, rsmi = gpu
    z = np.load(os.path.join(GOLDEN, "vectors_k10_m4.npz"))
    for B in (4099, 6, 1):
        shards = [bytes(r.tobytes()) for r in z["shards_%d" % B]]
        e = rsmi.NewErasure(10, 4, B)
        assert e.verify(shards) is True, B
        if B == 4099:
            for a, b in ((0, 1), (3, 12), (10, 13)):
                sw = list(shards)
                sw[a], sw[b] = sw[b], sw[a]
                assert sw[a] != shards[a]
                assert e.verify(sw) is False, (a, b)
        e._codec.close()


# ---------------------------------------------------------------- 9: no side effects
@pytest.mark.gpu
def test_no_side_effects_on_encode_and_reconstruct(gpu):
    """The plan cache and the scratch are shared: after a verify (and after a fallback verify's
    scratch encode) the context's encode and reconstruct still match the oracle and report their
    own labels."""
    torch, rsmi = gpu
    for k, m, S, vlabel, elabel, rlabel in (
            (10, 4, 4099, "rs_verify_kernel<K=10,MT=4>", "rs_fast_kernel<K=10,MT=4,NT=1>", "rs_fast_kernel<K=10,MT=2,NT=2>"),
            (7, 2, 1025, "rs_compare_rows_kernel", "rs_generic_kernel<K=7,MT=2>", "rs_generic_kernel<K=7,MT=2>")):
        lay = Lay(rsmi, k, m, S, NB, True)
        full = stripes(k, m, S)
        with rsmi.Codec(k, m) as c:
            assert not run_dev(torch, c, lay, lay.fill(full), vlabel).any()
            host = lay.fill(full)
            lay.rows(host)[:, k:] = 0xEE
            d = torch.from_numpy(host).cuda()
            h = torch.cuda.current_stream().cuda_stream
            c.encode_batch_dev(d.data_ptr(), lay.rs, lay.bs, d.data_ptr() + k * lay.rs, lay.rs, lay.bs, S, NB, h)
            torch.cuda.synchronize()
            assert c.last_kernel() == elabel
            assert np.array_equal(d.cpu().numpy(), lay.fill(full))
            lost = [1, k + 1]
            host = lay.fill(full)
            lay.rows(host)[:, lost] = 0xEE
            d = torch.from_numpy(host).cuda()
            c.reconstruct_batch_dev(d.data_ptr(), lay.rs, lay.bs, S, NB, [i not in lost for i in range(k + m)],
                                    False, h)
            torch.cuda.synchronize()
            assert c.last_kernel() == rlabel
            assert np.array_equal(d.cpu().numpy(), lay.fill(full))
            assert not run_dev(torch, c, lay, lay.fill(full), vlabel).any()
