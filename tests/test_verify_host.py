"""rsmi_verify_batch_host past what test_verify.py reaches, against the CPU oracle, exactly.

verify_host_impl (rsmi_verify.cpp) either runs one kernel over page-locked rows at pitch S (in
place, or over the context's page-locked staging for a small pageable call: the ",UA" label at the
odd S used here), or cuts the call into chunks of about 64 MiB of pitched device rows that rotate
over three staging streams (the aligned kernel: no ",UA").  The upload of a chunk is one 2-D DMA
(S % 8 == 0, contiguous blocks), one 2-D DMA per block (block strides with gaps), or linear copies
and rs_repitch_kernel (other S).  Each of these runs here, with four chunks (the fourth reuses
staging stream 0), with one chunk, and with data and parity in different kinds of memory.

The stored parity is the oracle's (oracle_lib.encode_fast, checked against the scalar oracle on
the damaged blocks) with one bit flipped in the first block, the last block and the two blocks on
each side of every chunk seam.  Every expected flag is stated twice: from where the damage was
put, and as oracle parity != stored parity.  Data, parity and the gap bytes must come back byte
for byte, and the label is pinned.  Everything is bit-exact: there are no tolerances.
"""
import os
import time

import numpy as np
import pytest

import oracle_lib as orc
from test_host_pipeline import Bufs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "filedag-storage_amd", "csrc")

S_2D = 65544    # S % 8 == 0, S % 16 != 0: 2-D DMA rows
S_LIN = 65539   # odd: linear copies and the repitch kernel
S_ODD = 2049    # the mixed-memory cases: rows at pitch S are unaligned windows
S_2D_SMALL = 2056
GAP_DATA, GAP_PARITY = 24, 40            # bytes after every data block / parity block in the padded layouts
FILL_DATA, FILL_PARITY = 0x77, 0x3C      # what those bytes hold
SMALL = 2 << 20                          # option small_call_bytes, the default
WALL = {}


def chunk_blocks(k, m, S):
    """Blocks per chunk of the verify pipeline, as test_host_pipeline_pageable computes it."""
    import rsmi

    return max(1, (64 << 20) // ((k + m) * rsmi.recommended_pitch(S)))


def takes_one_kernel_path(zero_copy, data_pinned, parity_pinned, total, small=SMALL):
    """The path choice of verify_host_impl, restated: true = one kernel over page-locked rows at
    pitch S (in place or staged by CPU copies), false = the chunked pipeline."""
    pinned = data_pinned and parity_pinned
    return bool((zero_copy and pinned) or (total <= small and (2 * total <= small or data_pinned)))


def seam_hits(nb, chunk):
    s = {0, nb - 1}
    for seam in range(chunk, nb, chunk):
        s |= {seam - 2, seam - 1, seam, seam + 1}
    return sorted(b for b in s if 0 <= b < nb)


# ---------------------------------------------------------------- CPU: the rules above match the source
def test_rules_match_source():
    with open(os.path.join(CSRC, "rsmi_verify.cpp")) as f:
        src = f.read()
    body = src[src.index("int verify_host_impl("):src.index('extern "C"')]
    assert "if ((c->opt_zero_copy && pinned) ||" in body
    assert "(total <= size_t(c->opt_small_bytes) && (2 * total <= size_t(c->opt_small_bytes) || zd))) {" in body
    assert "const bool pinned = zd && zp;" in body
    assert "const size_t total = nblocks * (k + m) * S;" in body
    assert "const size_t Sp = rsmi_recommended_pitch(S);" in body
    assert "const size_t in_bs = k * Sp, par_bs = m * Sp;" in body
    assert "const size_t chunk = std::max<size_t>(1, (size_t(64) << 20) / (in_bs + par_bs));" in body
    assert "const int ns = nblocks > chunk ? 3 : 1;" in body
    assert "Staging& st = c->staging[i % ns];" in body
    with open(os.path.join(CSRC, "rsmi_impl.hpp")) as f:
        impl = f.read()
    assert "int opt_zero_copy = 1;" in impl and "long opt_small_bytes = 2L << 20;" in impl


def test_shapes_of_this_module():
    import rsmi

    assert rsmi.recommended_pitch(S_2D) == rsmi.recommended_pitch(S_LIN) == 69632
    assert S_2D % 8 == 0 and S_2D % 16 != 0 and S_LIN % 8 != 0
    ch = chunk_blocks(2, 1, S_2D)
    assert ch == chunk_blocks(2, 1, S_LIN) == 321
    nb = 3 * ch + 2
    assert -(-nb // ch) == 4                      # four chunks: staging[0] serves chunks 0 and 3
    assert seam_hits(nb, ch) == [0, 319, 320, 321, 322, 640, 641, 642, 643, 961, 962, 963, 964]
    assert chunk_blocks(10, 4, S_2D_SMALL) == 1170 and chunk_blocks(2, 1, S_ODD) == 5461


# ---------------------------------------------------------------- GPU plumbing
@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    rsmi = pytest.importorskip("rsmi")
    if not torch.cuda.is_available() or rsmi.device_count() == 0:
        pytest.skip("no GPU")
    yield torch, rsmi
    _REF.clear()
    _BASE.clear()
    print("\nverify host: wall seconds per case:", ", ".join("%s %.2f" % kv for kv in sorted(WALL.items())))


_BASE = {}
_REF = {}


def _ref(k, m, S, nb):
    """(data, parity) of nb blocks: a prefix of one random byte stream, and the oracle's parity;
    computed once per (k, m, S) and read-only."""
    if "bytes" not in _BASE:
        _BASE["bytes"] = np.random.default_rng(50001).integers(0, 256, size=966 * 2 * S_2D, dtype=np.uint8)
    key = (k, m, S)
    if key not in _REF or _REF[key][0].shape[0] < nb:
        data = _BASE["bytes"][:nb * k * S].reshape(nb, k, S)
        par = orc.encode_fast(k, m, data)
        data.setflags(write=False)
        par.setflags(write=False)
        _REF[key] = (data, par)
    data, par = _REF[key]
    return data[:nb], par[:nb]


def _rows(buf, nb, nrows, S, bs):
    return np.lib.stride_tricks.as_strided(buf, shape=(nb, nrows, S), strides=(bs, S, 1))


def _verify_host(gpu, name, k, m, S, nb, hit, label, padded=False, data_pinned=False, parity_pinned=False,
                 zero_copy=None):
    torch, rsmi = gpu
    t0 = time.perf_counter()
    data, par = _ref(k, m, S, nb)
    dbs = k * S + (GAP_DATA if padded else 0)
    pbs = m * S + (GAP_PARITY if padded else 0)
    bufs = Bufs(rsmi)
    try:
        dptr, dbuf = bufs.full(nb * dbs, FILL_DATA, data_pinned)
        pptr, pbuf = bufs.full(nb * pbs, FILL_PARITY, parity_pinned)
        _rows(dbuf, nb, k, S, dbs)[:] = data
        prows = _rows(pbuf, nb, m, S, pbs)
        prows[:] = par
        want = np.zeros((nb, m), dtype=bool)
        for i, b in enumerate(hit):
            assert np.array_equal(orc.encode(k, m, data[b]), par[b]), b  # the SIMD oracle against the scalar one
            prows[b, i % m, (i * 211 + b) % S] ^= 1 << (i % 8)
            want[b, i % m] = True
        assert want.sum() == len(hit)
        assert np.array_equal((prows != par).any(axis=2), want)
        d0, p0 = dbuf.copy(), pbuf.copy()
        bad = np.full(nb * m, 0x5EED, dtype=np.uint32)
        with rsmi.Codec(k, m) as c:
            if zero_copy is not None:
                c.set_option("zero_copy", zero_copy)
            c.verify_batch_host_ptr(dptr, dbs, pptr, pbs, S, nb, bad.ctypes.data)
            assert c.last_kernel() == label, (name, c.last_kernel(), label)
        assert np.array_equal(dbuf, d0) and np.array_equal(pbuf, p0), name
        got = bad.reshape(nb, m) != 0
        assert np.array_equal(np.argwhere(got), np.argwhere(want)), (name, np.argwhere(got)[:16], np.argwhere(want))
        del prows, dbuf, pbuf
    finally:
        bufs.free()
        WALL[name] = time.perf_counter() - t0


ALIGNED_2_1 = "rs_verify_kernel<K=2,MT=1>"
WINDOW_2_1 = "rs_verify_kernel<K=2,MT=1>,UA"


# ---------------------------------------------------------------- 1-3: four chunks, every upload branch
@pytest.mark.gpu
@pytest.mark.parametrize("S,padded", [(S_2D, False), (S_2D, True), (S_LIN, True)],
                         ids=["2d-contiguous", "2d-per-block", "linear-per-block"])
def test_pipeline_four_chunks(gpu, S, padded):
    """RS(2,1), pageable, 3 * chunk + 2 blocks of rows of about 64 KiB: four chunks, the last of two
    blocks on staging stream 0 again.  S % 8 == 0 and contiguous blocks: one 2-D DMA per chunk
    and side; with block strides k * S + 24 and m * S + 40: one 2-D DMA per block; odd S with the
    same strides: one linear copy per block and rs_repitch_kernel."""
    k, m = 2, 1
    ch = chunk_blocks(k, m, S)
    nb = 3 * ch + 2
    assert nb * (k + m) * S > SMALL and not takes_one_kernel_path(1, False, False, nb * (k + m) * S)
    _verify_host(gpu, "four-chunks-%d%s" % (S, "-padded" if padded else ""), k, m, S, nb, seam_hits(nb, ch),
                 ALIGNED_2_1, padded=padded)


# ---------------------------------------------------------------- 4: the one-chunk pipeline
@pytest.mark.gpu
def test_pipeline_one_chunk(gpu):
    """nb <= chunk and above the small-call limit: ns = 1, one upload and one launch."""
    k, m, S, nb = 2, 1, S_2D, 100
    assert nb <= chunk_blocks(k, m, S) and nb * (k + m) * S > SMALL
    _verify_host(gpu, "one-chunk", k, m, S, nb, [0, 49, 50, nb - 1], ALIGNED_2_1)


# ---------------------------------------------------------------- 5: mixed memory
# (data page-locked, parity page-locked, blocks) -> the path the condition gives -> its label.
# S = 2049, RS(2,1): 100 blocks are 614700 bytes (2 * total <= 2 MiB), 250 blocks 1536750 bytes
# (total <= 2 MiB < 2 * total), 3000 blocks 18441000 bytes.  zero_copy is 1, the default.
MIXED = [
    # zd is set: total <= small is enough; the data rows are read in place, the parity is staged
    (True, False, 250, True, WINDOW_2_1),
    # well above the limit: `pinned` needs both, so the pipeline runs
    (True, False, 3000, False, ALIGNED_2_1),
    # zd is null and 2 * total > small: the pipeline, although total <= small
    (False, True, 250, False, ALIGNED_2_1),
    (False, True, 3000, False, ALIGNED_2_1),
    # zd is null and 2 * total <= small: the data is staged, the parity read in place
    (False, True, 100, True, WINDOW_2_1),
]


@pytest.mark.gpu
@pytest.mark.parametrize("data_pinned,parity_pinned,nb,one_kernel,label", MIXED,
                         ids=["data-locked-1.5M", "data-locked-18M", "parity-locked-1.5M", "parity-locked-18M",
                              "parity-locked-0.6M"])
def test_mixed_memory(gpu, data_pinned, parity_pinned, nb, one_kernel, label):
    """One side from rsmi_host_alloc, the other pageable, block strides with sentinel gaps.  The
    one-kernel path reads rows at pitch 2049 (",UA"); the pipeline stages them at pitch 4096."""
    k, m, S = 2, 1, S_ODD
    total = nb * (k + m) * S
    assert takes_one_kernel_path(1, data_pinned, parity_pinned, total) == one_kernel
    assert (label == WINDOW_2_1) == one_kernel
    assert nb <= chunk_blocks(k, m, S)
    _verify_host(gpu, "mixed-%d%d-%d" % (data_pinned, parity_pinned, nb), k, m, S, nb,
                 sorted({0, 1, nb // 2, nb - 2, nb - 1}), label, padded=True, data_pinned=data_pinned,
                 parity_pinned=parity_pinned)


# ---------------------------------------------------------------- 6: page-locked, zero_copy 0
@pytest.mark.gpu
def test_page_locked_copies(gpu):
    """Both buffers page-locked with zero_copy 0: the pipeline (no ",UA") with copies that really
    are asynchronous, three chunks on three streams."""
    k, m, S = 2, 1, S_ODD
    ch = chunk_blocks(k, m, S)
    nb = 2 * ch + 3
    assert not takes_one_kernel_path(0, True, True, nb * (k + m) * S)
    assert takes_one_kernel_path(1, True, True, nb * (k + m) * S)
    _verify_host(gpu, "page-locked-zero-copy-0", k, m, S, nb, seam_hits(nb, ch), ALIGNED_2_1, data_pinned=True,
                 parity_pinned=True, zero_copy=0)


# ---------------------------------------------------------------- 7: a 14-row shape through the pipeline
@pytest.mark.gpu
def test_pipeline_rs_10_4(gpu):
    """RS(10,4), S = 2056, pageable, contiguous, 3 * 1170 + 2 blocks: case 1's branch with ten
    data rows and four parity rows per block, the damage spread over the four parity rows."""
    k, m, S = 10, 4, S_2D_SMALL
    ch = chunk_blocks(k, m, S)
    nb = 3 * ch + 2
    _verify_host(gpu, "four-chunks-10-4", k, m, S, nb, seam_hits(nb, ch), "rs_verify_kernel<K=10,MT=4>")
