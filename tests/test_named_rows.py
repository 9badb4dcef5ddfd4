"""rsmi_crc_named_rows_dev on the GPU against the CPU references, exactly.

Every expected value comes from the row as stored:
  CRC-16  rsmi.crc16_entry(b"", raw, S) == oracle crc16_ibm(row)
  CRC-32  rsmi.crc32_entry(b"", raw, S) == zlib.crc32(row)
both bijections of raw at fixed S; rows of at most 2 KiB are also compared with the raw references
themselves (test_crc16.raw_crc; raw16 / raw32 of test_crc32_paths.py).  An entry that names nothing
gives 0.  The outputs lie between guard words and start as garbage, the row buffers come back byte
for byte, and each half is an allocation that ends at its last row's last byte.  No tolerances.

  1  the sizes, RS(10,4) and RS(4,2), three layouts, both folds, both checksums
  2  a sheet of entries in one call: every row, the seam, every kind of junk, a row named twice,
     slots 1, 2 and k+m, an all-empty array
  3  the eight kernels by label; either output alone
  4  many items per wave, mostly empty (waves_per_cu 1)
  5  stream order behind heal pair and heal, with no host sync: the second witness
  6  block strides past 2^32 on both halves
"""
import zlib

import numpy as np
import pytest

import oracle_lib as orc
from test_crc16 import raw_crc
from test_crc32_paths import raw16, raw32
from test_verify import stripes

NB = 3
GUARD = 8
POISON, GUARD_WORD = 0x7EA5, 0x6A6A
PAD = 0xD7  # every byte of a half that is not a row byte
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31
SIZES = [1, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 32767, 32768, 32769, 65537]
LABELS = {(16, 0): "rs_crc16_named_kernel", (16, 1): "rs_crc16_named_mfma_kernel",
          (32, 0): "rs_crc32_named_kernel", (32, 1): "rs_crc32_named_mfma_kernel"}


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    rsmi = pytest.importorskip("rsmi")
    if not torch.cuda.is_available() or rsmi.device_count() == 0:
        pytest.skip("no GPU")
    return torch, rsmi


def junk(n):
    """Every kind of entry that names nothing."""
    return [-1, -2, n, n + 1, I32_MAX, I32_MIN, -3, 1 << 16]


_REFS = {}


def row_refs(key, shards):
    """(crc16_ibm, zlib.crc32) of every row of shards (nb, n, S), computed once per key."""
    if key not in _REFS:
        nb, n, _ = shards.shape
        c16 = np.array([[orc.crc16_ibm(shards[b, r].tobytes()) for r in range(n)] for b in range(nb)], dtype=np.uint32)
        c32 = np.array([[zlib.crc32(shards[b, r].tobytes()) for r in range(n)] for b in range(nb)], dtype=np.uint32)
        _REFS[key] = (c16, c32)
    return _REFS[key]


def refs_of(shards):
    """row_refs of rows that are not kept."""
    return (np.array([[orc.crc16_ibm(r.tobytes()) for r in blk] for blk in shards], dtype=np.uint32),
            np.array([[zlib.crc32(r.tobytes()) for r in blk] for blk in shards], dtype=np.uint32))


def assert_named(rsmi, shards, entries, got16, got32, refs, ctx):
    """got16 / got32 (nb, slots) uint32 or None against the rows entries (nb, slots) names."""
    nb, n, S = shards.shape
    c16, c32 = refs
    for b in range(nb):
        for s, e in enumerate(entries[b]):
            e = int(e)
            named = 0 <= e < n
            for bits, got, want in ((16, got16, c16), (32, got32, c32)):
                if got is None:
                    continue
                raw = int(got[b, s])
                if not named:
                    assert raw == 0, (ctx, bits, b, s, e, hex(raw))
                    continue
                if bits == 16:
                    assert raw >> 16 == 0, (ctx, b, s, hex(raw))
                    fin = rsmi.crc16_entry(b"", raw, S)
                else:
                    fin = rsmi.crc32_entry(b"", raw, S)
                assert fin == int(want[b, e]), (ctx, bits, b, s, e, hex(fin), hex(int(want[b, e])))
                if S <= 2048:
                    row = shards[b, e].tobytes()
                    if bits == 16:
                        assert raw == raw_crc(row) == raw16(row), (ctx, b, s, e)
                    else:
                        assert raw == raw32(row), (ctx, b, s, e)


class Outputs:
    """The device outputs, pre-filled with garbage (the call must zero what it accumulates into),
    each between guard words."""

    def __init__(self, torch, words, want16=True, want32=True):
        self.words = words
        self.t = [torch.full((2 * GUARD + words,), POISON, dtype=torch.int32, device="cuda") if w else None
                  for w in (want16, want32)]
        for t in self.t:
            if t is not None:
                t[:GUARD] = GUARD_WORD
                t[-GUARD:] = GUARD_WORD

    def ptr(self, i):
        return self.t[i].data_ptr() + 4 * GUARD if self.t[i] is not None else 0

    def read(self, shape):
        out = []
        for t in self.t:
            if t is None:
                out.append(None)
                continue
            a = t.cpu().numpy()
            assert (a[:GUARD] == GUARD_WORD).all() and (a[-GUARD:] == GUARD_WORD).all(), "a guard word was written"
            out.append(a[GUARD:-GUARD].astype(np.uint32).reshape(shape))
        return out


class Halves:
    """Data and parity rows in two allocations, each with its own byte phase, pitch and block stride
    (geo: d_off, d_rs, d_bs, p_off, p_rs, p_bs), each ending at its last row's last byte."""

    def __init__(self, torch, shards, k, geo):
        nb, n, S = shards.shape
        self.nb, self.n, self.k, self.S, self.geo = nb, n, k, S, geo
        d_off, d_rs, d_bs, p_off, p_rs, p_bs = geo
        m = n - k
        assert d_rs >= S and p_rs >= S and (nb == 1 or (d_bs >= k * d_rs and p_bs >= m * p_rs))
        self.hd = np.full(d_off + (nb - 1) * d_bs + (k - 1) * d_rs + S, PAD, dtype=np.uint8)
        self.hp = np.full(p_off + (nb - 1) * p_bs + (m - 1) * p_rs + S, PAD, dtype=np.uint8)
        np.lib.stride_tricks.as_strided(self.hd[d_off:], shape=(nb, k, S), strides=(d_bs, d_rs, 1))[:] = shards[:, :k]
        np.lib.stride_tricks.as_strided(self.hp[p_off:], shape=(nb, m, S), strides=(p_bs, p_rs, 1))[:] = shards[:, k:]
        self.dd, self.dp = torch.from_numpy(self.hd.copy()).cuda(), torch.from_numpy(self.hp.copy()).cuda()
        assert self.dd.data_ptr() % 256 == 0 and self.dp.data_ptr() % 256 == 0
        self.aligned = all(x % 16 == 0 for x in geo)

    def call(self, c, d_rows, slots, out, stream):
        d_off, d_rs, d_bs, p_off, p_rs, p_bs = self.geo
        c.crc_named_rows_dev(self.dd.data_ptr() + d_off, d_rs, d_bs, self.dp.data_ptr() + p_off, p_rs, p_bs, self.S,
                             self.nb, d_rows, slots, out.ptr(0), out.ptr(1), stream)

    def unchanged(self):
        return np.array_equal(self.dd.cpu().numpy(), self.hd) and np.array_equal(self.dp.cpu().numpy(), self.hp)


def geometry(rsmi, k, m, S, layout):
    """aligned: rows at recommended_pitch from aligned bases; ua: rows back to back at pitch S from
    an odd base, so every misalignment occurs; halves: each half its own phase, pitch and stride."""
    if layout == "aligned":
        rs = rsmi.recommended_pitch(S)
        return (0, rs, k * rs + 48, 256, rs, m * rs + 16)
    if layout == "ua":
        return (3, S, k * S, 5, S, m * S)
    rs = rsmi.recommended_pitch(S)
    return (16, rs, k * rs + 32, 7, S + 3, m * (S + 3) + 11)


def run(torch, rsmi, c, shards, k, geo, entries, refs, ctx, want16=True, want32=True, label=None):
    entries = np.asarray(entries, dtype=np.int64)
    nb, slots = entries.shape
    assert nb == shards.shape[0]
    h = Halves(torch, shards, k, geo)
    d_rows = torch.from_numpy(entries.astype(np.int32)).cuda()
    out = Outputs(torch, nb * slots, want16, want32)
    torch.cuda.synchronize()
    h.call(c, d_rows.data_ptr(), slots, out, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    if label is not None:
        assert c.last_kernel() == label, (ctx, c.last_kernel(), label)
    assert h.unchanged(), ("the call wrote to a row buffer", ctx)
    assert np.array_equal(d_rows.cpu().numpy(), entries.astype(np.int32)), ("the call wrote to d_rows", ctx)
    got16, got32 = out.read((nb, slots))
    assert_named(rsmi, shards, entries, got16, got32, refs, ctx)
    return got16, got32


def set_folds(c, fold):
    c.set_option("crc16_fold", fold)
    c.set_option("crc32_fold", fold)


def last_label(fold, aligned):
    """A call with both outputs launches the CRC-32 pass last."""
    return LABELS[(32, fold)] + ("" if aligned else ",UA")


# ---------------------------------------------------------------- 1: the sizes
@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["aligned", "ua", "halves"])
@pytest.mark.parametrize("k,m", [(10, 4), (4, 2)])
def test_sizes(gpu, k, m, layout):
    """The tile (1 KiB), the pipelined half group (4 KiB), the group (8 KiB), the 32-tile item
    (32 KiB: two items per row) and the CRC-16's order 32767 (the end shift's exponent wraps), each
    with its neighbours; the smallest rows.  Two slots: the seam (k-1 and k), the first and last
    rows, a row named twice and an entry that names nothing."""
    torch, rsmi = gpu
    n = k + m
    entries = [[k - 1, k], [-1, 0], [n - 1, n - 1]]
    with rsmi.Codec(k, m) as c:
        for S in SIZES:
            full = stripes(k, m, S)
            refs = row_refs((k, m, S, NB), full)
            geo = geometry(rsmi, k, m, S, layout)
            for fold in (1, 0):
                set_folds(c, fold)
                run(torch, rsmi, c, full, k, geo, entries, refs, (k, m, S, layout, fold),
                    label=last_label(fold, layout == "aligned"))


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", [(10, 4), (4, 2)])
def test_alignment_predicate(gpu, k, m):
    """The aligned kernels need both bases, both pitches and both block strides on the 16-byte grid.
    All six hold: the aligned label.  Each broken alone: the UA label.  The answers are the same."""
    torch, rsmi = gpu
    S, n = 1025, k + m
    full = stripes(k, m, S)
    refs = row_refs((k, m, S, NB), full)
    up = lambda x: (x + 15) // 16 * 16
    base = (0, 1088, k * 1088 + 64, 0, 1056, m * 1056 + 32)
    cases = [
        (base, True),
        ((5,) + base[1:], False),                                                # data base
        (base[:3] + (9,) + base[4:], False),                                     # parity base
        ((0, 1089, up(k * 1089)) + base[3:], False),                             # data pitch
        ((0, 1088, k * 1088 + 72) + base[3:], False),                            # data block stride
        (base[:3] + (0, 1057, up(m * 1057)), False),                             # parity pitch
        (base[:3] + (0, 1056, m * 1056 + 36), False),                            # parity block stride
    ]
    entries = [[0, n - 1], [k, k - 1], [1, -2]]
    with rsmi.Codec(k, m) as c:
        for fold in (1, 0):
            set_folds(c, fold)
            for geo, aligned in cases:
                assert sum(1 for x in geo if x % 16) == (0 if aligned else 1), geo
                run(torch, rsmi, c, full, k, geo, entries, refs, (k, m, geo, fold), label=last_label(fold, aligned))


# ---------------------------------------------------------------- 2: a sheet of entries
def sheet(k, m, slots):
    """Block b < n names row b in slot b % slots, junk in the other slots; then a block of junk
    alone per kind of junk; a block naming one row in two slots; a block whose first and last slots
    name the seam; a block naming rows 0 .. slots-1 in reverse."""
    n = k + m
    J = junk(n)
    rows = []
    for b in range(n):
        e = [J[(b + s) % len(J)] for s in range(slots)]
        e[b % slots] = b
        rows.append(e)
    for j in range(len(J)):
        rows.append([J[(j + s) % len(J)] for s in range(slots)])
    if slots >= 2:
        rows.append([k] * 2 + [J[s % len(J)] for s in range(slots - 2)])
        rows.append([k - 1] + [J[(3 + s) % len(J)] for s in range(slots - 2)] + [k])
    rows.append(list(range(slots - 1, -1, -1)))
    return np.array(rows, dtype=np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["aligned", "ua", "halves"])
@pytest.mark.parametrize("k,m", [(10, 4), (4, 2)])
def test_entry_sheet(gpu, k, m, layout):
    torch, rsmi = gpu
    n = k + m
    with rsmi.Codec(k, m) as c:
        for S in (17, 4097, 32769):
            for slots in (1, 2, n):
                entries = sheet(k, m, slots)
                assert set(range(n)) <= set(entries.reshape(-1).tolist())
                assert {-1, -2, n, I32_MAX, I32_MIN} <= set(entries.reshape(-1).tolist())
                nb = len(entries)
                full = stripes(k, m, S, nb)
                refs = row_refs((k, m, S, nb), full)
                geo = geometry(rsmi, k, m, S, layout)
                for fold in (1, 0):
                    set_folds(c, fold)
                    run(torch, rsmi, c, full, k, geo, entries, refs, (k, m, S, layout, slots, fold))
                # nothing named at all: zeros, and nothing read
                empty = np.array([[junk(n)[(b + s) % 8] for s in range(slots)] for b in range(nb)])
                g16, g32 = run(torch, rsmi, c, full, k, geo, empty, refs, (k, m, S, layout, slots, "empty"))
                assert not g16.any() and not g32.any()


# ---------------------------------------------------------------- 3: the eight kernels; one output
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "ua"])
@pytest.mark.parametrize("fold", [1, 0], ids=["mfma", "nibble"])
@pytest.mark.parametrize("bits", [16, 32])
def test_labels_and_single_outputs(gpu, bits, fold, aligned):
    """Each of the eight kernels is reached through its fold option and the layout, with the other
    output NULL: the label is that kernel's, and the other fold option does not matter."""
    torch, rsmi = gpu
    k, m, S = 10, 4, 8193
    full = stripes(k, m, S)
    refs = row_refs((k, m, S, NB), full)
    geo = geometry(rsmi, k, m, S, "aligned" if aligned else "ua")
    entries = [[3, -1], [k, k + 3], [-2, 9]]
    with rsmi.Codec(k, m) as c:
        c.set_option("crc16_fold", fold if bits == 16 else 1 - fold)
        c.set_option("crc32_fold", fold if bits == 32 else 1 - fold)
        got = run(torch, rsmi, c, full, k, geo, entries, refs, (bits, fold, aligned), want16=bits == 16,
                  want32=bits == 32, label=LABELS[(bits, fold)] + ("" if aligned else ",UA"))
        assert (got[0] is None) == (bits == 32) and (got[1] is None) == (bits == 16)


# ---------------------------------------------------------------- 4: many items per wave
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "ua"])
def test_many_items_per_wave_mostly_empty(gpu, aligned):
    """waves_per_cu 1 and several times more entries than the grid has waves, each of two items
    (S = 40 000): every wave walks many entries.  Most name nothing; the named ones are clustered at
    the end and sprinkled singly, so waves meet runs of empty items before, between and after named
    ones, and most waves meet no named item at all.  The prefetch of the pipelined pass must step
    over the empty ones.  The blocks overlap (a block stride of 16 or 7 bytes: the call puts no
    bound on it), so a few hundred KB hold them, and the buffer ends at the last row's last byte."""
    torch, rsmi = gpu
    k, m, S, slots = 4, 2, 40000, 2
    n = k + m
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    nb = 3 * cu + 5          # 2 nb entries of 2 items each; at most cu waves
    rs, bs, off = (rsmi.recommended_pitch(S), 16, 0) if aligned else (S, 7, 3)
    rng = np.random.default_rng(77)
    host = rng.integers(0, 256, size=off + (nb - 1) * bs + (n - 1) * rs + S, dtype=np.uint8)
    shards = np.lib.stride_tricks.as_strided(host[off:], shape=(nb, n, S), strides=(bs, rs, 1))
    J = junk(n)
    entries = np.array([[J[(b + s) % len(J)] for s in range(slots)] for b in range(nb)], dtype=np.int64)
    entries[nb - 6:, :] = rng.integers(0, n, size=(6, slots))
    for b in (0, 1, cu, 2 * cu + 1):
        entries[b, b % slots] = rng.integers(0, n)
    c16, c32 = np.zeros((nb, n), dtype=np.uint32), np.zeros((nb, n), dtype=np.uint32)
    for b, r in {(b, int(e)) for b in range(nb) for e in entries[b] if 0 <= e < n}:
        c16[b, r], c32[b, r] = orc.crc16_ibm(shards[b, r].tobytes()), zlib.crc32(shards[b, r].tobytes())
    d = torch.from_numpy(host.copy()).cuda()
    d_rows = torch.from_numpy(entries.astype(np.int32)).cuda()
    base = d.data_ptr() + off
    with rsmi.Codec(k, m) as c:
        c.set_option("waves_per_cu", 1)
        for fold in (1, 0):
            set_folds(c, fold)
            out = Outputs(torch, nb * slots)
            c.crc_named_rows_dev(base, rs, bs, base + k * rs, rs, bs, S, nb, d_rows.data_ptr(), slots, out.ptr(0),
                                 out.ptr(1), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert c.last_kernel() == last_label(fold, aligned)
            r16, r32 = out.read((nb, slots))
            assert_named(rsmi, shards, entries, r16, r32, (c16, c32), ("wpc1", aligned, fold))
        assert np.array_equal(d.cpu().numpy(), host)


# ---------------------------------------------------------------- 5: stream order, the second witness
def _lay(rsmi, k, m, S, aligned):
    rs = rsmi.recommended_pitch(S) if aligned else S
    off = 0 if aligned else 3
    return off, rs, (k + m) * rs


def _gated_heal_then_named(torch, rsmi, k, m, S, aligned, dirty, slots, want_verdicts):
    """Behind a delay on a side stream, with no host sync in between: the damaged stripes arrive,
    heal (pair) runs, the named rows pass consumes its verdict array.  Returns (verdicts, raw16,
    raw32, the rows after)."""
    from test_stream_order import Gate
    gate = Gate(torch)
    nb, n = dirty.shape[0], k + m
    off, rs, bs = _lay(rsmi, k, m, S, aligned)
    host = np.full(off + nb * bs, PAD, dtype=np.uint8)
    rows = np.lib.stride_tricks.as_strided(host[off:], shape=(nb, n, S), strides=(bs, rs, 1))
    rows[:] = dirty
    pinned = torch.from_numpy(host).pin_memory()
    st = torch.cuda.Stream()
    with rsmi.Codec(k, m) as c:
        for gated in (False, True):  # the first pass builds the plans, the tables and the scratch
            d = torch.full((host.size,), 0xEE, dtype=torch.uint8, device="cuda")
            verdict = torch.full((nb * slots,), 0x0BAD, dtype=torch.int32, device="cuda")
            out = Outputs(torch, nb * slots)
            torch.cuda.synchronize()
            e1, e2 = torch.cuda.Event(), torch.cuda.Event()
            with torch.cuda.stream(st):
                if gated:
                    gate()
                e1.record()
                d.copy_(pinned, non_blocking=True)
                base = d.data_ptr() + off
                args = (base, rs, bs, base + k * rs, rs, bs, S, nb)
                if slots == 2:
                    c.heal_pair_batch_dev(*args, verdict.data_ptr(), 0, st.cuda_stream)
                else:
                    c.heal_batch_dev(*args, verdict.data_ptr(), 0, st.cuda_stream)
                c.crc_named_rows_dev(*args, verdict.data_ptr(), slots, out.ptr(0), out.ptr(1), st.cuda_stream)
                kept = verdict.clone()
                verdict.fill_(-1)  # behind the pass on the stream: a pass that ran late names nothing
                e2.record()
            if gated:
                assert not e1.query(), "a call waited for the stream"
            e2.synchronize()
            assert c.last_kernel().startswith("rs_crc32_named"), c.last_kernel()
            got = kept.cpu().numpy().reshape(nb, slots)
            assert got.tolist() == want_verdicts, (gated, got.tolist())
            r16, r32 = out.read((nb, slots))
            after = d.cpu().numpy()
            healed = np.lib.stride_tricks.as_strided(after[off:], shape=(nb, n, S), strides=(bs, rs, 1)).copy()
            assert_named(rsmi, healed, got, r16, r32, refs_of(healed), ("stream order", aligned, slots, gated))
    return got, r16, r32, healed


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "ua"])
def test_stream_order_behind_heal_pair(gpu, aligned):
    """RS(10,4), S = 4097: singles, pairs, a clean block and a block of three damaged shards
    (-2, -2).  The raws are those of the original rows -- the second witness passes -- and clean and
    unknown blocks give zeros."""
    torch, rsmi = gpu
    k, m, S, nb = 10, 4, 4097, 6
    full = stripes(k, m, S, nb)
    sh = full.copy()
    sh[0, 4, 4096] ^= 0x01; sh[0, 9, 3] ^= 0x10                               # a pair of data shards
    sh[1, 0, 1] ^= 0x01; sh[1, 6, 1000] ^= 0x02; sh[1, k + 3, 4096] ^= 0x03     # three: unknown
    sh[2, k + 3, 0] ^= 0x80                                                   # a single parity shard
    sh[4, k - 1, 1024] ^= 0x02; sh[4, k, 4095] ^= 0x02                        # the seam
    sh[5, 2, 4096] ^= 0x40                                                    # a single data shard
    want = [[4, 9], [-2, -2], [k + 3, -1], [-1, -1], [k - 1, k], [2, -1]]
    got, r16, r32, healed = _gated_heal_then_named(torch, rsmi, k, m, S, aligned, sh, 2, want)
    assert np.array_equal(healed[[0, 2, 3, 4, 5]], full[[0, 2, 3, 4, 5]]) and np.array_equal(healed[1], sh[1])
    c16, c32 = row_refs((k, m, S, nb), full)
    for b, pair in enumerate(want):
        for s, r in enumerate(pair):
            if r >= 0:   # the witness: R(healed row) finishes to the checksum kept from the write
                assert rsmi.crc16_entry(b"", int(r16[b, s]), S) == c16[b, r]
                assert rsmi.crc32_entry(b"", int(r32[b, s]), S) == c32[b, r]
            else:
                assert r16[b, s] == 0 and r32[b, s] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "ua"])
def test_stream_order_behind_heal(gpu, aligned):
    """rsmi_heal_batch_dev's culprits with slots = 1."""
    torch, rsmi = gpu
    k, m, S, nb = 10, 4, 4097, 4
    full = stripes(k, m, S, nb)
    sh = full.copy()
    sh[0, k, 4096] ^= 0x01
    sh[2, 7, 0] ^= 0x80
    sh[3, 0, 5] ^= 0x01; sh[3, 1, 6] ^= 0x01                                  # two shards: unknown to heal
    want = [[k], [-1], [7], [-2]]
    got, r16, r32, healed = _gated_heal_then_named(torch, rsmi, k, m, S, aligned, sh, 1, want)
    assert np.array_equal(healed[:3], full[:3]) and np.array_equal(healed[3], sh[3])
    c16, c32 = row_refs((k, m, S, nb), full)
    assert rsmi.crc16_entry(b"", int(r16[0, 0]), S) == c16[0, k] and rsmi.crc32_entry(b"", int(r32[2, 0]), S) == c32[2, 7]
    assert r16[1, 0] == r16[3, 0] == 0 and r32[1, 0] == r32[3, 0] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "ua"])
def test_witness_catches_the_imitated_pair(gpu, aligned):
    """test_heal_pair.py's imitation at RS(4,4): errors in three shards that imitate a pair are
    healed to a clean codeword that is not the original.  The checksums of the two rewritten rows
    are those of the bytes now stored, and differ from the originals': the witness catches it."""
    torch, rsmi = gpu
    from test_locate_pair import imitation_rs44
    k, m, three, pair, lam = imitation_rs44()
    mul = orc.lib().rs_oracle_gal_mul
    S, nb = 1040, 3
    full = stripes(k, m, S, nb)
    sh = full.copy()
    for b, (e, pos) in enumerate([(0x01, 7), (0xC3, 1033)]):
        sh[b, three[0], pos] ^= mul(lam[0], e)
        sh[b, three[1], pos] ^= mul(lam[1], e)
        sh[b, three[2], pos] ^= e
    want = [list(pair), list(pair), [-1, -1]]
    got, r16, r32, healed = _gated_heal_then_named(torch, rsmi, k, m, S, aligned, sh, 2, want)
    c16, c32 = row_refs((k, m, S, nb), full)
    for b in (0, 1):
        for s, r in enumerate(pair):
            assert not np.array_equal(healed[b, r], full[b, r])
            assert rsmi.crc16_entry(b"", int(r16[b, s]), S) != c16[b, r], (b, r)
            assert rsmi.crc32_entry(b"", int(r32[b, s]), S) != c32[b, r], (b, r)


# ---------------------------------------------------------------- 6: offsets past 4 GiB
@pytest.mark.gpu
def test_offsets_past_4gib(gpu):
    """Two blocks at block_stride = 2^32 + 256 on both halves, aligned and shifted by one byte; the
    rows written one by one into allocations that are otherwise not filled.  A truncated offset
    reads the near block or bytes no row was written to."""
    torch, rsmi = gpu
    if torch.cuda.mem_get_info()[0] < 12 << 30:
        pytest.skip("needs 12 GiB of free device memory")
    k, m, nb, S, bs = 4, 2, 2, 1040, 2 ** 32 + 256
    n = k + m
    try:
        with rsmi.Codec(k, m) as c:
            dd = torch.empty(2 ** 32 + 2 ** 20, dtype=torch.uint8, device="cuda")
            dp = torch.empty(2 ** 32 + 2 ** 20, dtype=torch.uint8, device="cuda")
            assert 1 + bs + k * S <= dd.numel()
            for off, aligned in ((0, True), (1, False)):
                sh = np.random.default_rng(6001 + off).integers(0, 256, size=(nb, n, S), dtype=np.uint8)
                for b in range(nb):
                    for i in range(k):
                        o = off + b * bs + i * S
                        dd[o:o + S].copy_(torch.from_numpy(sh[b, i]))
                    for j in range(m):
                        o = off + b * bs + j * S
                        dp[o:o + S].copy_(torch.from_numpy(sh[b, k + j]))
                entries = np.array([[0, k, -1], [k - 1, n - 1, 1]], dtype=np.int32)
                d_rows = torch.from_numpy(entries).cuda()
                out = Outputs(torch, nb * 3)
                c.crc_named_rows_dev(dd.data_ptr() + off, S, bs, dp.data_ptr() + off, S, bs, S, nb, d_rows.data_ptr(), 3,
                                     out.ptr(0), out.ptr(1), torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                assert c.last_kernel() == last_label(1, aligned), c.last_kernel()
                r16, r32 = out.read((nb, 3))
                assert_named(rsmi, sh, entries, r16, r32, refs_of(sh), ("far", off))
            del dd, dp
    finally:
        torch.cuda.empty_cache()
