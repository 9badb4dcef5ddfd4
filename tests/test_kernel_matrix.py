"""Every instantiated coding kernel against the CPU oracle, bit for bit.

The hot path is a matrix of compile-time instantiations: rs_fast_kernel and rs_fused_mfma_kernel
for K in KS x MT in 1..4, each in six layout / CRC forms (fn, ua, crc, ua_crc, fused, fused_ua),
the in-kernel-combine forms (INL), and the table-of-bases forms (TB).  Each (K, MT) pair is its
own unrolled code, which no other shape executes: this module runs every one of them, proves by
the launch label (rsmi_last_kernel) that the instantiation was reached, and compares parity,
rebuilt rows and R(row) with oracle_lib.  Shapes without an instantiation must fall to
rs_generic_kernel (and, with CRC, to the separate pass), whose two grid-stride loops run a second
iteration here.  Leg 0 keeps the tables below equal to the dispatch table in rs_kernels.hip and
rs_kernels_tb.hip.

Everything is bit-exact: there are no tolerances.
"""
import ctypes
import os
import re
import threading
import time

import numpy as np
import pytest

import oracle_lib as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "filedag-storage_amd", "csrc")
KERNELS_HIP = os.path.join(CSRC, "rs_kernels.hip")        # fill_k, fill_km, fill_inl
KERNELS_TB_HIP = os.path.join(CSRC, "rs_kernels_tb.hip")  # fill_tb_k, fill_tb_km, fill_tb_fused, fill_tb_fused_inl

# ---------------------------------------------------------------- the dispatch table, restated
KS = [1, 2, 3, 4, 5, 6, 8, 10, 12, 16]                      # fill_k<K>: six forms for MT = 1..4
MTS = [1, 2, 3, 4]                                          # fill_km<K, MT> inside fill_k
INL_SHAPES = [(2, 1), (4, 2), (10, 4), (16, 4)]             # fill_inl<K, MT>
TB_KS = [2, 4, 10, 16]                                      # fill_tb_k<K>: fn_tb / ua_tb for MT = 1..4
TB_FUSED_SHAPES = [(2, 1), (4, 2), (10, 4), (16, 4)]        # fill_tb_fused<K, MT>: four forms each
TB_FUSED_INL_SHAPES = [(4, 1), (10, 1), (10, 2), (10, 3), (16, 1), (16, 2), (16, 3)]  # fill_tb_fused_inl
GENERIC_SHAPES = [(7, 2), (9, 4), (11, 1), (13, 3), (14, 4), (15, 2)]  # K without an instantiation

NB = 3


def nt_of(K, MT):
    """stores are nontemporal (NT=1) unless the tile reads at least 4 rows per row
    written (NT=2).  Stated here on purpose, not imported from the library."""
    return 2 if K >= 4 * MT else 1


def fast_label(K, MT, ua=False, crc=False, tb=False):
    return ("rs_fast_kernel<K=%d,MT=%d,NT=%d>" % (K, MT, nt_of(K, MT)) + (",UA" if ua else "") +
            (",CRC" if crc else "") + (",TB" if tb else ""))


def fused_units(S):
    """4-tile units of a row: ceil(ceil(ceil(S/16)/64)/4)."""
    return (((S + 15) // 16 + 63) // 64 + 3) // 4


def fused_label(K, MT, S, nb, ua=False, tb=False):
    inl = (K, MT) in INL_SHAPES and nb * fused_units(S) <= 64
    return ("rs_fused_mfma_kernel<K=%d,MT=%d,NT=%d>" % (K, MT, nt_of(K, MT)) + (",UA" if ua else "") +
            (",INL" if inl else "") + (",TB" if tb else ""))


def generic_label(K, MT):
    return "rs_generic_kernel<K=%d,MT=%d>" % (K, MT)


# every instantiation a test of this module ran and asserted by its exact label
SEEN = set()
WALL = {}


def seen_label(kern):
    """Files an asserted label under its family of the dispatch table (FastKernelTable)."""
    m = re.match(r"(rs_\w+)<K=(\d+),MT=(\d+)(?:,NT=\d+)?>(.*)$", kern)
    name, K, MT, sfx = m.group(1), int(m.group(2)), int(m.group(3)), m.group(4).split(",")[1:]
    ua, crc, inl, tb = ("UA" in sfx), ("CRC" in sfx), ("INL" in sfx), ("TB" in sfx)
    if name == "rs_generic_kernel":
        SEEN.add(("generic",))
    elif name == "rs_fast_kernel":
        fam = ("ua_tb" if ua else "fn_tb") if tb else ("ua_crc" if ua else "crc") if crc else ("ua" if ua else "fn")
        SEEN.add((fam, K, MT))
    elif tb:
        SEEN.add(("fused_tb", K, MT, ua, inl))
    elif inl:
        SEEN.add(("inl", K, MT, ua))
    else:
        SEEN.add(("fused_ua" if ua else "fused", K, MT))


# ---------------------------------------------------------------- leg 0: the tables match the source
def _calls(src, name, nargs):
    pat = r"\b%s<\s*%s\s*>\s*\(" % (name, r"\s*,\s*".join([r"(\d+)"] * nargs))
    out = [tuple(int(x) for x in g) if nargs > 1 else int(g) for g in re.findall(pat, src)]
    return out


def test_tables_match_source():
    """The module's tables equal the arguments of fill_k / fill_inl / fill_tb_k / fill_tb_fused /
    fill_tb_fused_inl in rs_kernels.hip (the table-less forms) and rs_kernels_tb.hip (the
    table-of-bases forms): an instantiation added without extending this sweep fails the CPU suite."""
    with open(KERNELS_HIP) as f:
        src = f.read()
    with open(KERNELS_TB_HIP) as f:
        src_tb = f.read()
    assert _calls(src, "fill_k", 1) == KS
    assert _calls(src, "fill_inl", 2) == INL_SHAPES
    assert _calls(src_tb, "fill_tb_k", 1) == TB_KS
    assert _calls(src_tb, "fill_tb_fused", 2) == TB_FUSED_SHAPES
    assert _calls(src_tb, "fill_tb_fused_inl", 2) == TB_FUSED_INL_SHAPES
    # the table-of-bases forms are filled in their own unit only
    assert not re.search(r"\bfill_tb_\w+<", src)
    # fill_k and fill_tb_k expand to MT = 1..4 (the templates' K stays symbolic in the source)
    assert re.findall(r"\bfill_km<K,\s*(\d+)>\(", src) == [str(m) for m in MTS]
    assert re.findall(r"\bfill_tb_km<K,\s*(\d+)>\(", src_tb) == [str(m) for m in MTS]
    assert not set(k for k, _ in GENERIC_SHAPES) & set(KS)
    assert sorted(set(KS) | set(k for k, _ in GENERIC_SHAPES)) == list(range(1, 17))
    assert set(TB_KS) <= set(KS) and all(k in TB_KS for k, _ in TB_FUSED_SHAPES + TB_FUSED_INL_SHAPES)


def expected_counts():
    """Instantiations per family, from the tables leg 0 pins to the source."""
    pairs = len(KS) * len(MTS)
    return {"fn": pairs, "ua": pairs, "crc": pairs, "ua_crc": pairs, "fused": pairs, "fused_ua": pairs,
            "inl": 2 * len(INL_SHAPES), "fn_tb": len(TB_KS) * len(MTS), "ua_tb": len(TB_KS) * len(MTS),
            "fused_tb": 4 * len(TB_FUSED_SHAPES) + 2 * len(TB_FUSED_INL_SHAPES), "generic": 1}


def test_expected_counts():
    c = expected_counts()
    assert sum(c.values()) == 6 * 40 + 8 + 32 + 30 + 1 == 311


# ---------------------------------------------------------------- GPU plumbing
@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    rsmi = pytest.importorskip("rsmi")
    if not torch.cuda.is_available() or rsmi.device_count() == 0:
        pytest.skip("no GPU")
    yield torch, rsmi
    got = {}
    for e in SEEN:
        got[e[0]] = got.get(e[0], 0) + 1
    print("\nkernel matrix: instantiations run and asserted by label (of expected):",
          ", ".join("%s %d/%d" % (f, got.get(f, 0), e) for f, e in expected_counts().items()))
    print("kernel matrix: wall seconds per leg:", ", ".join("%s %.2f" % kv for kv in sorted(WALL.items())))


class _leg:
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.t0 = time.perf_counter()

    def __exit__(self, *a):
        WALL[self.name] = WALL.get(self.name, 0.0) + time.perf_counter() - self.t0


class Layout:
    """nb blocks of n rows of S bytes in one byte buffer with guard bytes all around.
    aligned: rows at rsmi_recommended_pitch(S) from offset 0 (padding at and past S in each row);
    unaligned window: rows back to back at pitch S + 3 from a base offset of 7."""

    def __init__(self, rsmi, n, S, nb, ua, off=None, rs=None):
        self.n, self.S, self.nb, self.ua = n, S, nb, ua
        self.rs = rs if rs is not None else (S + 3 if ua else rsmi.recommended_pitch(S))
        self.off = off if off is not None else (7 if ua else 0)
        self.bs = n * self.rs
        self.size = self.off + nb * self.bs + 32

    def buffer(self, fill):
        return np.full(self.size, fill, dtype=np.uint8)

    def rows(self, host):
        return np.lib.stride_tricks.as_strided(host[self.off:], shape=(self.nb, self.n, self.S),
                                               strides=(self.bs, self.rs, 1))


def _data(rng, K, S, nb, kind="random"):
    if kind == "ramp":  # row c holds all 256 byte values: every entry of every lookup table is read
        x = np.arange(S, dtype=np.int64)
        rows = np.stack([((x * (2 * c + 1) + c) & 0xFF).astype(np.uint8) for c in range(K)])
        return np.ascontiguousarray(np.broadcast_to(rows, (nb, K, S)))
    if kind == "ones":
        return np.full((nb, K, S), 0xFF, dtype=np.uint8)
    return rng.integers(0, 256, size=(nb, K, S), dtype=np.uint8)


def _full(K, MT, data):
    return np.concatenate([data, orc.encode_fast(K, MT, data, threads=4)], axis=1)


def _loss(rng, K, MT):
    """MT of the K + MT rows; with K >= 2 and MT >= 2 at least one data and one parity row."""
    n = K + MT
    if K >= 2 and MT >= 2:
        lost = {int(rng.integers(0, K)), K + int(rng.integers(0, MT))}
        rest = [i for i in range(n) if i not in lost]
        lost |= set(int(x) for x in rng.choice(rest, size=MT - 2, replace=False))
    else:
        lost = set(int(x) for x in rng.choice(n, size=MT, replace=False))
    assert len(lost) == MT
    return sorted(lost)


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _encode_then_rebuild(torch, rsmi, c, K, MT, S, ua, data, rng, enc_label, rec_label):
    """encode_batch_dev into a guarded buffer, then lose MT rows and rebuild them in place
    (reconstruct_batch_dev, data_only=False): the same (K, MT) instantiation with a decode matrix,
    a non-identity in_row, and output rows interleaved with input rows.  The whole buffer is
    compared each time: no guard or padding byte may change."""
    n = K + MT
    lay = Layout(rsmi, n, S, NB, ua)
    host = lay.buffer(0x5A)
    lay.rows(host)[:, :K] = data
    d = torch.from_numpy(host.copy()).cuda()
    base = d.data_ptr() + lay.off
    c.encode_batch_dev(base, lay.rs, lay.bs, base + K * lay.rs, lay.rs, lay.bs, S, NB, _stream(torch))
    torch.cuda.synchronize()
    assert c.last_kernel() == enc_label, (c.last_kernel(), enc_label, S)
    full = _full(K, MT, data)
    expect = host.copy()
    lay.rows(expect)[:] = full
    got = d.cpu().numpy()
    if not ua:  # stated on its own: padding at and past S in the parity rows is still 0x5A
        g = got[:NB * lay.bs].reshape(NB, n, lay.rs)
        assert (g[:, K:, S:] == 0x5A).all(), (K, MT, S)
    assert np.array_equal(got, expect), (K, MT, S, ua, "encode")

    lost = _loss(rng, K, MT)
    present = [i not in lost for i in range(n)]
    erased = expect.copy()
    lay.rows(erased)[:, lost] = 0xEE
    d.copy_(torch.from_numpy(erased))
    c.reconstruct_batch_dev(base, lay.rs, lay.bs, S, NB, present, False, _stream(torch))
    torch.cuda.synchronize()
    assert c.last_kernel() == rec_label, (c.last_kernel(), rec_label, S, lost)
    rebuilt = erased.copy()
    for b in range(NB):
        rc, sh = orc.reconstruct(K, MT, np.ascontiguousarray(lay.rows(erased)[b]), present, False)
        assert rc == 0
        lay.rows(rebuilt)[b] = sh
    assert np.array_equal(rebuilt, expect)  # the oracle's rebuild is the encode's input and output
    assert np.array_equal(d.cpu().numpy(), rebuilt), (K, MT, S, ua, lost, "reconstruct")
    seen_label(enc_label)
    seen_label(rec_label)


# ---------------------------------------------------------------- leg 1: plain coding kernels
ALIGNED_S = [1, 15, 16, 1024, 1040, 4097, 5000]
UA_S = [16, 17, 1023, 1025, 4097, 5000]


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
def test_plain_kernels(gpu, K):
    """fn and ua of every (K, MT): encode and an in-place MT-row reconstruct at sizes below one
    chunk, on and off the 16-byte grid, on and past a tile (1 KiB per row) and over several tiles,
    random rows and the all-values ramp, guards and padding untouched, the label exact."""
    torch, rsmi = gpu
    with _leg("leg1"):
        for MT in MTS:
            rng = np.random.default_rng(1000 * K + MT)
            with rsmi.Codec(K, MT) as c:
                for ua, sizes, ramp_at in ((False, ALIGNED_S, 1024), (True, UA_S, 1025)):
                    label = fast_label(K, MT, ua=ua)
                    for S in sizes:
                        data = _data(rng, K, S, NB, "ramp" if S == ramp_at else "random")
                        _encode_then_rebuild(torch, rsmi, c, K, MT, S, ua, data, rng, label, label)


# ---------------------------------------------------------------- leg 2: CRC-fused encodes
CRC_ALIGNED_S = [1, 15, 16, 1024, 4096, 4097, 5000, 16385]   # cross the 4-tile unit, last unit 1..4 tiles
CRC_SPLIT_S = [16, 17, 31, 4096, 4111] + [9216 + r for r in (0, 1, 7, 15)]


def _want_r(full):
    return [[orc.crc16_ibm(row.tobytes()) for row in blk] for blk in full]


def _check_raw(rsmi, raw, want_r, S, ctx):
    r = raw.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    assert (r < 0x10000).all(), ctx
    for b in range(len(want_r)):
        for i in range(len(want_r[b])):
            assert rsmi.crc16_entry(b"", int(r[b, i]), S) == want_r[b][i], ctx + (b, i)


def _crc_encode(torch, rsmi, c, K, MT, S, split, data, full, want_r, label, ctx):
    n = K + MT
    # aligned: pitched rows whose padding must neither reach the CRC nor be written; split: rows
    # back to back at pitch S from a base misaligned by 1
    lay = Layout(rsmi, n, S, NB, split, off=1 if split else 0, rs=S if split else None)
    host = lay.buffer(0xA5)
    lay.rows(host)[:, :K] = data
    d = torch.from_numpy(host.copy()).cuda()
    raw = torch.zeros((NB, n), dtype=torch.int32, device="cuda")
    base = d.data_ptr() + lay.off
    c.encode_batch_dev_crc(base, lay.rs, lay.bs, base + K * lay.rs, lay.rs, lay.bs, S, NB, raw.data_ptr(),
                           _stream(torch))
    torch.cuda.synchronize()
    kern = c.last_kernel()
    if label is not None:
        assert kern == label, (kern, label) + ctx
    expect = host.copy()
    lay.rows(expect)[:] = full
    assert np.array_equal(d.cpu().numpy(), expect), ctx  # parity rows; padding and guards still 0xA5
    _check_raw(rsmi, raw, want_r, S, ctx)
    if label is not None:
        seen_label(kern)
    return kern


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
def test_crc_fused_encodes(gpu, K):
    """crc, ua_crc, fused and fused_ua of every (K, MT) through rsmi_encode_batch_dev_crc: parity
    and all K + MT values of R(row).  All-0xFF rows drive every count of the matrix-core fold to
    its maximum for every accumulator pairing (odd K + MT leaves a lone last accumulator)."""
    torch, rsmi = gpu
    with _leg("leg2"):
        for MT in MTS:
            rng = np.random.default_rng(2000 * K + MT)
            cases = [(False, S, "random") for S in CRC_ALIGNED_S] + [(False, 4097, "ones")] + \
                    [(True, S, "random") for S in CRC_SPLIT_S] + [(True, 9223, "ones")]
            prepared = []
            for split, S, kind in cases:
                data = _data(rng, K, S, NB, kind)
                full = _full(K, MT, data)
                prepared.append((split, S, kind, data, full, _want_r(full)))
            for fold in (1, 0):
                with rsmi.Codec(K, MT) as c:
                    c.set_option("crc16_fused_fold", fold)
                    for split, S, kind, data, full, want_r in prepared:
                        if fold == 1:
                            label = fused_label(K, MT, S, NB, ua=split)
                        else:
                            label = fast_label(K, MT, ua=split, crc=True)
                        _crc_encode(torch, rsmi, c, K, MT, S, split, data, full, want_r, label,
                                    (K, MT, S, split, kind, fold))


@pytest.mark.gpu
@pytest.mark.parametrize("K,MT", INL_SHAPES)
def test_inl_shapes_two_launch_form(gpu, K, MT):
    """The INL shapes past kFusedInlineUnits (nb * units > 64) take the two-launch form again:
    the plain fused / fused_ua instantiation of these four pairs, which leg 2's small launches
    (always combined in the kernel) never reach."""
    torch, rsmi = gpu
    with _leg("leg2"):
        rng = np.random.default_rng(2500 + K)
        with rsmi.Codec(K, MT) as c:
            for split, S in ((False, 22 * 4096 + 16), (True, 22 * 4096 + 17)):
                assert NB * fused_units(S) > 64
                data = _data(rng, K, S, NB)
                full = _full(K, MT, data)
                label = fused_label(K, MT, S, NB, ua=split)
                assert ",INL" not in label
                _crc_encode(torch, rsmi, c, K, MT, S, split, data, full, _want_r(full), label, (K, MT, S, split))


# ---------------------------------------------------------------- leg 3: verified reconstruct, fused kernels
def _host_rows(rsmi, nbytes):
    p = rsmi.lib().rsmi_host_alloc(nbytes)
    assert p
    return p, np.ctypeslib.as_array((ctypes.c_uint8 * nbytes).from_address(p))


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
def test_verified_reconstruct_fused(gpu, K):
    """The non-encode plan path of launch_plan_crc: rsmi_reconstruct_batch_host_verify over
    page-locked rows rebuilds MT lost rows with the fused kernel of (K, MT) and returns R of the
    first K present rows.  S = 32: rows on the 16-byte grid; S = 4111: unaligned windows."""
    torch, rsmi = gpu
    with _leg("leg3"):
        for MT in MTS:
            n = K + MT
            rng = np.random.default_rng(3000 * K + MT)
            with rsmi.Codec(K, MT) as c:
                for S in (32, 4111):
                    p, flat = _host_rows(rsmi, NB * n * S)
                    try:
                        sh = flat.reshape(NB, n, S)
                        full = _full(K, MT, _data(rng, K, S, NB))
                        want_r = _want_r(full)
                        lost = _loss(rng, K, MT)
                        present = [i not in lost for i in range(n)]
                        used = [i for i in range(n) if present[i]][:K]
                        sh[:] = full
                        sh[:, lost] = 0xEE
                        raw = np.zeros((NB, K), dtype=np.uint32)
                        c.reconstruct_batch_host_verify_ptr(p, n * S, S, NB, present, False, raw.ctypes.data)
                        kern = c.last_kernel()
                        # the suffix (",UA", ",INL") is leg 2's subject; here the prefix shows that
                        # the fused kernel of this pair coded the decode plan
                        assert kern.startswith("rs_fused_mfma_kernel<K=%d,MT=%d," % (K, MT)), kern
                        assert np.array_equal(sh, full), (K, MT, S, lost)  # rebuilt rows and survivors
                        for b in range(NB):
                            for j, i in enumerate(used):
                                assert raw[b, j] < 0x10000
                                assert rsmi.crc16_entry(b"", int(raw[b, j]), S) == want_r[b][i], (K, MT, S, b, j)
                        del sh
                    finally:
                        del flat
                        rsmi.lib().rsmi_host_free(p)


def _lone_cases():
    out = [("encode", k, m, m) for k, m in TB_FUSED_SHAPES]
    # a lone verified reconstruct of the BASELINE configs: MT rows lost of RS(K, m)
    base_m = dict(TB_FUSED_SHAPES)
    out += [("reconstruct", k, base_m[k], mt) for k, mt in TB_FUSED_INL_SHAPES]
    out += [("reconstruct", k, m, m) for k, m in TB_FUSED_SHAPES]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("flag", [1, 0])
@pytest.mark.parametrize("kind,k,m,MT", _lone_cases())
def test_lone_table_forms(gpu, kind, k, m, MT, flag):
    """One-block in-place host calls on page-locked rows take the table form with a single zero
    base, the combine inside the kernel and a completion flag (option coalesce_flag 1): the
    fused_inl_tb / fused_ua_inl_tb instantiations.  Three calls on one context: the flag slots and
    the unit counters are reused.  coalesce_flag 0: the same call without the table."""
    torch, rsmi = gpu
    n = k + m
    rng = np.random.default_rng(3500 + 100 * k + 10 * MT + flag)
    with _leg("leg3"), rsmi.Codec(k, m) as c:
        c.set_option("coalesce_flag", flag)
        for S in (32, 4111):
            ua = S % 16 != 0
            p, flat = _host_rows(rsmi, n * S)
            try:
                sh = flat.reshape(n, S)
                for rep in range(3):
                    full = _full(k, m, _data(rng, k, S, 1))[0]
                    want_r = [orc.crc16_ibm(r.tobytes()) for r in full]
                    if kind == "encode":
                        sh[:] = 0x5A
                        sh[:k] = full[:k]
                        raw = np.zeros(n, dtype=np.uint32)
                        c.encode_batch_host_crcs_ptr(p, n * S, p + k * S, n * S, S, 1, raw.ctypes.data, None)
                        rows = list(range(n))
                    else:
                        lost = sorted(int(x) for x in rng.choice(n, size=MT, replace=False))
                        present = [i not in lost for i in range(n)]
                        sh[:] = full
                        sh[lost] = 0xEE
                        raw = np.zeros(k, dtype=np.uint32)
                        c.reconstruct_batch_host_verify_ptr(p, n * S, S, 1, present, False, raw.ctypes.data)
                        rows = [i for i in range(n) if present[i]][:k]
                    kern = c.last_kernel()
                    assert np.array_equal(sh, full), (kind, k, m, MT, S, rep)
                    assert [rsmi.crc16_entry(b"", int(x), S) for x in raw] == [want_r[i] for i in rows], (S, rep)
                    assert (raw < 0x10000).all()
                    if flag:
                        assert kern == ("rs_fused_mfma_kernel<K=%d,MT=%d,NT=%d>" % (k, MT, nt_of(k, MT)) +
                                        (",UA" if ua else "") + ",INL,TB"), kern
                    else:
                        # without the flag the call is an ordinary launch: leg 2's label rule
                        assert kern == fused_label(k, MT, S, 1, ua=ua), kern
                    seen_label(kern)
                del sh
            finally:
                del flat
                rsmi.lib().rsmi_host_free(p)


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", TB_FUSED_SHAPES)
def test_lone_table_forms_two_launch(gpu, k, m):
    """fused_tb / fused_ua_tb: a lone block of more than kFusedInlineUnits (64) units keeps the
    table form but combines in a second launch (no ",INL", no completion flag)."""
    torch, rsmi = gpu
    n = k + m
    rng = np.random.default_rng(3900 + k)
    with _leg("leg3"), rsmi.Codec(k, m) as c:
        c.set_option("coalesce_flag", 1)
        for S in (64 * 4096 + 16, 64 * 4096 + 17):
            assert fused_units(S) == 65
            ua = S % 16 != 0
            p, flat = _host_rows(rsmi, n * S)
            try:
                sh = flat.reshape(n, S)
                full = _full(k, m, _data(rng, k, S, 1))[0]
                sh[:] = 0x5A
                sh[:k] = full[:k]
                raw = np.zeros(n, dtype=np.uint32)
                c.encode_batch_host_crcs_ptr(p, n * S, p + k * S, n * S, S, 1, raw.ctypes.data, None)
                kern = c.last_kernel()
                assert kern == ("rs_fused_mfma_kernel<K=%d,MT=%d,NT=%d>" % (k, m, nt_of(k, m)) +
                                (",UA" if ua else "") + ",TB"), kern
                assert np.array_equal(sh, full), (k, m, S)
                assert [rsmi.crc16_entry(b"", int(x), S) for x in raw] == [orc.crc16_ibm(r.tobytes()) for r in full]
                seen_label(kern)
                del sh
            finally:
                del flat
                rsmi.lib().rsmi_host_free(p)


# ---------------------------------------------------------------- leg 4: table-of-bases plain kernels
@pytest.mark.gpu
@pytest.mark.parametrize("K", TB_KS)
def test_table_plain_kernels(gpu, K):
    """fn_tb / ua_tb of every (K, MT): T = 3 callers, each with their own page-locked buffer, lose
    the same MT rows and call rsmi_reconstruct_coalesced at once (one lane, coalesce_us and
    coalesce_max T make them one batch, as in test_random_coalesced_groups): one launch over the
    table of the three bases."""
    torch, rsmi = gpu
    T = 3
    L = rsmi.lib()
    with _leg("leg4"):
        for MT in MTS:
            n = K + MT
            rng = np.random.default_rng(4000 * K + MT)
            with rsmi.Codec(K, MT) as c:
                c.set_option("coalesce_lanes", 1)
                c.set_option("coalesce_us", 100000)
                c.set_option("coalesce_max", T)
                for S in (32, 33):
                    ptrs = [L.rsmi_host_alloc(n * S) for _ in range(T)]
                    assert all(ptrs)
                    try:
                        views = [np.ctypeslib.as_array((ctypes.c_uint8 * (n * S)).from_address(p)).reshape(n, S)
                                 for p in ptrs]
                        full = _full(K, MT, _data(rng, K, S, T))
                        lost = _loss(rng, K, MT)
                        present = (ctypes.c_uint8 * n)(*[0 if i in lost else 1 for i in range(n)])
                        for t in range(T):
                            views[t][:] = full[t]
                            views[t][lost] = 0xEE
                        rcs = [None] * T

                        def rec(t):
                            rcs[t] = L.rsmi_reconstruct_coalesced(c._h, ptrs[t], S, present, 0)

                        th = [threading.Thread(target=rec, args=(t,)) for t in range(T)]
                        for x in th:
                            x.start()
                        for x in th:
                            x.join()
                        assert rcs == [0] * T
                        assert c.last_kernel() == fast_label(K, MT, ua=S % 16 != 0, tb=True), c.last_kernel()
                        for t in range(T):
                            assert np.array_equal(views[t], full[t]), (K, MT, S, t, lost)
                        seen_label(c.last_kernel())
                        del views
                    finally:
                        for p in ptrs:
                            L.rsmi_host_free(p)


# ---------------------------------------------------------------- leg 5: shapes without an instantiation
@pytest.mark.gpu
@pytest.mark.parametrize("k,m", GENERIC_SHAPES)
def test_uninstantiated_shapes_fall_to_generic(gpu, k, m):
    """K in {7, 9, 11, 13, 14, 15} has no fast kernel: plain calls run rs_generic_kernel, and the
    encode with CRC succeeds through the separate pass (no fused, no ",CRC" kernel)."""
    torch, rsmi = gpu
    with _leg("leg5"):
        rng = np.random.default_rng(5000 + 10 * k + m)
        label = generic_label(k, m)
        with rsmi.Codec(k, m) as c:
            for S in (5, 1040):
                for ua in (False, True):
                    data = _data(rng, k, S, NB)
                    _encode_then_rebuild(torch, rsmi, c, k, m, S, ua, data, rng, label, label)
                    full = _full(k, m, data)
                    want_r = _want_r(full)
                    n = k + m
                    lay = Layout(rsmi, n, S, NB, ua)
                    host = lay.buffer(0xA5)
                    lay.rows(host)[:, :k] = data
                    d = torch.from_numpy(host.copy()).cuda()
                    raw = torch.zeros((NB, n), dtype=torch.int32, device="cuda")
                    base = d.data_ptr() + lay.off
                    for fold in (1, 0):
                        c.set_option("crc16_fused_fold", fold)
                        d.copy_(torch.from_numpy(host))
                        raw.zero_()
                        c.encode_batch_dev_crc(base, lay.rs, lay.bs, base + k * lay.rs, lay.rs, lay.bs, S, NB,
                                               raw.data_ptr(), _stream(torch))
                        torch.cuda.synchronize()
                        kern = c.last_kernel()
                        assert "rs_fused_mfma_kernel" not in kern and ",CRC" not in kern, kern
                        expect = host.copy()
                        lay.rows(expect)[:] = full
                        assert np.array_equal(d.cpu().numpy(), expect), (k, m, S, ua, fold)
                        _check_raw(rsmi, raw, want_r, S, (k, m, S, ua, fold))


# ---------------------------------------------------------------- leg 6: rs_generic_kernel's stride loops
@pytest.mark.gpu
@pytest.mark.parametrize("S,nb", [(3, 65535 + 2), (4 * 256 * 4096 + 5, 1)])
def test_generic_stride_loops(gpu, S, nb):
    """The launcher caps rs_generic_kernel's grid at 65535 blocks in y and at 4096 x 256 four-byte
    groups in x: more blocks, and a row longer than 4 MiB (with a partial last group), run the
    second pass of each grid-stride loop."""
    torch, rsmi = gpu
    k, m = 7, 1
    n = k + m
    with _leg("leg6"):
        data = _data(np.random.default_rng(6000 + nb), k, S, nb)
        want = orc.encode_fast(k, m, data)
        host = np.full((nb, n, S), 0x5A, dtype=np.uint8)  # contiguous rows
        host[:, :k] = data
        d = torch.from_numpy(host.reshape(-1)).cuda()
        with rsmi.Codec(k, m) as c:
            c.encode_batch_dev(d.data_ptr(), S, n * S, d.data_ptr() + k * S, S, n * S, S, nb, _stream(torch))
            torch.cuda.synchronize()
            assert c.last_kernel() == generic_label(k, m), c.last_kernel()
        got = d.cpu().numpy().reshape(nb, n, S)
        assert np.array_equal(got[:, :k], data)
        assert np.array_equal(got[:, k:], want)


# ---------------------------------------------------------------- leg 7: rsmi_reconstruct_rows_batch_dev
@pytest.mark.gpu
@pytest.mark.parametrize("S", [17, 4099])
@pytest.mark.parametrize("ua", [False, True])
def test_reconstruct_rows_batch_dev(gpu, S, ua):
    """Only the rows that are required and missing are rebuilt; missing rows not asked for keep
    their 0xEE fill, present rows (required or not) and every guard byte are left alone, and the
    launch writes exactly as many rows as the label's MT says."""
    torch, rsmi = gpu
    k, m, nb = 10, 4, 5
    n = k + m
    lost = [1, 4, 11, 13]
    present = [i not in lost for i in range(n)]
    with _leg("leg7"):
        lay = Layout(rsmi, n, S, nb, ua)
        full = _full(k, m, _data(np.random.default_rng(7000 + S), k, S, nb))
        erased = lay.buffer(0x5A)
        lay.rows(erased)[:] = full
        lay.rows(erased)[:, lost] = 0xEE
        for b in range(nb):  # the oracle rebuilds every missing row
            rc, sh = orc.reconstruct(k, m, np.ascontiguousarray(lay.rows(erased)[b]), present, False)
            assert rc == 0 and np.array_equal(sh, full[b])
        d = torch.empty(lay.size, dtype=torch.uint8, device="cuda")
        base = d.data_ptr() + lay.off
        with rsmi.Codec(k, m) as c:
            for req in ([4], [11], [1, 13], [1, 4, 11, 13], [0, 4], []):
                d.copy_(torch.from_numpy(erased))
                before = c.last_kernel()
                c.reconstruct_rows_batch_dev(base, lay.rs, lay.bs, S, nb, present, [i in req for i in range(n)],
                                             _stream(torch))
                torch.cuda.synchronize()
                rebuilt = [i for i in req if i in lost]
                expect = erased.copy()
                lay.rows(expect)[:, rebuilt] = full[:, rebuilt]
                assert np.array_equal(d.cpu().numpy(), expect), (S, ua, req)
                kern = c.last_kernel()
                if rebuilt:
                    assert kern == fast_label(k, len(rebuilt), ua=ua), (kern, req)
                    assert int(re.search(r"MT=(\d+)", kern).group(1)) == len(rebuilt)
                else:
                    assert kern == before  # nothing required is missing: OK, no launch, nothing written
            few = list(present)
            few[0] = False  # 9 rows present
            with pytest.raises(rsmi.RsmiError) as e:
                c.reconstruct_rows_batch_dev(base, lay.rs, lay.bs, S, nb, few, [i == 4 for i in range(n)],
                                             _stream(torch))
            assert e.value.code == rsmi.ErrTooFewShards


# ---------------------------------------------------------------- leg 8: offsets past 2^32
def _far_case(torch, rsmi, c, d, off, rs, bs, S, nb, ua, seed):
    k, m = 4, 2
    n = k + m
    full = _full(k, m, _data(np.random.default_rng(seed), k, S, nb))

    def row(b, i):
        o = off + b * bs + i * rs
        return d[o:o + S]

    for b in range(nb):
        for i in range(n):
            if i < k:
                row(b, i).copy_(torch.from_numpy(full[b, i]))
            else:
                # the allocation is not filled: whatever an earlier run left where the parity
                # goes (the right bytes, even) must not pass for this run's output
                row(b, i).fill_(0xEE)
    base = d.data_ptr() + off
    label = fast_label(k, m, ua=ua)
    c.encode_batch_dev(base, rs, bs, base + k * rs, rs, bs, S, nb, _stream(torch))
    torch.cuda.synchronize()
    assert c.last_kernel() == label, c.last_kernel()
    for b in range(nb):
        for i in range(n):
            assert np.array_equal(row(b, i).cpu().numpy(), full[b, i]), ("encode", off, rs, bs, b, i)
    lost = [1, 4]
    for b in range(nb):
        for i in lost:
            row(b, i).fill_(0xEE)
    c.reconstruct_batch_dev(base, rs, bs, S, nb, [i not in lost for i in range(n)], False, _stream(torch))
    torch.cuda.synchronize()
    assert c.last_kernel() == label, c.last_kernel()
    for b in range(nb):
        for i in range(n):
            assert np.array_equal(row(b, i).cpu().numpy(), full[b, i]), ("reconstruct", off, rs, bs, b, i)


@pytest.mark.gpu
def test_offsets_past_4gib(gpu):
    """A block at block_stride = 2^32 + 256, and rows at shard_stride = 2^30 + 16 (row 4 and later
    past 2^32), aligned and shifted by one byte (the UA kernel).  An offset truncated to 32 bits
    would land inside the allocation, so it shows as wrong bytes, not as a fault."""
    torch, rsmi = gpu
    if torch.cuda.mem_get_info()[0] < 8 << 30:
        pytest.skip("needs 8 GiB of free device memory")
    S = 1040
    with _leg("leg8"):
        try:
            with rsmi.Codec(4, 2) as c:
                d = torch.empty(2 ** 32 + 2 ** 20, dtype=torch.uint8, device="cuda")
                bs = 2 ** 32 + 256
                assert 1 + bs + 6 * S <= d.numel()
                _far_case(torch, rsmi, c, d, 0, S, bs, S, 2, False, 8001)
                _far_case(torch, rsmi, c, d, 1, S, bs, S, 2, True, 8002)
                del d
                torch.cuda.empty_cache()
                rs = 2 ** 30 + 16
                d = torch.empty(5 * rs + S + 64, dtype=torch.uint8, device="cuda")
                assert 4 * rs >= 2 ** 32
                _far_case(torch, rsmi, c, d, 0, rs, 6 * rs, S, 1, False, 8003)
                _far_case(torch, rsmi, c, d, 1, rs, 6 * rs, S, 1, True, 8004)
                del d
        finally:
            torch.cuda.empty_cache()
