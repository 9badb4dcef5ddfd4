"""The device entry points with independent data and parity layouts, bit for bit.

include/rsmi.h gives rsmi_encode_batch_dev, rsmi_encode_batch_dev_crc and rsmi_verify_batch_dev two
independent halves: row c of data block b at d_data + b*data_block_stride + c*data_shard_stride,
parity row j at d_parity + b*parity_block_stride + j*parity_shard_stride.  The other modules call
them with one shard stride (and mostly one buffer and one block stride) for both halves, where
out_off taken from in_rs, a dropped term of the alignment predicate, a funnel shift taken from the
wrong pointer or enc_rs swapped with parity_rs all give the right address.  Here the two halves
differ in everything: allocation, base, shard stride, block stride, dword phase.

A case is a pair of sides, Side(alloc, off, rs, bs), for the k data rows and the m parity rows.
Every buffer has 64 guard bytes before and after, is filled with 0xA5 (it holds data rows) or 0x5A
(parity rows only), and its expected image is built on the CPU: after each call the whole of every
buffer is compared, so a row written at the wrong pitch, into the wrong buffer, or one byte too
long shows.  The launch label (rsmi_last_kernel) is part of every assertion: expected_form() below
restates the alignment predicate of launch_plan / launch_plan_crc / launch_verify (leg 0 pins its
text to the source), so a case that silently fell to another kernel fails.

References: oracle_lib.encode_fast, oracle_lib.crc16_ibm, zlib.crc32.  Everything is bit-exact:
there are no tolerances.  Leg 0 also shows, on the CPU, that the module's own comparison rejects
the slips it is there for (simulated "got" buffers; no wrong kernel is built or run).
"""
import collections
import ctypes
import os
import time
import zlib

import numpy as np
import pytest

import oracle_lib as orc
from test_kernel_matrix import KS, fast_label, fused_label, fused_units, generic_label, nt_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "filedag-storage_amd", "csrc")

GUARD = 64
FILL_DATA, FILL_PARITY = 0xA5, 0x5A
NB = 3

# (10,4): its own store-path kernel and the grouped tile order, NT=1; (16,4): NT=2, UA4 loads;
# (5,5): two plan tiles, the second with out_row = 4; (3,4): K < MT; (7,2): no instantiation;
# (20,4): K > 16
SHAPES = [(10, 4), (16, 4), (4, 2), (2, 1), (5, 5), (3, 4), (7, 2), (20, 4)]
ALIGNED_S = [1000, 1040, 2049]   # a partial last chunk; one tile plus one chunk; two tiles plus one byte
UA_S = [17, 1025, 2049]
S_SHORT = 15                     # unaligned rows below 16 bytes: rs_generic_kernel
ALIGNED_IDS = ["A0", "A0m", "below", "interleaved"]
T_IDS = ["T-dbase8", "T-drs8", "T-dbs8", "T-pbase8", "T-prs8", "T-pbs8", "T-dbase1", "T-pbase1"]
UA_IDS = T_IDS + ["split-in", "split-out", "phases"]
SHORT_IDS = ["split-in", "phases", "T-dbase8"]
ALL_S = sorted(set(ALIGNED_S + UA_S + [S_SHORT]))

Side = collections.namedtuple("Side", "alloc off rs bs")


def round_up(x, a):
    return (x + a - 1) // a * a


# ---------------------------------------------------------------- the geometry model
def geometries(k, m, S, nb=NB):
    """id -> (data side, parity side).  off counts from the end of the buffer's leading guard."""
    R = round_up(S, 16)

    def data(off=64, rs=R + 16, bs=None):
        return Side("d", off, rs, round_up(k * rs, 16) + 32 if bs is None else bs)

    def par(off=128, rs=R + 48, bs=None):
        return Side("p", off, rs, round_up(m * rs, 16) + 16 if bs is None else bs)

    g = collections.OrderedDict()
    g["A0"] = (data(), par())
    g["A0m"] = (data(rs=R + 48), par(rs=R + 16))
    # A0 with exactly one term of the predicate broken
    g["T-dbase8"] = (data(off=64 + 8), par())
    g["T-drs8"] = (data(rs=R + 16 + 8), par())
    g["T-dbs8"] = (data(bs=data().bs + 8), par())
    g["T-pbase8"] = (data(), par(off=128 + 8))
    g["T-prs8"] = (data(), par(rs=R + 48 + 8))
    g["T-pbs8"] = (data(), par(bs=par().bs + 8))
    g["T-dbase1"] = (data(off=64 + 1), par())
    g["T-pbase1"] = (data(), par(off=128 + 1))
    # the Split layout (rows back to back at pitch S) on one side, pitched rows on the other
    g["split-in"] = (Side("d", 0, S, k * S), par())
    g["split-out"] = (data(), Side("p", 0, S, m * S))
    # every row of either side at its own byte phase
    g["phases"] = (Side("d", 3, S + 1, k * (S + 1) + 5), Side("p", 2, S + 2, m * (S + 2) + 7))
    # one allocation: all parity blocks, then all data blocks (d_parity < d_data)
    p = Side("x", 64, R + 48, m * (R + 48) + 16)
    g["below"] = (Side("x", p.off + nb * p.bs + 32, R + 16, k * (R + 16) + 32), p)
    # one allocation: parity block b directly after data block b, one block stride, two pitches
    bs = k * (R + 16) + m * (R + 48)
    g["interleaved"] = (Side("x", 64, R + 16, bs), Side("x", 64 + k * (R + 16), R + 48, bs))
    assert list(g) == ["A0", "A0m"] + T_IDS + ["split-in", "split-out", "phases", "below", "interleaved"]
    return g


def terms(d, p, S, dbase=0, pbase=0):
    """The ten terms of the predicate, for bases dbase / pbase (mod 16) of the two allocations."""
    R = round_up(S, 16)
    return ((dbase + GUARD + d.off) % 16 == 0, (pbase + GUARD + p.off) % 16 == 0, d.rs % 16 == 0, d.bs % 16 == 0,
            p.rs % 16 == 0, p.bs % 16 == 0, d.rs >= R, p.rs >= R, S < 2 ** 31)


def expected_form(dptr, drs, dbs, pptr, prs, pbs, S):
    """The predicate of launch_plan, launch_plan_crc and launch_verify, written out here on
    purpose: aligned, else the unaligned-window kernels for rows of at least 16 bytes, else the
    byte-granular kernel."""
    R = round_up(S, 16)
    if (dptr % 16 == 0 and pptr % 16 == 0 and drs % 16 == 0 and dbs % 16 == 0 and prs % 16 == 0 and
            pbs % 16 == 0 and drs >= R and prs >= R and S < 2 ** 31):
        return "aligned"
    if S >= 16 and S < 2 ** 31 and drs >= S and prs >= S:
        return "ua"
    return "generic"


def sizes_of(gid):
    if gid in ALIGNED_IDS:
        return ALIGNED_S
    return UA_S + ([S_SHORT] if gid in SHORT_IDS else [])


def cases(k, m, nb=NB):
    """(id, S, data side, parity side, expected form) of every case of a shape; the form assumes
    16-byte-aligned allocations (the GPU legs assert that of each tensor)."""
    for S in ALL_S:
        for gid, (d, p) in geometries(k, m, S, nb).items():
            if S in sizes_of(gid):
                yield gid, S, d, p, expected_form(GUARD + d.off, d.rs, d.bs, GUARD + p.off, p.rs, p.bs, S)


def last_mt(m):
    """The encode plan cuts m output rows into tiles of at most 4; the label is the last tile's."""
    return m - 4 * ((m - 1) // 4)


def encode_label(k, m, form):
    if form == "generic" or k not in KS:
        return generic_label(k, last_mt(m))
    return fast_label(k, last_mt(m), ua=form == "ua")


def crc_label(k, m, S, nb, form, fold):
    """rsmi_encode_batch_dev_crc: one plan tile of an instantiated K on an aligned or UA layout
    runs a kernel with the CRC fused in; everything else is the encode and the separate pass."""
    if form == "generic" or k not in KS or m > 4:
        return encode_label(k, m, form)
    if fold:
        return fused_label(k, m, S, nb, ua=form == "ua")
    return fast_label(k, m, ua=form == "ua", crc=True)


def verify_label(k, m, form):
    if form == "generic" or k not in KS:
        return "rs_compare_rows_kernel"
    return "rs_verify_kernel<K=%d,MT=%d>%s" % (k, last_mt(m), ",UA" if form == "ua" else "")


def alloc_sizes(d, p, nb):
    size = {}
    for s in (d, p):
        size[s.alloc] = max(size.get(s.alloc, 0), GUARD + s.off + nb * s.bs + GUARD)
    return size


def blank(d, p, nb):
    """Every buffer of a case, filled: 0xA5 where data rows live, 0x5A in a parity-only buffer."""
    size = alloc_sizes(d, p, nb)
    return {a: np.full(n, FILL_DATA if a == d.alloc else FILL_PARITY, dtype=np.uint8) for a, n in size.items()}


def row_at(side, b, r):
    return GUARD + side.off + b * side.bs + r * side.rs


def put(bufs, side, rows, clip=False):
    """rows[b, r] into its place.  clip (the simulated slips only): bytes past the buffer's end are
    dropped, where a kernel would have written out of bounds."""
    buf = bufs[side.alloc]
    S = rows.shape[2]
    for b in range(rows.shape[0]):
        for r in range(rows.shape[1]):
            o = row_at(side, b, r)
            if clip:
                n = max(0, min(S, buf.size - o))
                buf[o:o + n] = rows[b, r, :n]
            else:
                assert o + S <= buf.size
                buf[o:o + S] = rows[b, r]


def check(got, want, ctx):
    """The module's comparison: every buffer of the case, whole."""
    assert sorted(got) == sorted(want), ctx
    for a in sorted(want):
        g, w = got[a], want[a]
        assert g.dtype == np.uint8 and g.shape == w.shape, (ctx, a, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.flatnonzero(g != w)
            raise AssertionError("%r: buffer %r: %d of %d bytes differ, first at %d (got %#x, want %#x), last at %d"
                                 % (ctx, a, bad.size, g.size, bad[0], g[bad[0]], w[bad[0]], bad[-1]))


def check_raw(rsmi, raw, want_r, S, ctx):
    """raw[b, r] is R(row r of block b), data rows first: through rsmi_crc16_entry with an empty
    head it must be the oracle's CRC-16 of the row."""
    r = np.asarray(raw).astype(np.int64) & 0xFFFFFFFF
    assert r.shape == (len(want_r), len(want_r[0])), ctx
    assert (r < 0x10000).all(), ctx
    for b in range(r.shape[0]):
        for i in range(r.shape[1]):
            assert rsmi.crc16_entry(b"", int(r[b, i]), S) == want_r[b][i], ctx + ("crc16", b, i)


class Ref:
    """Random data rows, the oracle's parity and the rows' checksums: computed once per
    (k, m, S, nb), read-only."""

    def __init__(self, k, m, S, nb):
        rng = np.random.default_rng(900001 * k + 9001 * m + 11 * S + nb)
        self.data = rng.integers(0, 256, size=(nb, k, S), dtype=np.uint8)
        self.parity = orc.encode_fast(k, m, self.data, threads=4)
        self.data.setflags(write=False)
        self.parity.setflags(write=False)
        self._r16 = self._r32 = None

    def rows(self, b):
        return list(self.data[b]) + list(self.parity[b])

    def r16(self):
        if self._r16 is None:
            self._r16 = [[orc.crc16_ibm(r.tobytes()) for r in self.rows(b)] for b in range(len(self.data))]
        return self._r16

    def r32(self):
        if self._r32 is None:
            self._r32 = [[zlib.crc32(r.tobytes()) for r in self.rows(b)] for b in range(len(self.data))]
        return self._r32


_REFS = {}


def ref_of(k, m, S, nb=NB):
    if (k, m, S, nb) not in _REFS:
        _REFS[(k, m, S, nb)] = Ref(k, m, S, nb)
    return _REFS[(k, m, S, nb)]


# ---------------------------------------------------------------- leg 0 (CPU)
def _spans(side, nrows, S, nb):
    return [(side.alloc, row_at(side, b, r), row_at(side, b, r) + S) for b in range(nb) for r in range(nrows)]


@pytest.mark.parametrize("k,m", SHAPES)
def test_geometries_are_well_formed(k, m):
    """Rows and blocks disjoint, everything between its buffer's guards, rs >= S, for every
    geometry at every size it is used with; each id has the form it is there for."""
    for nb in (NB, 65):
        todo = list(cases(k, m, nb))
        if nb == 65:  # the sizes of the two-launch CRC form
            todo = [(gid, S, d, p, expected_form(GUARD + d.off, d.rs, d.bs, GUARD + p.off, p.rs, p.bs, S))
                    for S in (1040, 1041) for gid, (d, p) in geometries(k, m, S, nb).items()]
        for gid, S, d, p, form in todo:
            ctx = (k, m, nb, gid, S)
            size = alloc_sizes(d, p, nb)
            assert d.rs >= S and p.rs >= S and d.bs >= k * d.rs and p.bs >= m * p.rs, ctx
            spans = sorted(_spans(d, k, S, nb) + _spans(p, m, S, nb))
            for a, lo, hi in spans:
                assert GUARD <= lo and hi <= size[a] - GUARD, ctx
            for (a0, _, hi0), (a1, lo1, _) in zip(spans, spans[1:]):
                assert a0 != a1 or hi0 <= lo1, ctx
            assert max(size.values()) <= 4 << 20, ctx
            if gid in ALIGNED_IDS:
                assert form == "aligned", ctx
            elif nb == NB:
                assert form == ("generic" if S < 16 else "ua"), ctx
            assert (d.alloc == p.alloc) == (gid in ("below", "interleaved")), ctx
            if gid == "below":
                assert p.off < d.off
            if gid not in ("split-in", "phases"):
                assert d.rs > S       # room for the byte at offset S of a data row
            if gid not in ("split-out", "phases"):
                assert p.rs > S
            assert d.rs != p.rs, ctx  # no case of this module is on the diagonal
    assert sorted({S for _, S, _, _, f in cases(k, m) if f == "aligned"}) == sorted(ALIGNED_S)
    assert sorted({S for _, S, _, _, f in cases(k, m) if f == "ua"}) == sorted(UA_S)
    assert sorted({g for g, S, _, _, f in cases(k, m) if f == "generic"}) == sorted(SHORT_IDS)


@pytest.mark.parametrize("k,m", SHAPES)
def test_single_term_cases_break_one_term(k, m):
    """Each T-* case differs from A0 in exactly one of the predicate's terms, the six modulo terms
    are each broken at least once, and the +8 cases are still aligned modulo 8 and modulo 4."""
    broken = set()
    for S in ALL_S:
        g = geometries(k, m, S)
        a0 = terms(g["A0"][0], g["A0"][1], S)
        assert all(a0), (k, m, S)
        for gid in T_IDS:
            t = terms(g[gid][0], g[gid][1], S)
            diff = [i for i in range(len(t)) if t[i] != a0[i]]
            assert len(diff) == 1 and diff[0] < 6, (k, m, S, gid, diff)
            broken.add(diff[0])
            if gid.endswith("8"):
                d, p = g[gid]
                assert all(x % 8 == 0 for x in (GUARD + d.off, d.rs, d.bs, GUARD + p.off, p.rs, p.bs)), (S, gid)
    assert broken == set(range(6))


def test_phases_case_rotates_the_rows():
    """The "phases" case at the sizes of the unaligned-window kernels: over the rows of the three
    blocks the data rows start at all four byte phases of a dword and the parity rows at two or
    more, and the two sides' rows do not run through the same sequence of phases (with one parity
    row per block: not in every block)."""
    for k, m in SHAPES:
        for S in UA_S:
            d, p = geometries(k, m, S)["phases"]
            din = [[row_at(d, b, r) % 4 for r in range(k)] for b in range(NB)]
            pout = [[row_at(p, b, r) % 4 for r in range(m)] for b in range(NB)]
            assert {x for blk in din for x in blk} == {0, 1, 2, 3}, (k, m, S)
            assert len({x for blk in pout for x in blk}) >= 2, (k, m, S)
            w = min(k, m)
            differ = [din[b][:w] != pout[b][:w] for b in range(NB)]
            assert all(differ) if w > 1 else any(differ), (k, m, S, differ)


def _body(src, name, ret="int"):
    a = src.index("\n%s %s(" % (ret, name))
    return " ".join(src[a:src.index("\n}\n", a)].split())


def test_predicate_matches_source():
    """expected_form() is what launch_plan, launch_plan_crc and StripeRows::layout (launch_verify's
    test) say, and the host path rule of leg 4 is what encode_host_impl says: an edit to any of them
    fails here instead of silently retargeting the cases."""
    with open(os.path.join(CSRC, "rsmi_core.cpp")) as f:
        plan = _body(f.read(), "launch_plan")
    with open(os.path.join(CSRC, "rsmi_crc.cpp")) as f:
        crc_src = f.read()
    with open(os.path.join(CSRC, "rsmi_verify.cpp")) as f:
        ver_src = f.read()
    with open(os.path.join(CSRC, "rsmi_host.cpp")) as f:
        host = _body(f.read(), "encode_host_impl")
    with open(os.path.join(CSRC, "rsmi_impl.hpp")) as f:
        impl = f.read()
    plan_crc, verify = _body(crc_src, "launch_plan_crc"), _body(ver_src, "StripeRows::layout", "StripeLayout")
    scratch = _body(ver_src, "encode_into_scratch")
    launch = _body(ver_src, "launch_verify")
    impl1 = " ".join(impl.split())
    # the rows descriptor: the members in the header's order, and the one place that applies a block stride
    assert ("const uint8_t* data = nullptr; uint64_t data_rs = 0, data_bs = 0; const uint8_t* parity = nullptr; "
            "uint64_t parity_rs = 0, parity_bs = 0; uint64_t S = 0, nblocks = 0;") in impl1
    assert ("StripeRows r = *this; r.data += b0 * data_bs; r.parity += b0 * parity_bs; r.nblocks = nb; return r;"
            in impl1)
    assert "const StripeLayout layout = rows.layout();" in launch
    assert ("{&enc, &enc_rs, &enc_bs, &r.parity, &r.parity_rs, &r.parity_bs, &r.S, &m32, &r.nblocks, &badb}"
            in launch)
    assert ("const bool aligned = ((reinterpret_cast<uintptr_t>(in) | tba) % 16 == 0) && "
            "((reinterpret_cast<uintptr_t>(out) | tba) % 16 == 0) && in_rs % 16 == 0 && in_bs % 16 == 0 && "
            "out_rs % 16 == 0 && out_bs % 16 == 0 && in_rs >= round_up(S, 16) && out_rs >= round_up(S, 16) && "
            "S < (uint64_t(1) << 31);") in plan
    assert "const bool ua = !aligned && S >= 16 && S < (uint64_t(1) << 31) && in_rs >= S && out_rs >= S;" in plan
    assert ("const bool aligned = (reinterpret_cast<uintptr_t>(in) | tba) % 16 == 0 && "
            "(reinterpret_cast<uintptr_t>(out) | tba) % 16 == 0 && in_rs % 16 == 0 && in_bs % 16 == 0 && "
            "out_rs % 16 == 0 && out_bs % 16 == 0 && in_rs >= round_up(S, 16) && out_rs >= round_up(S, 16) && "
            "S < (size_t(1) << 31);") in plan_crc
    assert "const bool ua = !aligned && S >= 16 && S < (size_t(1) << 31) && in_rs >= S && out_rs >= S;" in plan_crc
    assert ("const bool aligned = reinterpret_cast<uintptr_t>(data) % 16 == 0 && "
            "reinterpret_cast<uintptr_t>(parity) % 16 == 0 && data_rs % 16 == 0 && data_bs % 16 == 0 && "
            "parity_rs % 16 == 0 && parity_bs % 16 == 0 && data_rs >= round_up(S, 16) && "
            "parity_rs >= round_up(S, 16) && S < (uint64_t(1) << 31);") in verify
    assert ("const bool ua = !aligned && S >= 16 && S < (uint64_t(1) << 31) && data_rs >= S && parity_rs >= S;"
            in verify)
    for body in (plan, plan_crc, verify):
        assert body.count("const bool aligned =") == 1 and body.count("const bool ua =") == 1
    assert "inline size_t round_up(size_t x, size_t a) { return (x + a - 1) / a * a; }" in impl
    # the fallback of the verify compares scratch rows at pitch round_up(S, 16) with the stored ones
    assert "const uint64_t Sp = round_up(rows.S, 16);" in scratch
    assert "const StripeRows sub = rows.from(b0, std::min(chunk, rows.nblocks - b0));" in scratch
    assert "fn(b0, sub, vs.p, Sp, m * Sp)" in scratch  # enc, enc_rs, enc_bs
    # the entry points hand the caller's six numbers on unchanged, in the header's order
    tail = ("d_data, data_shard_stride, data_block_stride, d_parity, parity_shard_stride, parity_block_stride, "
            "S, nblocks, ")
    assert " ".join(ver_src.split()).count(
        "return stripe_dev_call( c, " + tail + "d_bad_out, [&](const Plan& plan, const StripeRows& rows) { "
        "return launch_verify(c, plan, rows, d_bad_out,") == 1
    assert impl1.count("return launch(*plan, StripeRows{d_data, data_shard_stride, data_block_stride, d_parity, "
                       "parity_shard_stride, parity_block_stride, S, nblocks});") == 1
    assert " ".join(crc_src.split()).count("rc = launch_encode_crc(c, *plan, " + tail + "d_raw_out, st);") == 1
    # leg 4: small_path() below
    assert "const size_t total = nblocks * (k + m) * S;" in host
    assert ("if ((c->opt_zero_copy && pinned) || (total <= size_t(c->opt_small_bytes) && "
            "(2 * total <= size_t(c->opt_small_bytes) || in_pinned)))") in host
    assert "const bool pinned = in_pinned && host_alias(parity," in host


def _slip_base(k=10, m=4, S=1000):
    d, p = geometries(k, m, S)["A0"]
    ref = ref_of(k, m, S)
    host = blank(d, p, NB)
    put(host, d, ref.data)
    want = {a: x.copy() for a, x in host.items()}
    put(want, p, ref.parity)
    return d, p, ref, host, want


def _copy(bufs):
    return {a: x.copy() for a, x in bufs.items()}


def test_checker_rejects_simulated_slips():
    """The checker can fail: "got" buffers built on the CPU from the slips this module is there
    for are each rejected by check() / check_raw(), and the right image passes."""
    import rsmi

    k, m, S = 10, 4, 1000
    d, p, ref, host, want = _slip_base(k, m, S)
    good = _copy(host)
    put(good, p, ref.parity)
    check(good, want, ("good",))
    # parity rows laid at the data pitch (out_off taken from in_rs)
    got = _copy(host)
    put(got, p._replace(rs=d.rs), ref.parity)
    with pytest.raises(AssertionError):
        check(got, want, ("pitch",))
    # parity blocks laid at the data block stride
    got = _copy(host)
    put(got, p._replace(bs=d.bs), ref.parity, clip=True)
    with pytest.raises(AssertionError):
        check(got, want, ("block stride",))
    # one byte written at offset S of a parity row (a store one byte too long)
    got = _copy(good)
    got["p"][row_at(p, 1, 2) + S] = 0
    with pytest.raises(AssertionError):
        check(got, want, ("offset S",))
    # one byte changed in the data buffer, in a row and in the padding
    for o in (row_at(d, 2, 3) + 5, row_at(d, 0, 0) + S, 0, want["d"].size - 1):
        got = _copy(good)
        got["d"][o] ^= 1
        with pytest.raises(AssertionError):
            check(got, want, ("data", o))
    # the parity in the data's buffer (one allocation where there are two)
    got = _copy(host)
    put(got, p._replace(alloc="d"), ref.parity, clip=True)
    with pytest.raises(AssertionError):
        check(got, want, ("alloc",))
    # the same two slips where both sides share one allocation
    for gid in ("below", "interleaved"):
        dx, px = geometries(k, m, S)[gid]
        hx = blank(dx, px, NB)
        put(hx, dx, ref.data)
        wx = _copy(hx)
        put(wx, px, ref.parity)
        gx = _copy(hx)
        put(gx, px._replace(rs=dx.rs), ref.parity)
        with pytest.raises(AssertionError):
            check(gx, wx, (gid, "pitch"))

    # R(row) from the oracle's checksum: rsmi_crc16_entry is affine in raw over GF(2), so with an
    # empty head raw = checksum ^ entry(raw = 0)
    n = k + m
    r16 = np.array(ref.r16(), dtype=np.uint32) ^ np.uint32(rsmi.crc16_entry(b"", 0, S))
    assert rsmi.crc16_entry(b"", int(r16[0, 0]), S) == orc.crc16_ibm(ref.data[0, 0].tobytes())
    check_raw(rsmi, r16, ref.r16(), S, ("good",))
    # the table laid out as [b][k rows at n-stride from the wrong side]: the parity columns hold
    # R of the rows the data geometry finds there
    got = r16.copy()
    got[:, k:] = r16[:, :m]
    with pytest.raises(AssertionError):
        check_raw(rsmi, got, ref.r16(), S, ("wrong side",))
    # the parity columns at stride k + k instead of k + m: block b's land in block b's data columns
    got = r16.copy()
    flat = got.reshape(-1)
    flat[:] = 0xFFFFFFFF
    for b in range(NB):
        flat[b * n:b * n + k] = r16[b, :k]
    for b in range(NB):
        for j in range(m):
            if b * 2 * k + k + j < flat.size:
                flat[b * 2 * k + k + j] = r16[b, k + j]
    with pytest.raises(AssertionError):
        check_raw(rsmi, got, ref.r16(), S, ("stride",))
    # a row of the table never written
    got = r16.copy()
    got[2, n - 1] = 0xFFFFFFFF
    with pytest.raises(AssertionError):
        check_raw(rsmi, got, ref.r16(), S, ("unwritten",))


def small_path(zero_copy, data_pinned, parity_pinned, total, X):
    """The path choice of encode_host_impl, restated: true = one kernel over page-locked rows at
    pitch S (a pageable side staged by CPU copies), false = the copy-engine pipeline."""
    return bool((zero_copy and data_pinned and parity_pinned) or (total <= X and (2 * total <= X or data_pinned)))


HOST_K, HOST_M, HOST_S = 10, 4, 2049
HOST_TOTAL = NB * (HOST_K + HOST_M) * HOST_S
# (data page-locked, parity page-locked, small_call_bytes, one kernel?)
HOST_CASES = [
    (False, True, 2 * HOST_TOTAL, True),        # 2 * total <= X: only the input staged
    (False, True, 2 * HOST_TOTAL - 1, False),   # X / 2 < total <= X, data pageable: the pipeline
    (False, True, HOST_TOTAL, False),
    (False, True, HOST_TOTAL - 1, False),       # total > X
    (True, False, 2 * HOST_TOTAL - 1, True),    # X / 2 < total <= X, data page-locked: only the output staged
    (True, False, HOST_TOTAL, True),
    (True, False, HOST_TOTAL - 1, False),       # total > X
]
HOST_IDS = ["parity-locked-2t", "parity-locked-2t-1", "parity-locked-t", "parity-locked-t-1",
            "data-locked-2t-1", "data-locked-t", "data-locked-t-1"]


def test_host_cases_follow_the_rule():
    for dp, pp, X, one in HOST_CASES:
        assert small_path(1, dp, pp, HOST_TOTAL, X) == one, (dp, pp, X)
    assert HOST_S % 2 == 1 and 2 * HOST_TOTAL < 2 << 20 and NB * fused_units(HOST_S) <= 64


# ---------------------------------------------------------------- GPU plumbing
SEEN = collections.Counter()
LEGS = set()
ALL_LEGS = {"encode", "reconstruct", "crc", "crc-two-launch", "verify", "host"}
REQUIRED = {"fn", "crc", "fused", "inl", "ua", "ua_crc", "fused_ua", "ua_inl", "generic",
            "rs_verify_kernel", "rs_verify_kernel,UA", "rs_compare_rows_kernel"}
T0 = []


def seen(label):
    if label.startswith("rs_verify_kernel"):
        SEEN["rs_verify_kernel,UA" if label.endswith(",UA") else "rs_verify_kernel"] += 1
    elif label.startswith("rs_generic_kernel"):
        SEEN["generic"] += 1
    elif label.startswith("rs_fast_kernel"):
        ua, crc = ",UA" in label, ",CRC" in label
        SEEN[("ua_crc" if ua else "crc") if crc else ("ua" if ua else "fn")] += 1
    elif label.startswith("rs_fused_mfma_kernel"):
        ua, inl = ",UA" in label, ",INL" in label
        SEEN[("ua_inl" if ua else "inl") if inl else ("fused_ua" if ua else "fused")] += 1
    else:
        SEEN[label] += 1


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    rsmi = pytest.importorskip("rsmi")
    if not torch.cuda.is_available() or rsmi.device_count() == 0:
        pytest.skip("no GPU")
    T0.append(time.perf_counter())
    yield torch, rsmi
    _REFS.clear()
    print("\nlayout contract: families run and asserted by label (calls):",
          ", ".join("%s %d" % kv for kv in sorted(SEEN.items())))
    print("layout contract: wall seconds of the GPU legs: %.2f" % (time.perf_counter() - T0[0]))
    if LEGS == ALL_LEGS:  # the whole module ran: every family the module is there for was reached
        assert REQUIRED <= set(SEEN), sorted(REQUIRED - set(SEEN))


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def upload(torch, bufs):
    dev = {a: torch.from_numpy(x.copy()).cuda() for a, x in bufs.items()}
    for t in dev.values():
        assert t.data_ptr() % 16 == 0
    return dev


def dptr(dev, side):
    return dev[side.alloc].data_ptr() + GUARD + side.off


def download(dev):
    return {a: t.cpu().numpy() for a, t in dev.items()}


def form_on_device(dev, d, p, S, form):
    """The form from the pointers the call really gets is the one cases() worked out."""
    got = expected_form(dptr(dev, d), d.rs, d.bs, dptr(dev, p), p.rs, p.bs, S)
    assert got == form, (got, form)
    return got


# ---------------------------------------------------------------- leg 1: rsmi_encode_batch_dev
@pytest.mark.gpu
@pytest.mark.parametrize("k,m", SHAPES)
def test_encode_independent_layouts(gpu, k, m):
    """Every geometry at its sizes through rsmi_encode_batch_dev: the label the predicate gives
    (each T-* case the ",UA" kernel, or rs_generic_kernel at S = 15), the data buffer byte for
    byte, the parity buffer the oracle's rows with every guard, gap and padding byte unchanged."""
    torch, rsmi = gpu
    LEGS.add("encode")
    with rsmi.Codec(k, m) as c:
        for gid, S, d, p, form in cases(k, m):
            ctx = (k, m, gid, S)
            ref = ref_of(k, m, S)
            host = blank(d, p, NB)
            put(host, d, ref.data)
            want = _copy(host)
            put(want, p, ref.parity)
            dev = upload(torch, host)
            form_on_device(dev, d, p, S, form)
            label = encode_label(k, m, form)
            c.encode_batch_dev(dptr(dev, d), d.rs, d.bs, dptr(dev, p), p.rs, p.bs, S, NB, _stream(torch))
            torch.cuda.synchronize()
            assert c.last_kernel() == label, (c.last_kernel(), label) + ctx
            check(download(dev), want, ctx)
            seen(label)


@pytest.mark.gpu
@pytest.mark.parametrize("k,m,lost", [(10, 4, [0]), (16, 4, [1, 17])], ids=["10-4", "16-4"])
def test_reconstruct_single_terms(gpu, k, m, lost):
    """rsmi_reconstruct_batch_dev has one side, so only the single-term cases apply: from an
    aligned layout, base + 8, shard_stride + 8 and block_stride + 8 each run the ",UA" kernel and
    the aligned layout the aligned one; the whole buffer is compared."""
    torch, rsmi = gpu
    LEGS.add("reconstruct")
    n = k + m
    present = [i not in lost for i in range(n)]
    with rsmi.Codec(k, m) as c:
        for S in (1000, 2049):
            R = round_up(S, 16)
            rs = R + 16
            bs = n * rs + 32
            ref = ref_of(k, m, S)
            full = np.concatenate([ref.data, ref.parity], axis=1)
            for name, side in (("aligned", Side("x", 64, rs, bs)), ("base8", Side("x", 72, rs, bs)),
                               ("rs8", Side("x", 64, rs + 8, round_up(n * (rs + 8), 16) + 32)),
                               ("bs8", Side("x", 64, rs, bs + 8))):
                ctx = (k, m, S, name)
                form = expected_form(GUARD + side.off, side.rs, side.bs, GUARD + side.off, side.rs, side.bs, S)
                assert form == ("aligned" if name == "aligned" else "ua"), ctx
                t = terms(side, side, S)
                assert sum(not x for x in t) == (0 if name == "aligned" else 2), ctx  # one term, on both "sides"
                want = {"x": np.full(GUARD + side.off + NB * side.bs + GUARD, FILL_DATA, dtype=np.uint8)}
                put(want, side, full)
                host = _copy(want)
                erased = full.copy()
                erased[:, lost] = 0xEE
                put(host, side, erased)
                dev = upload(torch, host)
                label = fast_label(k, len(lost), ua=form == "ua")
                assert "MT=%d,NT=%d>" % (len(lost), nt_of(k, len(lost))) in label
                c.reconstruct_batch_dev(dptr(dev, side), side.rs, side.bs, S, NB, present, False, _stream(torch))
                torch.cuda.synchronize()
                assert c.last_kernel() == label, (c.last_kernel(), label) + ctx
                check(download(dev), want, ctx)
                seen(label)


# ---------------------------------------------------------------- leg 2: rsmi_encode_batch_dev_crc
def _crc_case(torch, rsmi, c, k, m, S, nb, gid, d, p, form, fold):
    ctx = (k, m, gid, S, nb, fold)
    n = k + m
    ref = ref_of(k, m, S, nb)
    host = blank(d, p, nb)
    put(host, d, ref.data)
    want = _copy(host)
    put(want, p, ref.parity)
    dev = upload(torch, host)
    form_on_device(dev, d, p, S, form)
    raw = torch.full((nb, n), -1, dtype=torch.int32, device="cuda")
    label = crc_label(k, m, S, nb, form, fold)
    c.encode_batch_dev_crc(dptr(dev, d), d.rs, d.bs, dptr(dev, p), p.rs, p.bs, S, nb, raw.data_ptr(), _stream(torch))
    torch.cuda.synchronize()
    assert c.last_kernel() == label, (c.last_kernel(), label) + ctx
    check(download(dev), want, ctx)
    check_raw(rsmi, raw.cpu().numpy(), ref.r16(), S, ctx)
    seen(label)
    return label


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", SHAPES)
def test_encode_crc_independent_layouts(gpu, k, m):
    """The same cases through rsmi_encode_batch_dev_crc: both buffers as in leg 1 and R(row) of
    all k + m rows.  crc16_fused_fold 1: rs_fused_mfma_kernel, combined in the kernel (",INL") for
    the shapes that have that form; 0: the ",CRC" kernels.  (5,5), (7,2), (20,4) and S = 15
    unaligned: the encode, then launch_crc over the data rows with the data geometry and over the
    parity rows with the parity geometry (the label stays the encode's)."""
    torch, rsmi = gpu
    LEGS.add("crc")
    labels = set()
    for fold in (1, 0):
        with rsmi.Codec(k, m) as c:
            c.set_option("crc16_fused_fold", fold)
            for gid, S, d, p, form in cases(k, m):
                labels.add(_crc_case(torch, rsmi, c, k, m, S, NB, gid, d, p, form, fold))
    if (k, m) in ((10, 4), (16, 4)):
        for sfx in (",INL", ",UA,INL", ",CRC", ",UA,CRC"):
            assert any(x.endswith(">" + sfx) for x in labels), (sfx, sorted(labels))
        assert generic_label(k, m) in labels  # S = 15 unaligned: the separate pass
    if (k, m) in ((5, 5), (7, 2), (20, 4)):
        assert not any("fused" in x or ",CRC" in x for x in labels), sorted(labels)


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", [(10, 4), (16, 4)])
def test_encode_crc_two_launch_form(gpu, k, m):
    """More than 64 units in the launch (65 blocks of S = 1040, one unit each; S = 1041 for the
    unaligned cases): fused / fused_ua with the separate combine launch, which reads the records
    by block and writes raw[b * (k + m) + r] for 65 blocks."""
    torch, rsmi = gpu
    LEGS.add("crc-two-launch")
    nb = 65
    with rsmi.Codec(k, m) as c:
        for S, ids in ((1040, ALIGNED_IDS), (1041, ["T-prs8", "T-dbase1", "split-in", "split-out", "phases"])):
            assert nb * fused_units(S) == 65
            g = geometries(k, m, S, nb)
            for gid in ids:
                d, p = g[gid]
                form = expected_form(GUARD + d.off, d.rs, d.bs, GUARD + p.off, p.rs, p.bs, S)
                assert form == ("aligned" if S == 1040 else "ua")
                label = _crc_case(torch, rsmi, c, k, m, S, nb, gid, d, p, form, 1)
                assert ",INL" not in label and label.startswith("rs_fused_mfma_kernel")


# ---------------------------------------------------------------- leg 3: rsmi_verify_batch_dev
def _verify(torch, c, dev, host, d, p, S, m, label, ctx):
    """One rsmi_verify_batch_dev over what dev holds (= host): the flags (NB, m) as bool.  The
    flags start poisoned, the label must match, both buffers must come back byte for byte."""
    bad = torch.full((NB * m,), 0x5EED, dtype=torch.int32, device="cuda")
    c.verify_batch_dev(dptr(dev, d), d.rs, d.bs, dptr(dev, p), p.rs, p.bs, S, NB, bad.data_ptr(), _stream(torch))
    torch.cuda.synchronize()
    assert c.last_kernel() == label, (c.last_kernel(), label) + ctx
    check(download(dev), host, ctx + ("verify wrote to the shards",))
    return bad.cpu().numpy().reshape(NB, m) != 0


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", SHAPES)
def test_verify_independent_layouts(gpu, k, m):
    """The same cases through rsmi_verify_batch_dev on the oracle's stripes, data and parity in
    their own allocations, pitches and block strides: clean stripes raise no flag; byte 0 and byte
    S - 1 of one parity row raise exactly bad[b * m + j]; one data byte raises the m flags of its
    block and no other; a byte at offset S of a parity row or a data row, where the pitch leaves
    one, raises none.  rs_verify_kernel aligned and ",UA" for the shapes that have it,
    rs_compare_rows_kernel (scratch rows at pitch round_up(S, 16) against stored rows at
    parity_shard_stride) for (7,2), (20,4) and S = 15 unaligned."""
    torch, rsmi = gpu
    LEGS.add("verify")
    with rsmi.Codec(k, m) as c:
        M = np.frombuffer(c.encode_matrix(), dtype=np.uint8).reshape(k + m, k)
        assert (M[k:] != 0).all()  # one damaged data byte changes every parity row
        for gid, S, d, p, form in cases(k, m):
            ctx = (k, m, gid, S)
            ref = ref_of(k, m, S)
            clean = blank(d, p, NB)
            put(clean, d, ref.data)
            put(clean, p, ref.parity)
            dev = upload(torch, clean)
            form_on_device(dev, d, p, S, form)
            label = verify_label(k, m, form)
            got = _verify(torch, c, dev, clean, d, p, S, m, label, ctx)
            assert not got.any(), ctx + (got,)
            b, j, r = 1, m - 1, k // 2
            none = np.zeros((NB, m), dtype=bool)
            one = none.copy()
            one[b, j] = True
            blk = none.copy()
            blk[b, :] = True
            damage = [(p, row_at(p, b, j), one), (p, row_at(p, b, j) + S - 1, one),
                      (d, row_at(d, b, r) + S // 2, blk), (d, row_at(d, b, k - 1) + S - 1, blk)]
            if p.rs > S:
                damage.append((p, row_at(p, b, j) + S, none))
            if d.rs > S:
                damage.append((d, row_at(d, b, r) + S, none))
            for side, o, want in damage:
                host = _copy(clean)
                host[side.alloc][o] ^= 0x21
                dev[side.alloc].copy_(torch.from_numpy(host[side.alloc]))
                got = _verify(torch, c, dev, host, d, p, S, m, label, ctx + (side.alloc, o))
                assert np.array_equal(got, want), ctx + (side.alloc, o, got)
                dev[side.alloc].copy_(torch.from_numpy(clean[side.alloc]))
            seen(label)


# ---------------------------------------------------------------- leg 4: the host small-call path, one side page-locked
class HostBuf:
    """nb blocks of nrows rows of S bytes at block stride bs, 64 guard bytes before and after, in
    pageable or page-locked (rsmi_host_alloc) memory."""

    def __init__(self, rsmi, nrows, S, bs, fill, pinned, nb=NB):
        self.rsmi, self.side, self.nrows = rsmi, Side("h", 0, S, bs), nrows
        size = GUARD + nb * bs + GUARD
        self.p = None
        if pinned:
            self.p = rsmi.lib().rsmi_host_alloc(size)
            assert self.p
            self.a = np.ctypeslib.as_array((ctypes.c_uint8 * size).from_address(self.p))
        else:
            self.a = np.empty(size, dtype=np.uint8)
        self.a[:] = fill
        self.ptr = (self.p or self.a.ctypes.data) + GUARD

    def free(self):
        self.a = None
        if self.p:
            self.rsmi.lib().rsmi_host_free(self.p)
            self.p = None


@pytest.mark.gpu
@pytest.mark.parametrize("data_pinned,parity_pinned,X,one_kernel", HOST_CASES, ids=HOST_IDS)
def test_host_small_call_one_side_page_locked(gpu, data_pinned, parity_pinned, X, one_kernel):
    """rsmi_encode_batch_host and rsmi_encode_batch_host_crcs (both outputs), RS(10,4), S = 2049,
    3 blocks with gaps (dbs = k*S + 24, pbs = m*S + 40), one side from rsmi_host_alloc, zero_copy
    1, on both sides of each threshold of encode_host_impl's rule (small_path above; leg 0 pins
    its text).  encode_small stages only the pageable side, so the one kernel runs with the
    caller's block stride on one side and the staging's k*S / m*S on the other, in two allocations:
    its label ends ",UA" (",UA,INL" with the CRC-16 fused in).  The pipeline codes pitched device
    rows: no ",UA".  Parity, gaps and guards over the whole buffers; R(row) and R32(row) of every
    row.  The same rule of verify_host_impl is pinned by test_verify_host.py::test_mixed_memory,
    and the pipeline's own branches for mixed memory above the small-call limit by
    test_host_pipeline.py::test_encode_zc_writeback and ::test_encode_zin_upload_linear_writeback:
    those sub-cases are not repeated here."""
    torch, rsmi = gpu
    LEGS.add("host")
    k, m, S = HOST_K, HOST_M, HOST_S
    n = k + m
    assert small_path(1, data_pinned, parity_pinned, HOST_TOTAL, X) == one_kernel
    ref = ref_of(k, m, S)
    db = HostBuf(rsmi, k, S, k * S + 24, FILL_DATA, data_pinned)
    pb = HostBuf(rsmi, m, S, m * S + 40, FILL_PARITY, parity_pinned)
    try:
        put({"h": db.a}, db.side, ref.data)
        want_d = db.a.copy()
        want_p = np.full(pb.a.size, FILL_PARITY, dtype=np.uint8)
        put({"h": want_p}, pb.side, ref.parity)
        with rsmi.Codec(k, m) as c:
            c.set_option("zero_copy", 1)
            c.set_option("small_call_bytes", X)
            for crcs in (False, True):
                ctx = (data_pinned, parity_pinned, X, crcs)
                pb.a[:] = FILL_PARITY
                if crcs:
                    raw16 = np.full((NB, n), 0xA5A5A5A5, dtype=np.uint32)
                    raw32 = np.full((NB, n), 0xA5A5A5A5, dtype=np.uint32)
                    c.encode_batch_host_crcs_ptr(db.ptr, db.side.bs, pb.ptr, pb.side.bs, S, NB, raw16.ctypes.data,
                                                 raw32.ctypes.data)
                    label = fused_label(k, m, S, NB, ua=one_kernel)
                    assert label.endswith(",UA,INL" if one_kernel else ">,INL")
                else:
                    c.encode_batch_host_ptr(db.ptr, db.side.bs, pb.ptr, pb.side.bs, S, NB)
                    label = fast_label(k, m, ua=one_kernel)
                    assert label.endswith(",UA") == one_kernel
                assert c.last_kernel() == label, (c.last_kernel(), label) + ctx
                check({"d": db.a, "p": pb.a}, {"d": want_d, "p": want_p}, ctx)
                if crcs:
                    check_raw(rsmi, raw16, ref.r16(), S, ctx)
                    for b in range(NB):
                        for r in range(n):
                            assert rsmi.crc32_entry(b"", int(raw32[b, r]), S) == ref.r32()[b][r], ctx + ("crc32", b, r)
                seen(label)
    finally:
        db.free()
        pb.free()
