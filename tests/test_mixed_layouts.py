"""The layout contract of the in-place mixed reconstruct, bit for bit.

include/rsmi.h gives rsmi_reconstruct_mixed_batch_dev one side: row i of block b at
d_shards + b*block_stride + i*shard_stride.  test_mixed_reconstruct.py calls it through two
geometries only (test_verify.Lay: pitched rows from an aligned base, or rows back to back at pitch
S one byte off), where in_off / out_off taken from S, a dropped "* rs" or bs and rs swapped give the
right address in every unaligned case.  Here the geometries are test_layout_contract's, for one
side: a case is Side("x", off, rs, bs), off counted behind the 64 leading guard bytes; the buffer
is filled with 0xA5, missing rows hold MISSING, and after every call the whole buffer is compared
with the definition's image (test_mixed_reconstruct.definition: oracle_lib.reconstruct per block
under that block's masks), together with the per-block statuses and rsmi_last_kernel.  There are
no tolerances.

  0  CPU: the geometries are well formed and have the form they are there for; the predicate, the
     launch order and the kernels' K are pinned to the source; the comparison rejects simulated slips
  1  every geometry x its sizes x every shape of test_layout_contract.SHAPES
  2  per-block required masks, and data_only
  3  equality with rsmi_reconstruct_rows_batch_dev
  4  waves_per_cu = 1 at a pitch that is not S: 240 blocks, and 1200 blocks, whose class launches
     have more tiles than a 256-CU device has waves under the cap, so the strided walk restages
"""
import collections
import os
import re

import numpy as np
import pytest

import oracle_lib as orc
from test_kernel_matrix import KS, fast_label, generic_label
from test_layout_contract import (ALIGNED_S, FILL_DATA, GUARD, S_SHORT, SHAPES, UA_S, Side, _body, put, round_up,
                                  row_at)
from test_mixed_reconstruct import (MIXED_CPP, SEAM, TOO_FEW, definition, junk_unused_survivor, mixed_label,
                                    present_of, same_bytes, stored, u8, wanted)
from test_verify import stripes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "filedag-storage_amd", "csrc")

NB = 6
IDS = ["A0", "T-base8", "T-base1", "T-rs8", "T-bs8", "split", "phases", "transposed", "transposed-ua"]
T_IDS = ["T-base8", "T-base1", "T-rs8", "T-bs8"]
ALIGNED_IDS = ["A0", "transposed"]
SHORT_IDS = ["T-base8", "phases", "transposed-ua"]
ALL_S = sorted(set(ALIGNED_S + UA_S + [S_SHORT]))
REQUIRED_SHAPES = [(10, 4), (16, 4), (4, 2)]   # leg 2
WALK_SHAPE, WALK_S, WALK_IDS = (10, 4), 2049, ["T-rs8", "phases"]   # leg 4
WALK_REPS = [40, 200]      # the sheet repeated; 200: every class launch is capped on 256 CUs
WALK_CUS = 256             # the MI355X


# ---------------------------------------------------------------- the geometry model
def geometries(k, m, S, nb=NB):
    """id -> Side: row i of block b at GUARD + off + b*bs + i*rs of the one buffer."""
    n = k + m
    R = round_up(S, 16)

    def side(off=64, rs=R + 16, bs=None):
        return Side("x", off, rs, round_up(n * rs, 16) + 32 if bs is None else bs)

    g = collections.OrderedDict()
    g["A0"] = side()
    # A0 with exactly one term of the predicate broken
    g["T-base8"] = side(off=64 + 8)
    g["T-base1"] = side(off=64 + 1)
    g["T-rs8"] = side(rs=R + 24)
    g["T-bs8"] = side(bs=side().bs + 8)
    # the Split layout: rows back to back at pitch S
    g["split"] = Side("x", 0, S, n * S)
    # every row at its own byte phase
    g["phases"] = Side("x", 3, S + 1, n * (S + 1) + 5)
    # block_stride < shard_stride: row i of all blocks is contiguous
    bs = R + 16
    g["transposed"] = Side("x", 64, nb * bs, bs)
    g["transposed-ua"] = Side("x", 64, nb * (S + 1) + 3, S + 1)
    assert list(g) == IDS
    return g


def extent(side, n, S, nb):
    """Bytes from the first row's first byte to the end of the layout."""
    return max(nb * side.bs, (nb - 1) * side.bs + (n - 1) * side.rs + S)


def buf_size(side, n, S, nb):
    return GUARD + side.off + extent(side, n, S, nb) + GUARD


def terms(side, S, base=0):
    """The four terms of the predicate for one side, for an allocation at base (mod 16)."""
    return ((base + GUARD + side.off) % 16 == 0, side.rs % 16 == 0, side.bs % 16 == 0, side.rs >= round_up(S, 16))


def expected_form(ptr, rs, bs, S):
    """stripe_layout(base, rs, bs, base, rs, bs, S) as launch_mixed calls it, written out here on
    purpose: aligned, else the unaligned-window kernels for rows of at least 16 bytes, else neither
    (every block goes through launch_plan, which then runs the byte-granular kernel)."""
    if ptr % 16 == 0 and rs % 16 == 0 and bs % 16 == 0 and rs >= round_up(S, 16) and S < 2 ** 31:
        return "aligned"
    if S >= 16 and S < 2 ** 31 and rs >= S:
        return "ua"
    return "generic"


def sizes_of(gid):
    if gid == "split":
        return sorted(set(ALIGNED_S + UA_S))
    if gid in ALIGNED_IDS:
        return ALIGNED_S
    return UA_S + ([S_SHORT] if gid in SHORT_IDS else [])


def cases(k, m, nb=NB):
    """(id, S, side, expected form) of every case of a shape; the form assumes a 16-byte-aligned
    allocation (the GPU legs assert that of each tensor)."""
    for S in ALL_S:
        for gid, side in geometries(k, m, S, nb).items():
            if S in sizes_of(gid):
                yield gid, S, side, expected_form(GUARD + side.off, side.rs, side.bs, S)


# ---------------------------------------------------------------- the block sheet
def sheet(k, m):
    """The lost rows of the 6 blocks of a call.  No list index equals a block index (class 1 holds
    blocks 1 and 5 at indices 0 and 1), and block 0, whose address has no block-stride term, has
    no work."""
    n = k + m
    assert k >= 2
    order = [k - 1, n - 1, 0, k, 1]
    assert len(set(order)) == min(5, n)
    nl3 = m if m > 4 else min(m, 3)   # (5,5): 5 rows, a two-tile plan beside the fast blocks
    losses = [(), (0,), (1, k) if m >= 2 else (k,), tuple(sorted(order[:nl3])), tuple(range(m + 1)), (k - 1,)]
    assert len(losses[3]) == nl3 and len(losses[4]) == m + 1 and losses[1] != losses[5]
    return losses


def last_tile_mt(rows):
    """A plan cuts its rows into tiles of at most 4; a launch_plan's label is the last tile's."""
    return rows - 4 * ((rows - 1) // 4)


def expected_label(k, rows, form, seg=SEAM):
    """The label rule of launch_mixed, restated.  rows[b]: the rows the call rebuilds in block b
    (0: nothing to do, or too few present).  Per segment of seg blocks: the classes 1..4 launch in
    ascending order, then the fallback's runs in block order, so the last launch of the call is
    the last segment's last fallback run's last tile, or without a fallback block there the
    highest class that has a block there.  None: nothing is launched."""
    rows = np.asarray(rows)
    has_class = form != "generic" and k in KS
    last = None
    for s0 in range(0, rows.size, seg):
        r = rows[s0:s0 + seg]
        fast = (r > 0) & (r <= 4) if has_class else np.zeros(r.size, dtype=bool)
        back = np.flatnonzero((r > 0) & ~fast)
        if back.size:
            mt = last_tile_mt(int(r[back[-1]]))
            last = generic_label(k, mt) if not has_class else fast_label(k, mt, ua=form == "ua")
        elif fast.any():
            last = mixed_label(k, int(r[fast].max()), form == "aligned")
    return last


def rows_rebuilt(k, present, W):
    """Per block, the rows the call writes: W's, and none where fewer than k rows are present."""
    return np.where(present.sum(axis=1) >= k, W.sum(axis=1), 0)


_CASES = {}


def required_draw(k, m, nb=NB):
    """A fixed per-block required mask for the sheet's blocks: two rows in three are named."""
    return np.random.default_rng(7100 + 100 * k + m).random(size=(nb, k + m)) < 2.0 / 3


def sheet_case(k, m, S, required=False, data_only=False):
    """Everything the sheet's call needs at one size, the definition's answers included: computed
    once, read-only."""
    key = (k, m, S, required, data_only)
    if key not in _CASES:
        losses = sheet(k, m)
        present = present_of(k + m, losses)
        sh = stored(stripes(k, m, S, NB), present)
        junk_unused_survivor(k, sh, present)
        req = required_draw(k, m) if required else None
        W = wanted(k, present, req, data_only)
        status, image = definition(k, m, sh, present, W)
        for a in (present, sh, W, image):
            a.setflags(write=False)
        _CASES[key] = dict(present=present, sh=sh, required=req, W=W, status=status, image=image,
                           rows=rows_rebuilt(k, present, W))
    return _CASES[key]


def render(side, n, S, nb, rows):
    """The buffer of a case with rows[b, i] in place and the fill sentinel everywhere else."""
    buf = np.full(buf_size(side, n, S, nb), FILL_DATA, dtype=np.uint8)
    put({"x": buf}, side, rows)
    return buf


def compare(got_status, got_buf, got_label, want_status, want_buf, want_label, ctx):
    """The module's comparison: the statuses, the label and the whole buffer."""
    assert list(got_status) == list(want_status), (ctx, list(got_status), list(want_status))
    assert got_label == want_label, (ctx, got_label, want_label)
    assert got_buf.dtype == np.uint8 and got_buf.shape == want_buf.shape, ctx
    same_bytes(got_buf, want_buf, ctx)


# ---------------------------------------------------------------- leg 0 (CPU)
@pytest.mark.parametrize("k,m", SHAPES)
def test_geometries_are_well_formed(k, m):
    """No two rows overlap, every row lies between the guards, each T-* case breaks exactly one
    term of the predicate relative to A0, and every id has the form it is there for."""
    n = k + m
    for nb in [NB] + [NB * reps for reps in WALK_REPS]:
        for gid, S, side, form in cases(k, m, nb):
            if nb > NB and ((k, m) != WALK_SHAPE or S != WALK_S or gid not in WALK_IDS):
                continue   # leg 4 alone uses more than 6 blocks
            ctx = (k, m, nb, gid, S)
            size = buf_size(side, n, S, nb)
            assert side.rs >= S and size <= 64 << 20, ctx
            spans = sorted((row_at(side, b, r), row_at(side, b, r) + S) for b in range(nb) for r in range(n))
            assert GUARD <= spans[0][0] and spans[-1][1] <= size - GUARD, ctx
            for (_, hi0), (lo1, _) in zip(spans, spans[1:]):
                assert hi0 <= lo1, ctx
            if gid in ALIGNED_IDS:
                assert form == "aligned", ctx
            elif gid == "split":
                assert form == ("aligned" if S % 16 == 0 else "ua"), ctx
            else:
                assert form == ("generic" if S < 16 else "ua"), ctx
            if gid.startswith("transposed"):
                assert side.bs < side.rs and side.rs >= nb * side.bs, ctx
                assert row_at(side, 1, 0) - row_at(side, 0, 0) < row_at(side, 0, 1) - row_at(side, 0, 0), ctx
            else:
                assert side.bs >= n * side.rs, ctx
            if gid != "split":
                # room for the byte at offset S of a row; the pitch is not the row length
                assert side.rs > S and side.bs != n * S, ctx
    broken = set()
    for S in ALL_S:
        g = geometries(k, m, S)
        a0 = terms(g["A0"], S)
        assert all(a0), (k, m, S)
        for gid in T_IDS:
            t = terms(g[gid], S)
            diff = [i for i in range(len(t)) if t[i] != a0[i]]
            assert len(diff) == 1 and diff[0] < 3, (k, m, S, gid, diff)
            broken.add(diff[0])
            if gid.endswith("8"):
                assert all(x % 8 == 0 for x in (GUARD + g[gid].off, g[gid].rs, g[gid].bs)), (S, gid)
    assert broken == {0, 1, 2}
    forms = collections.defaultdict(set)
    for gid, S, _, form in cases(k, m):
        forms[form].add(S)
    assert sorted(forms["aligned"]) == sorted(ALIGNED_S) and sorted(forms["ua"]) == sorted(set(UA_S + [1000]))
    assert sorted(forms["generic"]) == [S_SHORT]
    assert sorted({g for g, S, _, f in cases(k, m) if f == "generic"}) == sorted(SHORT_IDS)


@pytest.mark.parametrize("k,m", SHAPES)
def test_sheet_is_what_it_is_there_for(k, m):
    """The block sheet: the statuses, the classes and the fallback blocks of every shape, and the
    required draw of leg 2 names present rows, leaves out missing ones and leaves work."""
    n = k + m
    c = sheet_case(k, m, 17)
    assert c["status"] == [0, 0, 0, 0, TOO_FEW, 0]
    assert c["rows"].tolist() == [0, 1, min(m, 2), m if m > 4 else min(m, 3), 0, 1]
    # class 1 holds two entries with different plans, at list indices 0 and 1 and blocks 1 and 5
    ones = np.flatnonzero(c["rows"] == 1).tolist()
    assert ones[0] == 1 and ones[-1] == 5
    assert not np.array_equal(c["present"][1], c["present"][5])
    for mt in (1, 2, 3, 4):
        for j, b in enumerate(np.flatnonzero(c["rows"] == mt)):
            assert j != b
    if (k, m) == (5, 5):
        assert c["rows"][3] == 5 and expected_label(k, c["rows"], "ua") == fast_label(5, 1, ua=True)
        assert expected_label(k, c["rows"], "generic") == generic_label(5, 1)
    elif k in KS:
        assert expected_label(k, c["rows"], "aligned") == mixed_label(k, int(c["rows"].max()), True)
        assert expected_label(k, c["rows"], "ua") == mixed_label(k, int(c["rows"].max()), False)
        assert expected_label(k, c["rows"], "generic") == generic_label(k, 1)
    else:
        assert expected_label(k, c["rows"], "aligned") == expected_label(k, c["rows"], "ua") == generic_label(k, 1)
    # a junk survivor exists wherever a block has more than k rows present
    full = stripes(k, m, 17, NB)
    junk = [b for b in range(NB) if (c["sh"][b][c["present"][b]] != full[b][c["present"][b]]).any()]
    assert junk == [b for b in range(NB) if c["present"][b].sum() > k]
    if (k, m) in REQUIRED_SHAPES:
        req = required_draw(k, m)
        r = sheet_case(k, m, 17, required=True)
        assert (req & c["present"]).any() and (~req & ~c["present"]).any(), (k, m)
        assert len(set(r["rows"].tolist())) >= 3 and not np.array_equal(r["rows"], c["rows"]), (k, m, r["rows"])
    assert expected_label(k, np.zeros(NB, dtype=int), "aligned") is None
    assert n <= 24


def test_rule_matches_source():
    """expected_form() is what StripeRows::layout says for the rows launch_mixed gives it, and
    expected_label() relies on what launch_mixed does: per segment of 2^22 blocks, the classes in
    ascending MT, behind them the fallback's runs in block order; a class for the K of
    fill_mixed_k and one-tile plans only."""
    with open(os.path.join(CSRC, "rsmi_verify.cpp")) as f:
        layout = _body(f.read(), "StripeRows::layout", "StripeLayout")
    with open(MIXED_CPP) as f:
        mixed = _body(f.read(), "launch_mixed")
    with open(os.path.join(CSRC, "rs_mixed_kernels.hip")) as f:
        kernels = f.read()
    with open(os.path.join(CSRC, "rsmi_impl.hpp")) as f:
        impl = f.read()
    assert ("const bool aligned = reinterpret_cast<uintptr_t>(data) % 16 == 0 && "
            "reinterpret_cast<uintptr_t>(parity) % 16 == 0 && data_rs % 16 == 0 && data_bs % 16 == 0 && "
            "parity_rs % 16 == 0 && parity_bs % 16 == 0 && data_rs >= round_up(S, 16) && "
            "parity_rs >= round_up(S, 16) && S < (uint64_t(1) << 31);") in layout
    assert ("const bool ua = !aligned && S >= 16 && S < (uint64_t(1) << 31) && data_rs >= S && parity_rs >= S;"
            in layout)
    assert "return aligned ? StripeLayout::kAligned : ua ? StripeLayout::kUA : StripeLayout::kNeither;" in layout
    assert "inline size_t round_up(size_t x, size_t a) { return (x + a - 1) / a * a; }" in impl
    assert "const StripeLayout layout = StripeRows{base, rs, bs, base, rs, bs, S, nb}.layout();" in mixed
    assert ("const uint8_t* data = nullptr; uint64_t data_rs = 0, data_bs = 0; const uint8_t* parity = nullptr; "
            "uint64_t parity_rs = 0, parity_bs = 0; uint64_t S = 0, nblocks = 0;") in " ".join(impl.split())
    assert "const bool aligned = layout == StripeLayout::kAligned;" in mixed
    assert ("const bool fast = layout != StripeLayout::kNeither && pl.tiles.size() == 1 && t.K == K && K <= 16 && "
            "(aligned ? mixed_kernels().fn : mixed_kernels().ua)[K][t.MT] != nullptr;") in mixed
    assert "cls[p] = fast ? t.MT : kFallback;" in mixed
    assert [int(x) for x in re.findall(r"fill_mixed_k<(\d+)>\(x\);", kernels)] == KS
    assert re.findall(r"fill_mixed_km<K, (\d)>\(t\);", kernels) == ["1", "2", "3", "4"]
    assert ("const uint64_t seg = std::min<uint64_t>(std::max<uint64_t>(1, uint64_t(c->opt_launch_units_max) / tpb), "
            "uint64_t(1) << 22);") in mixed
    assert mixed.count("const uint64_t seg =") == 1 and "<< 31" not in mixed
    # option launch_units_max defaults to 2^24 - 1 tiles: 2^22 blocks is the smaller arm while a
    # block has at most 3 tiles, as every segment expected_label counts on has
    assert "constexpr uint64_t kLaunchUnitsDefault = (uint64_t(1) << 24) - 1;" in impl
    assert "std::atomic<long> opt_launch_units_max{long(rsmi::impl::kLaunchUnitsDefault)};" in impl
    assert ((1 << 24) - 1) // 3 >= SEAM
    assert SEAM == 1 << 22   # expected_label's segment
    # the order of the launches inside one segment
    seg_loop = mixed.index("for (uint64_t s0 = b0; s0 < b0 + nb; s0 += seg) {")
    classes = mixed.index("for (int mt = 1; mt <= kMaxMT; mt++) { if (list[mt].empty()) continue;")
    launch = mixed.index("HIP_TRY(hipLaunchKernel(fn,")
    label = mixed.index('"rs_mixed_kernel<K=%d,MT=%d>%s", K, mt, aligned ? "" : ",UA"')
    runs = mixed.index("for (uint64_t b = 0; b < sn;) {")
    fallback = mixed.index("int rc = launch_plan(c, *plans[p], rb, rs, bs, rb, rs, bs, S, e - b, stream);")
    assert seg_loop < classes < launch < label < runs < fallback
    assert mixed.count("hipLaunchKernel(") == 1 and mixed.count("launch_plan(") == 1
    with open(os.path.join(CSRC, "rs_plan.hpp")) as f:
        assert "constexpr int kMaxMT = 4;" in f.read()


def walk_launches(reps, cus=WALK_CUS):
    """Leg 4's class launches under waves_per_cu = 1 on a device of cus CUs, as launch_mixed sizes
    them: per class (tiles, waves of the capped grid, the pattern of every list entry)."""
    k, m = WALK_SHAPE
    rows = np.concatenate([sheet_case(k, m, WALK_S)["rows"]] * reps)
    tpb = ((WALK_S + 15) // 16 + 63) // 64
    wg_cap = max(1, cus * 1 // 4)
    out = {}
    for mt in (1, 2, 3, 4):
        entries = np.flatnonzero(rows == mt)
        if entries.size:
            ntiles = entries.size * tpb
            out[mt] = (ntiles, 4 * min((ntiles + 3) // 4, wg_cap), entries % NB, tpb)
    return out


def test_strided_walk_is_reached():
    """Leg 4 is there for the walk: with the sheet repeated 200 times every class launch has
    several times more tiles than the capped grid has waves on a 256-CU device, and in class 1 a
    wave's next tile (t += nw; tile t belongs to list entry t / tpb) is of a block with another
    pattern than the one it staged.  The 40-fold repeat fits the cap and walks nowhere: it stays
    as the uncapped form of the same call."""
    with open(MIXED_CPP) as f:
        mixed = _body(f.read(), "launch_mixed")
    with open(os.path.join(CSRC, "rs_mixed_kernels.hip")) as f:
        kernel = " ".join(f.read().split())
    assert "constexpr int wpg = kFastWG / kWave;" in mixed
    assert ("if (c->opt_waves_per_cu > 0) wg_cap = std::max(1L, long(c->num_cu) * c->opt_waves_per_cu / wpg);"
            in mixed)
    assert "uint32_t ntiles = uint32_t(list[mt].size() * tpb);" in mixed
    assert ("const uint64_t wgs = std::min<uint64_t>((uint64_t(ntiles) + wpg - 1) / wpg, uint64_t(wg_cap));"
            in mixed)
    assert "for (TileWalk tw(t, nw, tpb); t < ntiles; t += nw, tw.next(tpb)) {" in kernel
    assert "const uint32_t blk = lst[tw.blk].blk, pat = lst[tw.blk].pat; if (pat != staged) {" in kernel
    small, big = walk_launches(40), walk_launches(200)
    assert sorted(big) == [1, 2, 3] and [big[mt][0] for mt in (1, 2, 3)] == [1200, 600, 600]
    for mt, (ntiles, nw, pats, tpb) in big.items():
        assert nw == 256 and ntiles >= 2 * nw + 64, (mt, ntiles, nw)
    for mt, (ntiles, nw, pats, tpb) in small.items():
        assert ntiles <= nw, (mt, ntiles, nw)
    ntiles, nw, pats, tpb = big[1]
    assert set(pats.tolist()) == {1, 5}
    restaging = 0
    for w in range(nw):
        seq = [int(pats[t // tpb]) for t in range(w, ntiles, nw)]
        assert len(seq) >= 4
        restaging += any(a != b for a, b in zip(seq, seq[1:]))
    assert restaging == nw, restaging


def _write(buf, side, b, r, row, where=None, clip=False):
    o = row_at(side, b, r) if where is None else where
    n = row.size if not clip else max(0, min(row.size, buf.size - o))
    assert o + n <= buf.size
    buf[o:o + n] = row[:n]


def test_checker_rejects_simulated_slips():
    """The comparison can fail: "got" buffers built on the CPU from the slips this module is there
    for are each rejected, and the right image passes.  Nothing is built or run."""
    k, m, S = 10, 4, 1000
    n = k + m
    c = sheet_case(k, m, S)
    sh, image, W, present, rows = c["sh"], c["image"], c["W"], c["present"], c["rows"]
    ok = [b for b in range(NB) if rows[b]]
    side = geometries(k, m, S)["A0"]
    host, want = render(side, n, S, NB, sh), render(side, n, S, NB, image)
    label = expected_label(k, rows, "aligned")
    assert label == mixed_label(10, 3, True) and not np.array_equal(host, want)

    def rejected(got, tag, status=None, lab=label, want_buf=want):
        with pytest.raises(AssertionError):
            compare(c["status"] if status is None else status, got, lab, c["status"], want_buf, label, tag)

    compare(c["status"], want.copy(), label, c["status"], want, label, "good")
    rejected(want.copy(), "status", status=[0] * NB)
    rejected(want.copy(), "label", lab=mixed_label(10, 3, False))
    rejected(host.copy(), "nothing written")
    # a rebuilt row written at pitch S instead of rs (out_off taken from S)
    got = host.copy()
    for b in ok:
        for r in np.flatnonzero(W[b]):
            _write(got, side, b, r, image[b, r], where=GUARD + side.off + b * side.bs + r * S)
    rejected(got, "pitch S")
    # the rows read at pitch S: what the plan then computes is not the definition's row
    got = host.copy()
    shifted = np.array(sh)
    flat = host[GUARD + side.off:]
    for b in ok:
        for r in range(n):
            shifted[b, r] = flat[b * side.bs + r * S:][:S]
        rc, rec = orc.reconstruct(k, m, shifted[b], present[b].tolist(), False)
        for r in np.flatnonzero(W[b]):
            _write(got, side, b, r, rec[r])
    rejected(got, "rows read at pitch S")
    # a row written to blk = list index instead of the entry's block
    got = host.copy()
    for mt in (1, 2, 3, 4):
        for j, b in enumerate(np.flatnonzero(rows == mt)):
            assert j != b
            for r in np.flatnonzero(W[b]):
                _write(got, side, j, r, image[b, r])
    rejected(got, "list index")
    # block 5 rebuilt with block 1's plan: block 1's row is written, from block 1's survivors
    got = want.copy()
    rc, rec = orc.reconstruct(k, m, sh[5], present[1].tolist(), False)
    assert rc == 0
    for r in range(n):
        _write(got, side, 5, r, rec[r] if not present[1][r] else sh[5, r])
    rejected(got, "block 5 with block 1's plan")
    # one byte written past S in a rebuilt row
    got = want.copy()
    r = int(np.flatnonzero(W[1])[0])
    got[row_at(side, 1, r) + S] ^= 0xFF
    rejected(got, "offset S")
    # a too-few block written to
    got = want.copy()
    assert c["status"][4] == TOO_FEW
    got[row_at(side, 4, 0) + S - 1] ^= 1
    rejected(got, "too few")
    # a guard byte
    for o in (0, GUARD + side.off - 1, want.size - 1):
        got = want.copy()
        got[o] ^= 1
        rejected(got, ("guard", o))
    # bs and rs swapped on the transposed geometry
    for gid in ("transposed", "transposed-ua"):
        t = geometries(k, m, S)[gid]
        thost, twant = render(t, n, S, NB, sh), render(t, n, S, NB, image)
        compare(c["status"], twant.copy(), label, c["status"], twant, label, gid)
        got = thost.copy()
        swapped = t._replace(rs=t.bs, bs=t.rs)
        for b in ok:
            for r in np.flatnonzero(W[b]):
                _write(got, swapped, b, r, image[b, r], clip=True)
        rejected(got, (gid, "swapped"), want_buf=twant)


# ---------------------------------------------------------------- GPU plumbing
@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    rsmi = pytest.importorskip("rsmi")
    if not torch.cuda.is_available() or rsmi.device_count() == 0:
        pytest.skip("no GPU")
    assert rsmi.ErrTooFewShards == TOO_FEW
    yield torch, rsmi
    _CASES.clear()


def run_mixed(torch, c, side, k, m, S, nb, sh, present, required, data_only, want_status, image, rows, form, ctx):
    """One rsmi_reconstruct_mixed_batch_dev over sh laid out by side: statuses, label and the
    whole buffer against the definition.  Returns what the buffer held afterwards."""
    n = k + m
    host = render(side, n, S, nb, sh)
    want = render(side, n, S, nb, image)
    d = torch.from_numpy(host).cuda()
    assert d.data_ptr() % 16 == 0
    ptr = d.data_ptr() + GUARD + side.off
    got_form = expected_form(ptr, side.rs, side.bs, S)
    assert got_form == form, (ctx, got_form, form)
    got = c.reconstruct_mixed_batch_dev(ptr, side.rs, side.bs, S, nb, u8(present),
                                        None if required is None else u8(required), data_only,
                                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d.cpu().numpy()
    compare(got, out, c.last_kernel(), want_status, want, expected_label(k, rows, form), ctx)
    return out


def run_sheet(torch, c, k, m, gid, S, side, form, required=False, data_only=False):
    s = sheet_case(k, m, S, required, data_only)
    return run_mixed(torch, c, side, k, m, S, NB, s["sh"], s["present"], s["required"], data_only, s["status"],
                     s["image"], s["rows"], form, (k, m, gid, S, required, data_only))


# ---------------------------------------------------------------- leg 1: every geometry, size and shape
@pytest.mark.gpu
@pytest.mark.parametrize("k,m", SHAPES)
def test_mixed_layouts(gpu, k, m):
    """Every geometry at its sizes: 6 blocks, classes 1..3 beside an intact and a too-few block
    ((5,5): a two-tile plan beside the classes; (7,2), (20,4) and S = 15: every block through
    launch_plan on the pitched geometry)."""
    torch, rsmi = gpu
    labels = set()
    with rsmi.Codec(k, m) as c:
        for gid, S, side, form in cases(k, m):
            run_sheet(torch, c, k, m, gid, S, side, form)
            labels.add(c.last_kernel())
    if k in KS and (k, m) != (5, 5):
        top = min(m, 3)
        assert {mixed_label(k, top, True), mixed_label(k, top, False), generic_label(k, 1)} == labels, labels
    elif k in KS:
        assert {fast_label(5, 1), fast_label(5, 1, ua=True), generic_label(5, 1)} == labels, labels
    else:
        assert {generic_label(k, 1)} == labels, labels


# ---------------------------------------------------------------- leg 2: required masks and data_only
@pytest.mark.gpu
@pytest.mark.parametrize("k,m", REQUIRED_SHAPES)
def test_mixed_layouts_required_and_data_only(gpu, k, m):
    torch, rsmi = gpu
    with rsmi.Codec(k, m) as c:
        for gid, S, side, form in cases(k, m):
            if gid not in ("A0", "T-rs8", "phases", "transposed-ua"):
                continue
            for required, data_only in ((True, False), (False, True), (True, True)):
                run_sheet(torch, c, k, m, gid, S, side, form, required, data_only)


# ---------------------------------------------------------------- leg 3: the uniform call
@pytest.mark.gpu
@pytest.mark.parametrize("gid", ["T-rs8", "phases", "transposed"])
def test_mixed_layouts_equal_the_uniform_call(gpu, gid):
    """One pattern for all 6 blocks: rsmi_reconstruct_rows_batch_dev and the mixed call on two
    copies give identical buffers, which differ from the input (and equal the definition's)."""
    torch, rsmi = gpu
    k, m, S, lost = 10, 4, 2049, (0, 5, 11)
    n = k + m
    side = geometries(k, m, S)[gid]
    present = present_of(n, [lost] * NB)
    sh = stored(stripes(k, m, S, NB), present)
    W = wanted(k, present, None, False)
    status, image = definition(k, m, sh, present, W)
    host = render(side, n, S, NB, sh)
    stream = torch.cuda.current_stream().cuda_stream
    with rsmi.Codec(k, m) as c:
        d1 = torch.from_numpy(host.copy()).cuda()
        assert d1.data_ptr() % 16 == 0
        c.reconstruct_rows_batch_dev(d1.data_ptr() + GUARD + side.off, side.rs, side.bs, S, NB, present[0].tolist(),
                                     W[0].tolist(), stream)
        torch.cuda.synchronize()
        form = "aligned" if gid == "transposed" else "ua"
        assert c.last_kernel() == fast_label(k, 3, ua=form == "ua")
        out = run_mixed(torch, c, side, k, m, S, NB, sh, present, None, False, status, image,
                        rows_rebuilt(k, present, W), form, (gid, "uniform"))
        same_bytes(out, d1.cpu().numpy(), (gid, "mixed against uniform"))
        assert not np.array_equal(out, host)


# ---------------------------------------------------------------- leg 4: the strided walk
@pytest.mark.gpu
@pytest.mark.parametrize("reps", WALK_REPS)
@pytest.mark.parametrize("gid", WALK_IDS)
def test_mixed_layouts_waves_per_cu_1(gpu, gid, reps):
    """waves_per_cu = 1 at a pitch that is not S, the sheet repeated: 240 blocks of 3 tiles, whose
    launches fit under the cap, and 1200 blocks, 1200 / 600 / 600 tiles per class against the 256
    waves the cap leaves a 256-CU device: a wave goes on to tiles of other blocks and, in class 1,
    of another pattern, and restages its tables and row offsets
    (test_strided_walk_is_reached)."""
    torch, rsmi = gpu
    (k, m), S = WALK_SHAPE, WALK_S
    s = sheet_case(k, m, S)
    nb = NB * reps
    side = geometries(k, m, S, nb)[gid]
    if reps == 200:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        for mt, (ntiles, nw, pats, tpb) in walk_launches(reps, cus).items():
            assert ntiles > nw, ("the walk is not reached on this device", cus, mt, ntiles, nw)

    def tiled(a):
        return np.concatenate([a] * reps)

    with rsmi.Codec(k, m) as c:
        c.set_option("waves_per_cu", 1)
        run_mixed(torch, c, side, k, m, S, nb, tiled(s["sh"]), tiled(s["present"]), None, False, s["status"] * reps,
                  tiled(s["image"]), tiled(s["rows"]), "ua", (gid, "waves_per_cu"))
