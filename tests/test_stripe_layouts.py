"""rsmi_locate and rsmi_heal with independent data and parity layouts, bit for bit.

rsmi_locate_batch_dev and rsmi_heal_batch_dev take the two halves rsmi_verify_batch_dev takes: row
c of data block b at d_data + b*data_block_stride + c*data_shard_stride, parity row j at d_parity +
b*parity_block_stride + j*parity_shard_stride.  The other locate and heal modules call them with
one buffer, one shard stride and one block stride for both halves, where a culprit row stored at
the other half's pitch or block stride, into the other allocation, or one stride pair used for both
halves of rs_heal_rows_kernel all give the right address.  Here the geometry model of
test_layout_contract.py (15 geometries at 3-4 sizes over 8 shapes, 4 blocks) carries a sheet of
damage through both calls; heal is the one that writes, so after it every allocation is compared
whole.

The sheet of a case (its index i rotates the culprit rows) is, from the oracle's clean stripes:
  block 0  data row i % k, bytes min(16, S - 1) and S - 1 flipped
  block 1  parity row k + i % m, bytes 0 and S - 1 flipped
  block 2  data row (i + 1) % k and parity row k + m - 1, both flipped at byte S // 2
  block 3  clean
and where a culprit row's pitch leaves a byte at offset S, that padding byte is flipped in the
buffer too: it changes no verdict and comes back flipped.  The verdicts are test_locate.want_verdict's
(replace shard x by its reconstruction, re-encode, compare), the flags test_verify.want_flags',
the image test_heal.want_image's: none comes from the library, and there are no tolerances.  The
launch label is part of every assertion; stripe_labels() below restates launch_verify,
launch_locate and launch_heal.

  0  the sheet's verdicts and images, the label rule's families, the comparison rejects the slips (CPU)
  1  rsmi_locate_batch_dev over every case
  2  rsmi_heal_batch_dev over every case, then rsmi_verify_batch_dev on the healed device buffers
  2b every geometry once more with the damage two blocks on: the data culprit behind a block stride
  3  rsmi_locate_batch_host and rsmi_heal_batch_host: mixed memory on every path, and the upload
     pipeline past a chunk boundary with different block strides
"""
import collections
import itertools
import os
import time

import numpy as np
import pytest

import oracle_lib as orc
from test_heal import want_image
from test_layout_contract import (FILL_DATA, FILL_PARITY, GUARD, SHAPES, HostBuf, Side, blank, cases, check, download,
                                  dptr, expected_form, form_on_device, geometries, put, ref_of, round_up, row_at,
                                  small_path, upload)
from test_locate import CLEAN, UNKNOWN, want_verdict, want_verdicts
from test_locate_matrix import LOCATE_KS, LOCATE_MTS
from test_verify import want_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "filedag-storage_amd", "csrc")
NB4 = 4
POISON = 0x5EED
COMPARE, LOCATE_ROWS, HEAL_ROWS = "rs_compare_rows_kernel", "rs_locate_rows_kernel", "rs_heal_rows_kernel"
FAMILIES = ["verify", "verify,UA", "compare_rows", "fused", "fused,UA", "rows"]


# ---------------------------------------------------------------- the label rule, restated
def stripe_labels(k, m, form):
    """(verify, locate, heal): the label each call leaves on a layout of expected_form() form.
    launch_verify: rs_verify_kernel over the plan's tiles of at most 4 parity rows (the label is
    the last tile's) when the layout is aligned or UA and K has a kernel, else the encode into
    scratch and rs_compare_rows_kernel.  launch_locate: m = 1 is Verify's launch and nothing else;
    a one-tile plan (m <= 4) of a K with an rs_locate_kernel on an aligned or UA layout runs it;
    everything else the rows kernel.  launch_heal: locate's launches, then rs_heal_kernel where
    rs_locate_kernel ran, rs_heal_rows_kernel where the rows kernel did, nothing for m = 1."""
    if form == "generic" or k not in LOCATE_KS:
        verify = COMPARE
    else:
        verify = "rs_verify_kernel<K=%d,MT=%d>%s" % (k, m - 4 * ((m - 1) // 4), ",UA" if form == "ua" else "")
    if m == 1:
        return verify, verify, verify
    if form != "generic" and k in LOCATE_KS and m in LOCATE_MTS:
        shape = "<K=%d,MT=%d>%s" % (k, m, ",UA" if form == "ua" else "")
        return verify, "rs_locate_kernel" + shape, "rs_heal_kernel" + shape
    return verify, LOCATE_ROWS, HEAL_ROWS


def family(label):
    if label.startswith("rs_verify_kernel"):
        return "verify,UA" if label.endswith(",UA") else "verify"
    if label == COMPARE:
        return "compare_rows"
    if label in (LOCATE_ROWS, HEAL_ROWS):
        return "rows"
    assert label.startswith(("rs_locate_kernel<", "rs_heal_kernel<")), label
    return "fused,UA" if label.endswith(",UA") else "fused"


# ---------------------------------------------------------------- the sheet
Sheet = collections.namedtuple("Sheet", "sh verdicts flags image image_flags culprits")
_SHEETS = {}


def sheet(k, m, S, i, rot=0):
    """The damaged stripes of case index i and the definition's answers for them, computed once
    per (k, m, S, i % k, i % m): the rows alone decide, never the geometry.  Read-only.  rot moves
    the damage of block b to block (b + rot) % 4 (leg 2b: with the sheet as it stands the one data
    culprit sits in block 0, where no block stride enters its address)."""
    key = (k, m, S, i % k, i % m, rot)
    if key not in _SHEETS:
        ref = ref_of(k, m, S, NB4)
        sh = np.concatenate([ref.data, ref.parity], axis=1)
        x0, x1, x2 = i % k, k + i % m, (i + 1) % k
        b0, b1, b2 = [(b + rot) % NB4 for b in range(3)]
        sh[b0, x0, min(16, S - 1)] ^= 0x40   # S <= 17: the same byte as the next line's, two masks
        sh[b0, x0, S - 1] ^= 0x01
        sh[b1, x1, 0] ^= 0x80
        sh[b1, x1, S - 1] ^= 0x02
        sh[b2, x2, S // 2] ^= 0x21
        sh[b2, k + m - 1, S // 2] ^= 0x9C
        verdicts = want_verdicts(k, m, sh)
        image = want_image(k, m, sh, verdicts)
        for a in (sh, verdicts, image):
            a.setflags(write=False)
        _SHEETS[key] = Sheet(sh, verdicts, want_flags(k, m, sh), image, want_flags(k, m, image),
                             ((b0, x0), (b1, x1), (b2, x2), (b2, k + m - 1)))
    return _SHEETS[key]


def side_row(k, d, p, x):
    """The side and the row within it of shard x."""
    return (d, x) if x < k else (p, x - k)


def before_of(k, m, S, sht, d, p):
    """(buffers, padding spots): the sheet laid out by the two sides, and the byte at offset S of
    every culprit row whose pitch leaves one flipped."""
    bufs = blank(d, p, NB4)
    put(bufs, d, sht.sh[:, :k])
    put(bufs, p, sht.sh[:, k:])
    pads = []
    for b, x in sht.culprits:
        side, r = side_row(k, d, p, x)
        if side.rs > S:
            o = row_at(side, b, r) + S
            assert bufs[side.alloc][o] in (FILL_DATA, FILL_PARITY)
            bufs[side.alloc][o] ^= 0xFF
            pads.append((side.alloc, o))
    return bufs, pads


def healed_of(k, sht, d, p, before):
    """before with the rows of the definition's image put back at their sides."""
    want = {a: x.copy() for a, x in before.items()}
    put(want, d, sht.image[:, :k])
    put(want, p, sht.image[:, k:])
    return want


# ---------------------------------------------------------------- leg 0 (CPU)
@pytest.mark.parametrize("k,m", SHAPES)
def test_sheet_is_what_the_definition_says(k, m):
    """For every case of the shape: one damaged shard names it and heals to the undamaged stripe
    (m >= 2), two damaged shards are UNKNOWN by the distance for m >= 3 and the definition's for
    m = 2, m = 1 names nothing; an UNKNOWN block is left as it is and alone keeps its flags."""
    n_cases = 0
    stored = set()
    for i, (gid, S, d, p, form) in enumerate(cases(k, m, NB4)):
        ctx = (k, m, gid, S, i)
        sht = sheet(k, m, S, i)
        ref = ref_of(k, m, S, NB4)
        full = np.concatenate([ref.data, ref.parity], axis=1)
        v = sht.verdicts.tolist()
        if m == 1:
            assert v == [UNKNOWN, UNKNOWN, UNKNOWN, CLEAN], ctx
            assert np.array_equal(sht.image, sht.sh), ctx
        else:
            assert v[:2] + v[3:] == [i % k, k + i % m, CLEAN], ctx
            assert v[2] == want_verdict(k, m, sht.sh[2]) and (m < 3 or v[2] == UNKNOWN), ctx
            assert np.array_equal(sht.image[:2], full[:2]) and np.array_equal(sht.image[3], full[3]), ctx
            stored.update(x for x in v if x >= 0)
        # flags: a data row raises all m, a parity row its own
        assert sht.flags[0].all() and sht.flags[1].tolist() == [j == i % m for j in range(m)], ctx
        assert sht.flags[2].any() and not sht.flags[3].any(), ctx
        for b in range(NB4):
            if v[b] < 0:
                assert np.array_equal(sht.image[b], sht.sh[b]), ctx
            assert sht.image_flags[b].any() == (v[b] == UNKNOWN), ctx
        # the buffers: the padding bytes are flipped where there is one and are no row's byte
        before, pads = before_of(k, m, S, sht, d, p)
        want = healed_of(k, sht, d, p, before)
        for a, o in pads:
            assert before[a][o] == want[a][o] and before[a][o] in (FILL_DATA ^ 0xFF, FILL_PARITY ^ 0xFF), ctx
        assert len(pads) == sum(side_row(k, d, p, x)[0].rs > S for _, x in sht.culprits), ctx
        n_cases += 1
    assert n_cases == 48
    if m >= 2:  # the case index rotates the culprits over every row of either side
        assert stored >= set(range(k + m)), (k, m, sorted(set(range(k + m)) - stored))


def test_label_rule_reaches_every_family():
    """Over SHAPES x cases the rule gives each of the six families to locate and to heal."""
    count = {"locate": collections.Counter(), "heal": collections.Counter()}
    for k, m in SHAPES:
        for gid, S, d, p, form in cases(k, m, NB4):
            assert form == expected_form(GUARD + d.off, d.rs, d.bs, GUARD + p.off, p.rs, p.bs, S)
            v, lo, he = stripe_labels(k, m, form)
            count["locate"][family(lo)] += 1
            count["heal"][family(he)] += 1
            assert (m == 1) == (lo == v == he)
            assert family(lo) == family(he) and lo.endswith(",UA") == he.endswith(",UA")
            assert lo.endswith(",UA") == (form == "ua" and family(lo) != "rows")
    for call in ("locate", "heal"):
        for fam in FAMILIES:
            assert count[call][fam] > 0, (call, fam, dict(count[call]))
    assert stripe_labels(10, 4, "aligned") == ("rs_verify_kernel<K=10,MT=4>", "rs_locate_kernel<K=10,MT=4>",
                                               "rs_heal_kernel<K=10,MT=4>")
    assert stripe_labels(5, 5, "ua") == ("rs_verify_kernel<K=5,MT=1>,UA", LOCATE_ROWS, HEAL_ROWS)
    assert stripe_labels(2, 1, "generic") == (COMPARE,) * 3


def test_label_rule_matches_source():
    """The branches stripe_labels() restates are the ones launch_verify, launch_locate and
    launch_heal have: an edit to them fails here instead of silently retargeting the cases."""
    src = {}
    for name in ("rsmi_verify.cpp", "rsmi_locate.cpp", "rsmi_heal.cpp"):
        with open(os.path.join(CSRC, name)) as f:
            src[name] = " ".join(f.read().split())
    ver, loc, heal = src["rsmi_verify.cpp"], src["rsmi_locate.cpp"], src["rsmi_heal.cpp"]
    # the table lookup and the label every tile launch shares
    assert ("void* stripe_kernel(const StripeKernelTable& table, StripeLayout layout, const DevTile& t) { "
            "if (layout == StripeLayout::kNeither || t.K > 16) return nullptr; "
            "return (layout == StripeLayout::kAligned ? table.fn : table.ua)[t.K][t.MT]; }") in ver
    assert ('"rs_%s_kernel<K=%d,MT=%d>%s", name, t.K, t.MT, layout == StripeLayout::kUA ? ",UA" : ""); '
            "set_last_kernel(c, buf);") in ver
    assert "if (!stripe_kernel(verify_kernels(), layout, t)) fast = false;" in ver
    assert ("void* lfn = loc && plan.tiles.size() == 1 ? stripe_kernel(locate_kernels(), layout, plan.tiles[0]) : "
            "nullptr;") in ver
    assert 'return tiles_launched(c, lfn ? "locate" : "verify", layout, plan.tiles.back());' in ver
    assert 'set_last_kernel(c, "rs_compare_rows_kernel");' in ver
    assert "if (m == 1) {" in loc and "if (plan.tiles.size() == 1) {" in loc
    assert 'if (loc.fused == StripeLayout::kNeither) {' in loc and 'set_last_kernel(c, "rs_locate_rows_kernel");' in loc
    assert "if (c->m == 1) return RSMI_OK;" in heal and "if (fused != StripeLayout::kNeither) {" in heal
    assert "void* fn = stripe_kernel(heal_kernels(), fused, t);" in heal
    assert 'return tiles_launched(c, "heal", fused, t);' in heal
    assert ('return launch_heal_rows(c, plan, heal_rows_kernel(), "rs_heal_rows_kernel", rows, culprit, 1, stream);'
            in heal)
    assert "set_last_kernel(c, label);" in heal


def _at(side, b, r):
    """The side whose row (0, 0) is side's row (b, r): put() of one row."""
    return side._replace(off=side.off + b * side.bs + r * side.rs)


def test_checker_rejects_simulated_slips():
    """RS(10,4), S = 1000, five geometries: "got" buffers built on the CPU with a healed row where
    a slip would have stored it (and the damage left where it was) are each rejected by check(),
    wherever the slip's address really differs from the right one; the right image passes."""
    k, m, S, i = 10, 4, 1000, 3
    R = round_up(S, 16)
    tried = skipped = 0
    # the sheet as it stands, and with the damage moved on by two blocks: the data culprit of the
    # first sits in block 0, where a wrong block stride gives the right address
    for rot, gid in itertools.product((0, 2), ("A0", "A0m", "split-in", "phases", "interleaved")):
        sht = sheet(k, m, S, i, rot)
        assert np.roll(sht.verdicts, -rot).tolist() == [3, k + 3, UNKNOWN, CLEAN]
        d, p = geometries(k, m, S, NB4)[gid]
        before, _ = before_of(k, m, S, sht, d, p)
        want = healed_of(k, sht, d, p, before)
        check(healed_of(k, sht, d, p, before), want, (gid, "good"))
        with pytest.raises(AssertionError):
            check(before, want, (gid, "nothing healed"))
        healed = [(rot, 3, d, 3), (rot + 1, k + 3, p, 3)]   # (block, shard, side, row within the side)
        # slip -> the side each healed row is stored through
        slips = collections.OrderedDict([
            ("data row at parity_rs", {3: d._replace(rs=p.rs)}),
            ("data row at parity_bs", {3: d._replace(bs=p.bs)}),
            ("parity row at data_rs", {k + 3: p._replace(rs=d.rs)}),
            ("parity row at data_bs", {k + 3: p._replace(bs=d.bs)}),
            ("into the other allocation", {3: d._replace(alloc=p.alloc), k + 3: p._replace(alloc=d.alloc)}),
        ])
        for name, wrong in slips.items():
            tried += 1
            differs = any((wrong[x].alloc, row_at(wrong[x], b, r)) != (side.alloc, row_at(side, b, r))
                          for b, x, side, r in healed if x in wrong)
            if not differs:
                skipped += 1
                assert (rot == 0 and name == "data row at parity_bs") or gid == "interleaved", (rot, gid, name)
                continue
            got = {a: v.copy() for a, v in before.items()}
            for b, x, side, r in healed:
                put(got, _at(wrong.get(x, side), b, r), sht.image[b, x][None, None], clip=True)
            with pytest.raises(AssertionError):
                check(got, want, (rot, gid, name))
        # the row's last chunk stored as 16 whole bytes: bytes S .. round_up(S, 16) change
        tried += 1
        got = {a: v.copy() for a, v in want.items()}
        for b, x, side, r in healed:
            o = row_at(side, b, r)
            got[side.alloc][o + S:o + R] = 0
        with pytest.raises(AssertionError):
            check(got, want, (rot, gid, "whole last chunk"))
    assert tried == 60 and skipped * 4 < tried, (tried, skipped)


# ---------------------------------------------------------------- GPU plumbing
SEEN = collections.Counter()
LEGS = set()
WALL = collections.OrderedDict()


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    rsmi = pytest.importorskip("rsmi")
    if not torch.cuda.is_available() or rsmi.device_count() == 0:
        pytest.skip("no GPU")
    assert (rsmi.LocateClean, rsmi.LocateUnknown) == (CLEAN, UNKNOWN)
    yield torch, rsmi
    for call in ("locate", "heal"):
        print("\nstripe layouts: %s calls run and asserted by label, per family:" % call,
              ", ".join("%s %d" % (f, SEEN[call, f]) for f in FAMILIES), end="")
    print("\nstripe layouts: wall seconds per leg:", ", ".join("%s %.2f" % kv for kv in WALL.items()))
    if LEGS == {(call, km) for call in ("locate", "heal") for km in SHAPES}:  # both device legs ran whole
        for call in ("locate", "heal"):
            for f in FAMILIES:
                assert SEEN[call, f] > 0, (call, f)


class _leg:
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.t0 = time.perf_counter()

    def __exit__(self, *a):
        WALL[self.name] = WALL.get(self.name, 0.0) + time.perf_counter() - self.t0


def _outputs(torch, m, nb=NB4):
    return (torch.full((nb + 2,), POISON, dtype=torch.int32, device="cuda"),
            torch.full((nb * m + 2,), POISON, dtype=torch.int32, device="cuda"))


def _results(cul, bad, m, flags, ctx, nb=NB4):
    """The verdicts and the flags as bool (None when no pointer was given); the entries past the
    outputs' end, and the flags nobody asked for, are still poisoned."""
    cul, bad = np.asarray(cul), np.asarray(bad)
    assert (cul[nb:] == POISON).all() and (bad[nb * m:] == POISON).all(), ctx + ("wrote past its outputs",)
    if not flags:
        assert (bad == POISON).all(), ctx
        return cul[:nb], None
    return cul[:nb], bad[:nb * m].reshape(nb, m) != 0


# ---------------------------------------------------------------- leg 1: rsmi_locate_batch_dev
@pytest.mark.gpu
@pytest.mark.parametrize("k,m", SHAPES)
def test_locate_independent_layouts(gpu, k, m):
    """Every geometry at its sizes through rsmi_locate_batch_dev, with the flags pointer on even
    case indices and without on odd ones: the label of the rule, the definition's verdicts and
    flags, the outputs' tails poisoned, every allocation byte for byte as uploaded."""
    torch, rsmi = gpu
    h = torch.cuda.current_stream().cuda_stream
    with _leg("locate"), rsmi.Codec(k, m) as c:
        for i, (gid, S, d, p, form) in enumerate(cases(k, m, NB4)):
            ctx = (k, m, gid, S, i)
            sht = sheet(k, m, S, i)
            host, _ = before_of(k, m, S, sht, d, p)
            dev = upload(torch, host)
            form_on_device(dev, d, p, S, form)
            label = stripe_labels(k, m, form)[1]
            flags = i % 2 == 0
            cul, bad = _outputs(torch, m)
            c.locate_batch_dev(dptr(dev, d), d.rs, d.bs, dptr(dev, p), p.rs, p.bs, S, NB4, cul.data_ptr(),
                               bad.data_ptr() if flags else 0, h)
            torch.cuda.synchronize()
            assert c.last_kernel() == label, (c.last_kernel(), label) + ctx
            got, gbad = _results(cul.cpu().numpy(), bad.cpu().numpy(), m, flags, ctx)
            assert np.array_equal(got, sht.verdicts), ctx + (got.tolist(), sht.verdicts.tolist())
            if flags:
                assert np.array_equal(gbad, sht.flags), ctx + (gbad.tolist(),)
            check(download(dev), host, ctx + ("locate wrote to the shards",))
            SEEN["locate", family(label)] += 1
    LEGS.add(("locate", (k, m)))


# ---------------------------------------------------------------- leg 2: rsmi_heal_batch_dev
def _heal_case(torch, c, k, m, gid, S, i, d, p, form, rot=0):
    """One rsmi_heal_batch_dev and, behind it on the stream, one rsmi_verify_batch_dev over the
    sheet of case i laid out by (d, p); returns heal's label."""
    ctx = (k, m, gid, S, i, rot)
    h = torch.cuda.current_stream().cuda_stream
    sht = sheet(k, m, S, i, rot)
    host, pads = before_of(k, m, S, sht, d, p)
    want = healed_of(k, sht, d, p, host)
    dev = upload(torch, host)
    form_on_device(dev, d, p, S, form)
    vlabel, _, label = stripe_labels(k, m, form)
    flags = i % 2 == 1
    cul, bad = _outputs(torch, m)
    vbad = torch.full((NB4 * m,), POISON, dtype=torch.int32, device="cuda")
    c.heal_batch_dev(dptr(dev, d), d.rs, d.bs, dptr(dev, p), p.rs, p.bs, S, NB4, cul.data_ptr(),
                     bad.data_ptr() if flags else 0, h)
    healed_by = c.last_kernel()
    c.verify_batch_dev(dptr(dev, d), d.rs, d.bs, dptr(dev, p), p.rs, p.bs, S, NB4, vbad.data_ptr(), h)
    torch.cuda.synchronize()
    assert healed_by == label, (healed_by, label) + ctx
    assert c.last_kernel() == vlabel, (c.last_kernel(), vlabel) + ctx
    got, gbad = _results(cul.cpu().numpy(), bad.cpu().numpy(), m, flags, ctx)
    assert np.array_equal(got, sht.verdicts), ctx + (got.tolist(), sht.verdicts.tolist())
    if flags:
        assert np.array_equal(gbad, sht.flags), ctx + (gbad.tolist(),)
    after = download(dev)
    check(after, want, ctx)
    for a, o in pads:
        assert after[a][o] in (FILL_DATA ^ 0xFF, FILL_PARITY ^ 0xFF), ctx
    gv = vbad.cpu().numpy().reshape(NB4, m) != 0
    assert np.array_equal(gv, sht.image_flags), ctx + (gv.tolist(),)
    return label


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", SHAPES)
def test_heal_independent_layouts(gpu, k, m):
    """The same cases through rsmi_heal_batch_dev (the flags pointer on odd case indices), then,
    with no host copy in between, rsmi_verify_batch_dev on the same device buffers: the labels of
    the rule, the definition's verdicts and flags, Verify's flags exactly those of the image (set
    for an UNKNOWN block, which is left alone, and for nothing else), and every allocation, whole,
    "before" with the image's rows put back at their sides: guards, gaps, padding and the flipped
    padding bytes unchanged.  Over the shape's 48 cases every data row and every parity row is the
    stored one at least once (leg 0 asserts the rotation)."""
    torch, rsmi = gpu
    with _leg("heal"), rsmi.Codec(k, m) as c:
        for i, (gid, S, d, p, form) in enumerate(cases(k, m, NB4)):
            SEEN["heal", family(_heal_case(torch, c, k, m, gid, S, i, d, p, form))] += 1
    LEGS.add(("heal", (k, m)))


def later_block_cases(k, m):
    """Leg 2b's cases: every geometry once, at the sizes in turn."""
    by_gid = collections.OrderedDict()
    for i, (gid, S, d, p, form) in enumerate(cases(k, m, NB4)):
        by_gid.setdefault(gid, []).append((i, gid, S, d, p, form))
    for j, at in enumerate(by_gid.values()):
        yield at[j % len(at)]


def test_later_block_cases_cover_every_geometry():
    for k, m in SHAPES:
        got = list(later_block_cases(k, m))
        assert sorted(g for _, g, _, _, _, _ in got) == sorted(geometries(k, m, 1000, NB4)), (k, m)
        assert len({S for _, _, S, _, _, _ in got}) >= 3, (k, m)
        if m >= 2:
            for i, gid, S, d, p, form in got:
                v = sheet(k, m, S, i, 2).verdicts.tolist()
                assert [v[2], v[3], v[1]] == [i % k, k + i % m, CLEAN] and (m < 3 or v[0] == UNKNOWN), (k, m, gid, S)


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", SHAPES)
def test_heal_culprits_in_later_blocks(gpu, k, m):
    """Leg 2b.  In the sheet as it stands the one data culprit is in block 0, whose rows' addresses
    no block stride enters, so a data row stored at b * parity_block_stride would pass leg 2.  Every
    geometry once more with the damage moved on by two blocks: the data culprit in block 2, the
    parity culprit in block 3, the two damaged shards in block 0.  Leg 2's assertions."""
    torch, rsmi = gpu
    with _leg("heal-later-blocks"), rsmi.Codec(k, m) as c:
        for i, gid, S, d, p, form in later_block_cases(k, m):
            _heal_case(torch, c, k, m, gid, S, i, d, p, form, rot=2)


# ---------------------------------------------------------------- leg 3: the host entry points
HOST_K, HOST_M, HOST_S = 10, 4, 2049
HOST_TOTAL = NB4 * (HOST_K + HOST_M) * HOST_S
SMALL = 2 << 20
# path -> (zero_copy, small_call_bytes)
HOST_PATHS = collections.OrderedDict([
    ("zero-copy", (1, 0)),      # both sides page-locked: in place; any other mix: the pipeline
    ("small-call", (0, SMALL)),  # one kernel over the caller's page-locked rows and the staged pageable ones
    ("pipeline", (0, 0)),       # chunks of pitched device rows, whatever the memory
])


def test_host_paths_follow_the_rule():
    """What the three option pairs select for the four memory mixes, by the rule of
    verify_host_impl (test_layout_contract.small_path restates it; its text in the source is pinned
    by test_verify_host.py::test_mixed_memory and test_layout_contract.py's leg 0)."""
    mixes = [(dp, pp) for dp in (True, False) for pp in (True, False)]
    one = {path: [small_path(zc, dp, pp, HOST_TOTAL, X) for dp, pp in mixes] for path, (zc, X) in HOST_PATHS.items()}
    assert one == {"zero-copy": [True, False, False, False], "small-call": [True] * 4, "pipeline": [False] * 4}
    assert 2 * HOST_TOTAL <= SMALL and HOST_S % 2 == 1


def _host_call(c, heal, db, pb, S, nb, flags=True):
    m = c.m
    cul = np.full(nb + 2, POISON, dtype=np.int32)
    bad = np.full(nb * m + 2, POISON, dtype=np.uint32)
    fn = c.heal_batch_host_ptr if heal else c.locate_batch_host_ptr
    fn(db.ptr, db.side.bs, pb.ptr, pb.side.bs, S, nb, cul.ctypes.data, bad.ctypes.data if flags else 0)
    return _results(cul, bad, m, flags, ("host", heal), nb)


@pytest.mark.gpu
@pytest.mark.parametrize("parity_pinned", [True, False], ids=["parity-locked", "parity-pageable"])
@pytest.mark.parametrize("data_pinned", [True, False], ids=["data-locked", "data-pageable"])
@pytest.mark.parametrize("path", list(HOST_PATHS))
def test_host_mixed_memory(gpu, path, data_pinned, parity_pinned):
    """rsmi_locate_batch_host and rsmi_heal_batch_host, RS(10,4), S = 2049, 4 blocks with gaps
    (dbs = k*S + 24, pbs = m*S + 40), 64 guard bytes around each side, either side page-locked or
    pageable, on the in-place path, the small staged call (which stages only the pageable side, so
    the one kernel runs with the caller's block stride on one side and the staging's on the other)
    and the upload pipeline (which copies a healed row home at the caller's own block stride).
    Both arrays whole, verdicts and flags against the definition.  The label ends ",UA" exactly
    where one kernel reads the caller's rows or the staging at pitch S: verify_host_impl's rule,
    whose text test_verify_host.py::test_mixed_memory pins."""
    torch, rsmi = gpu
    k, m, S = HOST_K, HOST_M, HOST_S
    zero_copy, X = HOST_PATHS[path]
    one_kernel = small_path(zero_copy, data_pinned, parity_pinned, HOST_TOTAL, X)
    db = HostBuf(rsmi, k, S, k * S + 24, FILL_DATA, data_pinned, NB4)
    pb = HostBuf(rsmi, m, S, m * S + 40, FILL_PARITY, parity_pinned, NB4)
    try:
        with _leg("host"), rsmi.Codec(k, m) as c:
            c.set_option("zero_copy", zero_copy)
            c.set_option("small_call_bytes", X)
            # the sheet as it stands and moved on by two blocks (leg 2b: the data culprit in block 2)
            for rot, heal in itertools.product((0, 2), (False, True)):
                ctx = (path, data_pinned, parity_pinned, rot, heal)
                sht = sheet(k, m, S, 7, rot)
                assert np.roll(sht.verdicts, -rot).tolist() == [7, k + 3, UNKNOWN, CLEAN]
                db.a[:] = FILL_DATA
                pb.a[:] = FILL_PARITY
                put({"h": db.a}, db.side, sht.sh[:, :k])
                put({"h": pb.a}, pb.side, sht.sh[:, k:])
                want = {"d": db.a.copy(), "p": pb.a.copy()}
                if heal:
                    put({"h": want["d"]}, db.side, sht.image[:, :k])
                    put({"h": want["p"]}, pb.side, sht.image[:, k:])
                got, gbad = _host_call(c, heal, db, pb, S, NB4)
                label = ("rs_heal_kernel" if heal else "rs_locate_kernel") + "<K=10,MT=4>" + (",UA" if one_kernel else "")
                assert label == stripe_labels(k, m, "ua" if one_kernel else "aligned")[2 if heal else 1]
                assert c.last_kernel() == label, (c.last_kernel(), label) + ctx
                assert np.array_equal(got, sht.verdicts), ctx + (got.tolist(),)
                assert np.array_equal(gbad, sht.flags), ctx
                check({"d": db.a, "p": pb.a}, want, ctx)
    finally:
        db.free()
        pb.free()


@pytest.mark.gpu
def test_host_pipeline_past_a_chunk_with_two_block_strides(gpu):
    """RS(3,2), S = 2049, pageable arrays with dbs = k*S + 24 != pbs = m*S + 40, small_call_bytes 0,
    3 * chunk + 3 blocks (test_heal.py::test_host_pipeline_pageable's sizing): the fourth chunk
    takes the first chunk's staging slot.  Culprits in the first, second and last block of every
    chunk, alternately a data row and a parity row, one flipped byte each: locate names them and
    leaves both arrays alone, heal restores them and changes nothing else, gaps and guards
    included."""
    torch, rsmi = gpu
    k, m, S = 3, 2, 2049
    chunk = max(1, (64 << 20) // ((k + m) * rsmi.recommended_pitch(S)))
    nb = 3 * chunk + 3
    dside, pside = Side("d", 0, S, k * S + 24), Side("p", 0, S, m * S + 40)
    with _leg("host-seam"):
        rng = np.random.default_rng(S + nb)
        data = rng.integers(0, 256, size=(nb, k, S), dtype=np.uint8)
        parity = orc.encode_fast(k, m, data, threads=8)
        clean = blank(dside, pside, nb)

        def rows(buf, side, nrows):
            return np.lib.stride_tricks.as_strided(buf[GUARD:], shape=(nb, nrows, S), strides=(side.bs, side.rs, 1))

        rows(clean["d"], dside, k)[:] = data
        rows(clean["p"], pside, m)[:] = parity
        dirty = {a: x.copy() for a, x in clean.items()}
        hit = sorted({b for c0 in range(0, nb, chunk) for b in (c0, c0 + 1, min(c0 + chunk, nb) - 1)})
        assert len(hit) == 12 and hit[-1] == nb - 1
        want = np.full(nb, CLEAN, dtype=np.int32)
        flags = np.zeros((nb, m), dtype=bool)
        for i, b in enumerate(hit):
            x = (i // 2) % k if i % 2 == 0 else k + (i // 2) % m
            side, r = side_row(k, dside, pside, x)
            dirty[side.alloc][row_at(side, b, r) + (i * 211) % S] ^= 1 << (i % 8)
            sh = np.concatenate([rows(dirty["d"], dside, k)[b], rows(dirty["p"], pside, m)[b]])
            want[b] = want_verdict(k, m, sh)
            assert want[b] == x, (b, x, want[b])   # one damaged shard, distance 3
            assert np.array_equal(want_image(k, m, sh[None], want[b:b + 1])[0], np.concatenate([data[b], parity[b]]))
            flags[b] = want_flags(k, m, sh[None])[0]
        assert {int(v) for v in want[hit]} == set(range(k + m))
        work = {a: x.copy() for a, x in dirty.items()}
        ptr = {a: x.ctypes.data + GUARD for a, x in work.items()}
        with rsmi.Codec(k, m) as c:
            c.set_option("small_call_bytes", 0)
            for heal in (False, True):
                cul = np.full(nb + 2, POISON, dtype=np.int32)
                bad = np.full(nb * m + 2, POISON, dtype=np.uint32)
                fn = c.heal_batch_host_ptr if heal else c.locate_batch_host_ptr
                fn(ptr["d"], dside.bs, ptr["p"], pside.bs, S, nb, cul.ctypes.data, bad.ctypes.data)
                assert c.last_kernel() == stripe_labels(k, m, "aligned")[2 if heal else 1] == \
                    ("rs_heal_kernel" if heal else "rs_locate_kernel") + "<K=3,MT=2>"
                got, gbad = _results(cul, bad, m, True, ("seam", heal), nb)
                assert np.array_equal(np.flatnonzero(got != CLEAN), np.array(hit)), np.flatnonzero(got != CLEAN)[:16]
                assert np.array_equal(got, want)
                assert np.array_equal(gbad, flags)
                check(work, clean if heal else dirty, ("seam", heal))
