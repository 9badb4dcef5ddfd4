"""rsmi_locate_pair, rsmi_heal_pair and rsmi_scrub with independent data and parity layouts, bit for bit.

The three calls take the two halves rsmi_verify_batch_dev takes: row c of data block b at d_data +
b*data_block_stride + c*data_shard_stride, parity row j at d_parity + b*parity_block_stride +
j*parity_shard_stride.  The other pair modules call them with one buffer, one shard stride and one
block stride for both halves, where the second row of a pair that spans the halves stored at the
other half's pitch or block stride, p0/p1 or e0/e1 of rs_heal_pair_rows_kernel taken at the wrong
stride, a_rs and b_rs swapped in rs_locate_pair_rows_kernel, home() carrying a healed row back at
the other half's block stride, small_done copying from the half that was not staged, or the scrub
kernel's par_off all give the right address.  Here the geometry model of test_layout_contract.py
(15 geometries at 3-4 sizes, 6 blocks) carries a sheet of damage through the calls; heal_pair is
the one that writes, so after it every allocation is compared whole.

The sheet of a case (its index i rotates the rows: c = i % k, j = i % m, d = (i + 1 + (i // k) %
max(1, k - 1)) % k, never c) is, from the oracle's clean stripes:
  block 0  the pair {c, k + j}, one row in each half
  block 1  the pair {c, d}, both in the data half
  block 2  the pair {k + j, k + (j + 1) % m}, both in the parity half (m >= 2)
  block 3  data row (i + 2) % k alone, byte S // 2
  block 4  three damaged shards, two bytes each: c, k + j and k + m - 1 (k where that is k + j; data
           row d at m = 1)
  block 5  clean
where a pair {x, y}, x < y, is x[min(16, S - 1)] ^= 0x40, x[S - 1] ^= 0x01, y[S - 1] ^= 0x9C (one
case has the first flip at byte 0: FIRST_FLIP_AT_0 below), and where a damaged row's pitch leaves a
byte at offset S, that padding byte is flipped in the buffer too: it changes no verdict, flag or
raw and comes back flipped.  rot moves every block on by rot places.  The verdicts are
test_locate_pair.want_pairs' (for n >= 20 its span form, which leg 0 shows equal on this sheet),
the image test_heal_pair.want_image's, the flags test_verify.want_flags', the raws go through
test_scrub.assert_raws (once per sheet, image_raws() below): none comes from the library, and
there are no tolerances.  The launch label is part of every assertion; pair_labels() below restates
launch_locate_pair, launch_heal_pair and launch_scrub.

  0  the sheet's verdicts and images, the label rule's families, the comparison rejects the slips (CPU)
  1  rsmi_locate_pair_batch_dev over every case
  2  rsmi_heal_pair_batch_dev over every case, then rsmi_scrub_batch_dev on the healed device buffers
  2b every geometry once more with rot = 3: the pair that spans the halves behind a block stride
  3  the three host entry points: mixed memory on every path, and the upload pipeline past a chunk
     boundary with different block strides
  4  16 seeds of random halves, sizes and damage through locate_pair and heal_pair

RS(10,4) and RS(6,3) run all 48 cases, one test per size; every other shape runs every geometry
once, at the sizes in turn, under its case index, one test per group of geometries.
"""
import collections
import itertools
import os
import re
import time

import numpy as np
import pytest

import oracle_lib as orc
from test_heal_pair import want_image
from test_heal_pair_fuzz import DEAL, SIZES, check_deal
from test_heal_pair_fuzz import SHAPES as FUZZ_SHAPES
from test_layout_contract import (ALIGNED_IDS, ALL_S, FILL_DATA, FILL_PARITY, GUARD, T_IDS, HostBuf, Side, blank, cases,
                                  check, download, dptr, expected_form, form_on_device, geometries, put, ref_of,
                                  round_up, row_at, small_path, upload)
from test_locate_matrix import LOCATE_KS
from test_locate_pair import CLEAN, UNKNOWN, want_pair_np, want_pairs
from test_scrub import Outputs, assert_raws, entries_of, scrub_label, want_entries
from test_scrub_abi import SCRUB_KS
from test_scrub_fuzz import draw_half
from test_stripe_layouts import COMPARE, HEAL_ROWS, LOCATE_ROWS, stripe_labels
from test_verify import stripes, want_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "filedag-storage_amd", "csrc")
NB6 = 6
POISON = 0x5EED
PAIR_SHAPES = [(10, 4), (6, 3), (16, 4), (3, 4), (7, 3), (5, 5), (20, 4), (4, 2), (2, 1)]
FULL = [(10, 4), (6, 3)]   # all 48 cases; the others every geometry once
PAIR_ROWS, HEAL_PAIR_ROWS = "rs_locate_pair_rows_kernel", "rs_heal_pair_rows_kernel"
# what the last launch of a call was: the pair kernels, the byte-granular pair kernels, rsmi_locate's
# or rsmi_heal's kernels (m = 2), Verify's (m = 1)
PAIR_FAMILIES = ["pair", "pair,UA", "pair_rows", "named", "named,UA", "named_rows", "verify", "verify,UA",
                 "compare_rows"]
FAMILIES = {"locate_pair": PAIR_FAMILIES, "heal_pair": PAIR_FAMILIES, "scrub": ["scrub", "scrub,UA", "two_pass"]}


# ---------------------------------------------------------------- the label rule, restated
def pair_labels(k, m, form):
    """(locate_pair, heal_pair, scrub): the label each call leaves on a layout of expected_form()
    form; scrub's is None where the two passes run (any label that is not the scrub kernel's).
    launch_locate_pair: launch_locate's launches, and for m <= 2 nothing else; where
    rs_locate_kernel ran (m = 3 or 4, a K with a kernel, aligned or UA) rs_locate_pair_kernel, else
    the rows kernel.  launch_heal_pair: locate_pair's launches; m = 1 nothing more, m = 2
    launch_heal_named, else rs_heal_pair_kernel where rs_locate_pair_kernel ran and the rows kernel
    where the rows kernel did.  launch_scrub: rs_scrub_mfma_kernel for a one-tile plan of a K with
    a kernel on an aligned or UA layout, else Verify and the CRC-16 rows pass."""
    _, named_locate, named_heal = stripe_labels(k, m, form)
    ua = ",UA" if form == "ua" else ""
    if m <= 2:
        locate = named_locate
    elif m in (3, 4) and k in LOCATE_KS and form in ("aligned", "ua"):
        locate = "rs_locate_pair_kernel<K=%d,MT=%d>%s" % (k, m, ua)
    else:
        locate = PAIR_ROWS
    if m == 1:
        heal = locate
    elif m == 2:
        heal = named_heal
    elif locate != PAIR_ROWS:
        heal = "rs_heal_pair_kernel<K=%d,MT=%d>%s" % (k, m, ua)
    else:
        heal = HEAL_PAIR_ROWS
    scrub = None
    if m <= 4 and k in SCRUB_KS and form in ("aligned", "ua"):
        scrub = scrub_label(k, m, form == "aligned")
    return locate, heal, scrub


def family(label):
    for prefix, fam in (("rs_locate_pair_kernel<", "pair"), ("rs_heal_pair_kernel<", "pair"),
                        ("rs_locate_kernel<", "named"), ("rs_heal_kernel<", "named"), ("rs_verify_kernel<", "verify"),
                        ("rs_scrub_mfma_kernel<", "scrub")):
        if label.startswith(prefix):
            return fam + (",UA" if label.endswith(",UA") else "")
    return {PAIR_ROWS: "pair_rows", HEAL_PAIR_ROWS: "pair_rows", LOCATE_ROWS: "named_rows", HEAL_ROWS: "named_rows",
            COMPARE: "compare_rows"}[label]


def scrub_family(label):
    return family(label) if label.startswith("rs_scrub") else "two_pass"


# ---------------------------------------------------------------- the cases
# the geometries in three groups, one test each: aligned, one term of the predicate broken, the rest
GROUPS = collections.OrderedDict([("aligned", ALIGNED_IDS), ("one-term", T_IDS),
                                  ("rows", ["split-in", "split-out", "phases"])])


def once_per_geometry(k, m, group=None):
    """Every geometry (of a group, when one is given) once, at the sizes in turn, under its case
    index of cases()."""
    by_gid = collections.OrderedDict()
    for i, (gid, S, d, p, form) in enumerate(cases(k, m, NB6)):
        by_gid.setdefault(gid, []).append((i, gid, S, d, p, form))
    for j, at in enumerate(by_gid.values()):
        if group is None or at[0][1] in GROUPS[group]:
            yield at[j % len(at)]


def shape_cases(k, m, part=None):
    """(i, gid, S, data side, parity side, form) of the cases legs 1 and 2 run for a shape: all 48
    for the shapes of FULL (part: a size), every geometry once for the rest (part: a group)."""
    if (k, m) not in FULL:
        yield from once_per_geometry(k, m, part)
        return
    for i, (gid, s, d, p, form) in enumerate(cases(k, m, NB6)):
        if part is None or s == part:
            yield i, gid, s, d, p, form


DEVICE_PARAMS = [(k, m, S) for k, m in FULL for S in ALL_S] + \
                [(k, m, g) for k, m in PAIR_SHAPES if (k, m) not in FULL for g in GROUPS]
DEVICE_IDS = ["%d-%d-%s" % (k, m, "S%d" % part if isinstance(part, int) else part) for k, m, part in DEVICE_PARAMS]
LATER_PARAMS = [(k, m, g) for k, m in PAIR_SHAPES for g in GROUPS]
LATER_IDS = ["%d-%d-%s" % prm for prm in LATER_PARAMS]


# ---------------------------------------------------------------- the sheet
Sheet = collections.namedtuple("Sheet", "sh verdicts flags image image_flags raws damaged moved")
_SHEETS = {}


def case_rows(k, m, i):
    return i % k, i % m, (i + 1 + (i // k) % max(1, k - 1)) % k


def third_row(k, m, j, d):
    """Block 4's third damaged shard."""
    if m == 1:
        return d
    return k + m - 1 if k + m - 1 != k + j else k


# Rows of at most 17 bytes take all of a pair's damage in one byte column, which at m = 3 a second
# pair may explain as well (test_locate_pair.py::test_ambiguity_at_m3).  Of the sheets of this module
# that happens once, at RS(6,3), S = 17, case 10, block 1 ({0, 4}): there the first flip of the first
# row is at byte 0, a column of its own.  (k, m, S, c, j, d) -> blocks
FIRST_FLIP_AT_0 = {(6, 3, 17, 4, 1, 0): (1,)}


def damage_pair(sh, b, x, y, first=None):
    S = sh.shape[2]
    x, y = min(x, y), max(x, y)
    sh[b, x, min(16, S - 1) if first is None else first] ^= 0x40   # S <= 17: the next line's byte, two masks
    sh[b, x, S - 1] ^= 0x01
    sh[b, y, S - 1] ^= 0x9C


def definition(k, m, sh):
    """The verdicts of the definition: want_pairs, for codes of 20 shards and more in its span form
    (test_locate_pair_abi.py::test_span_form_equals_oracle_form; leg 0 compares the two here)."""
    if k + m >= 20:
        return np.array([want_pair_np(k, m, sh[b]) for b in range(sh.shape[0])], dtype=np.int32).reshape(-1, 2)
    return want_pairs(k, m, sh)


def image_raws(image, ctx):
    """R(row) of every row of image (nb, n, S), computed once per sheet for the device legs: the
    oracle's checksum of the row, through rsmi_crc16_entry's being affine in raw over GF(2) (with an
    empty head raw = checksum ^ entry(raw = 0)), and then through test_scrub.assert_raws, the
    byte-serial CRC-16 of the rows.  At a fixed S the entry is a bijection of raw, so assert_raws
    accepts exactly this one value per row: a device output equal to it is one assert_raws accepts."""
    import rsmi

    raws = want_entries(image) ^ np.uint32(rsmi.crc16_entry(b"", 0, image.shape[2]))
    assert_raws(rsmi, raws, image, ctx)
    return raws


def sheet(k, m, S, i, rot=0):
    """The damaged stripes of case index i and the definition's answers for them, computed once
    per (k, m, S, c, j, d): the rows alone decide, never the geometry.  Read-only.  rot moves block
    b, stripe and damage, to block (b + rot) % 6 (leg 2b: with the sheet as it stands the pair that
    spans the halves sits in block 0, where no block stride enters an address); the definition is
    one block's, so its answers move with the blocks."""
    c, j, d = case_rows(k, m, i)
    key = (k, m, S, c, j, d, rot)
    if key in _SHEETS:
        return _SHEETS[key]
    if rot:
        base = sheet(k, m, S, i)
        arrays = [np.roll(a, rot, axis=0) for a in base[:6]]
        damaged = tuple(((b + rot) % NB6, x) for b, x in base.damaged)
        moved = tuple((b + rot) % NB6 for b in base.moved)
    else:
        ref = ref_of(k, m, S, NB6)
        sh = np.concatenate([ref.data, ref.parity], axis=1)
        rows = [(c, k + j), (c, d), (k + j, k + (j + 1) % m) if m >= 2 else (), ((i + 2) % k,),
                (c, k + j, third_row(k, m, j, d)), ()]
        assert c != d and len(set(rows[4])) == 3
        moved = FIRST_FLIP_AT_0.get(key[:6], ())
        for b in (0, 1, 2):
            if rows[b]:
                damage_pair(sh, b, *rows[b], first=0 if b in moved else None)
        sh[3, (i + 2) % k, S // 2] ^= 0x21
        three = ((0, S - 1, 0x11, 0x22), (1, S - 2, 0x33, 0x44), (2, S - 3, 0x55, 0x66))
        for x, (lo, hi, e0, e1) in zip(rows[4], three):
            sh[4, x, lo] ^= e0
            sh[4, x, hi] ^= e1
        verdicts = definition(k, m, sh)
        image = want_image(k, m, sh, verdicts)
        arrays = [sh, verdicts, want_flags(k, m, sh), image, want_flags(k, m, image), image_raws(image, key)]
        damaged = tuple((b, x) for b in range(NB6) for x in rows[b])
    for a in arrays:
        a.setflags(write=False)
    _SHEETS[key] = Sheet(*arrays, damaged, moved)
    return _SHEETS[key]


def side_row(k, d, p, x):
    """The side and the row within it of shard x."""
    return (d, x) if x < k else (p, x - k)


def before_of(k, m, S, sht, d, p, nb=NB6):
    """(buffers, padding spots): the sheet laid out by the two sides, and the byte at offset S of
    every damaged row whose pitch leaves one flipped."""
    bufs = blank(d, p, nb)
    put(bufs, d, sht.sh[:, :k])
    put(bufs, p, sht.sh[:, k:])
    pads = []
    for b, x in sht.damaged:
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
def _assert_sheet(k, m, S, i, sht, rot, ctx):
    """What the sheet is meant to produce, of the definition's answers (block numbers: before rot)."""
    c, j, d = case_rows(k, m, i)
    ref = ref_of(k, m, S, NB6)
    full = np.concatenate([ref.data, ref.parity], axis=1)
    v = np.roll(sht.verdicts, -rot, axis=0).tolist()
    sh, image = np.roll(sht.sh, -rot, axis=0), np.roll(sht.image, -rot, axis=0)
    flags, image_flags = np.roll(sht.flags, -rot, axis=0), np.roll(sht.image_flags, -rot, axis=0)
    pairs = [[c, k + j], sorted([c, d]), sorted([k + j, k + (j + 1) % m])]
    if m >= 3:
        assert v[:3] == pairs, ctx + (v,)
    elif m == 2:  # no pair is ever named: UNKNOWN, or the one shard that imitates the two
        assert all(x == [UNKNOWN, UNKNOWN] or (0 <= x[0] < k + m and x[1] == CLEAN) for x in v[:3]), ctx + (v,)
    else:
        assert v[:3] == [[UNKNOWN, UNKNOWN], [UNKNOWN, UNKNOWN], [CLEAN, CLEAN]], ctx + (v,)
    assert v[3] == ([(i + 2) % k, CLEAN] if m >= 2 else [UNKNOWN, UNKNOWN]), ctx + (v,)
    assert v[4] == [UNKNOWN, UNKNOWN] and v[5] == [CLEAN, CLEAN], ctx + (v,)
    for b in range(NB6):
        if v[b][0] < 0:
            assert np.array_equal(image[b], sh[b]), ctx + (b,)
        elif m >= 3 or b == 3:  # the damaged rows, named: the undamaged stripe
            assert np.array_equal(image[b], full[b]), ctx + (b,)
        assert image_flags[b].any() == (v[b][0] == UNKNOWN), ctx + (b,)
    # flags: a damaged data row raises all m, a parity row its own
    for b in (0, 1, 3, 4):
        assert flags[b].all(), ctx + (b,)
    assert flags[2].tolist() == [m >= 2 and l in (j, (j + 1) % m) for l in range(m)], ctx
    assert not flags[5].any(), ctx
    assert sorted(sht.damaged) == sorted(set(sht.damaged))
    assert len(sht.damaged) == 2 + 2 + 2 * (m >= 2) + 1 + 3, ctx
    assert not sht.moved or (m == 3 and S <= 17), ctx + (sht.moved,)   # FIRST_FLIP_AT_0
    return v


@pytest.mark.parametrize("k,m", PAIR_SHAPES)
def test_sheet_is_what_the_definition_says(k, m):
    """For every case of the shape, and for leg 2b's cases at rot = 3: m >= 3 names each of the
    three pairs and heals them to the undamaged stripe, m >= 2 names the one damaged data row of
    block 3, three damaged shards are (-2, -2) and left as they are, the clean block is (-1, -1);
    an UNKNOWN block alone keeps its flags.  Over a 48-case shape every data row is the first row
    of a named pair and every parity row the second row of a pair that spans the halves."""
    first, second, n_cases = set(), set(), 0
    for i, gid, S, d, p, form in shape_cases(k, m):
        ctx = (k, m, gid, S, i)
        sht = sheet(k, m, S, i)
        v = _assert_sheet(k, m, S, i, sht, 0, ctx)
        if m >= 3:
            first.update((v[0][0], v[1][0]))
            second.add(v[0][1])
        # the buffers: the padding bytes are flipped where there is one and are no row's byte
        before, pads = before_of(k, m, S, sht, d, p)
        want = healed_of(k, sht, d, p, before)
        for a, o in pads:
            assert before[a][o] == want[a][o] and before[a][o] in (FILL_DATA ^ 0xFF, FILL_PARITY ^ 0xFF), ctx
        assert len(pads) == sum(side_row(k, d, p, x)[0].rs > S for _, x in sht.damaged), ctx
        n_cases += 1
    assert n_cases == (48 if (k, m) in FULL else 15)
    if (k, m) in FULL:
        assert first >= set(range(k)), (k, m, sorted(set(range(k)) - first))
        assert second == set(range(k, k + m)), (k, m, sorted(second))
    later = list(once_per_geometry(k, m))
    assert sorted(g for _, g, _, _, _, _ in later) == sorted(geometries(k, m, 1000, NB6))
    by_group = [x for g in GROUPS for x in once_per_geometry(k, m, g)]   # the groups are all of them, once
    assert len(by_group) == len(later) and all(x in later for x in by_group)
    assert len({S for _, _, S, _, _, _ in later}) >= 3
    for n, (i, gid, S, d, p, form) in enumerate(later):
        sht = sheet(k, m, S, i, 3)
        _assert_sheet(k, m, S, i, sht, 3, (k, m, gid, S, i, "rot 3"))
        assert sht.damaged[0] == (3, i % k) and sht.damaged[1] == (3, k + i % m)  # the pair that spans the halves
        if n == 0:  # the answers moved with the blocks: the definition once more, on the moved stripes
            assert np.array_equal(definition(k, m, sht.sh), sht.verdicts)
            assert np.array_equal(want_image(k, m, sht.sh, sht.verdicts), sht.image)


@pytest.mark.parametrize("k,m", [(16, 4), (20, 4)])
def test_span_form_is_the_definition_on_this_sheet(k, m):
    """definition() takes want_pair_np for these two shapes: on a sheet of each (every kind of
    block) it gives what want_pairs gives through the oracle's reconstruct."""
    i, gid, S, d, p, form = next(iter(once_per_geometry(k, m)))
    sht = sheet(k, m, S, i)
    assert np.array_equal(want_pairs(k, m, sht.sh), sht.verdicts)


def test_label_rule_reaches_every_family():
    """Over PAIR_SHAPES x cases the rule gives every family to each of the three calls."""
    count = {call: collections.Counter() for call in FAMILIES}
    for k, m in PAIR_SHAPES:
        for i, gid, S, d, p, form in shape_cases(k, m):
            assert form == expected_form(GUARD + d.off, d.rs, d.bs, GUARD + p.off, p.rs, p.bs, S)
            lo, he, sc = pair_labels(k, m, form)
            count["locate_pair"][family(lo)] += 1
            count["heal_pair"][family(he)] += 1
            count["scrub"]["two_pass" if sc is None else scrub_family(sc)] += 1
            assert family(lo) == family(he)
            assert (m == 1) == (lo == he)
            assert lo.endswith(",UA") == (form == "ua" and not family(lo).endswith("_rows"))
            assert (sc is None) == (form == "generic" or m > 4 or k not in SCRUB_KS)
    for call, fams in FAMILIES.items():
        for fam in fams:
            assert count[call][fam] > 0, (call, fam, dict(count[call]))
    assert pair_labels(10, 4, "aligned") == ("rs_locate_pair_kernel<K=10,MT=4>", "rs_heal_pair_kernel<K=10,MT=4>",
                                             "rs_scrub_mfma_kernel<K=10,MT=4>")
    assert pair_labels(3, 4, "ua") == ("rs_locate_pair_kernel<K=3,MT=4>,UA", "rs_heal_pair_kernel<K=3,MT=4>,UA",
                                       "rs_scrub_mfma_kernel<K=3,MT=4>,UA")
    assert pair_labels(6, 3, "generic") == (PAIR_ROWS, HEAL_PAIR_ROWS, None)
    assert pair_labels(7, 3, "aligned") == pair_labels(20, 4, "ua") == pair_labels(5, 5, "ua") == \
        (PAIR_ROWS, HEAL_PAIR_ROWS, None)
    assert pair_labels(4, 2, "ua") == ("rs_locate_kernel<K=4,MT=2>,UA", "rs_heal_kernel<K=4,MT=2>,UA",
                                       "rs_scrub_mfma_kernel<K=4,MT=2>,UA")
    assert pair_labels(4, 2, "generic") == (LOCATE_ROWS, HEAL_ROWS, None)
    assert pair_labels(2, 1, "aligned") == ("rs_verify_kernel<K=2,MT=1>",) * 2 + ("rs_scrub_mfma_kernel<K=2,MT=1>",)
    assert pair_labels(2, 1, "generic") == (COMPARE, COMPARE, None)


def test_label_rule_matches_source():
    """The branches pair_labels() restates are the ones launch_locate_pair, launch_heal_pair and
    launch_scrub have, and the pair kernels are built for the K and m the rule says: an edit to
    them fails here instead of silently retargeting the cases."""
    src = {}
    for name in ("rsmi_pair.cpp", "rsmi_heal_pair.cpp", "rsmi_scrub.cpp", "rs_pair_kernels.hip",
                 "rs_heal_pair_kernels.hip", "rs_scrub_kernels.hip"):
        with open(os.path.join(CSRC, name)) as f:
            src[name] = " ".join(f.read().split())
    pair, heal, scrub = src["rsmi_pair.cpp"], src["rsmi_heal_pair.cpp"], src["rsmi_scrub.cpp"]
    assert "if ((rc = launch_locate(c, plan, rows, culprit, bad, stream, &fused))) return rc;" in pair
    assert ("if (c->m <= 2) { if ((rc = launch_pair_verdict(culprit, nullptr, n32, 0, nblocks, out, stream))) "
            "return rc; return hip_status(hipGetLastError()); }") in pair
    assert "if (fused != StripeLayout::kNeither) {" in pair
    # stripe_kernel and tiles_launched (rsmi_verify.cpp; tests/test_stripe_layouts.py pins them):
    # null for kNeither or K > 16, else the layout's table entry; "rs_<name>_kernel<K=..,MT=..>[,UA]"
    assert "void* fn = stripe_kernel(pair_kernels(), fused, t);" in pair
    assert 'return tiles_launched(c, "locate_pair", fused, t);' in pair
    assert 'set_last_kernel(c, "rs_locate_pair_rows_kernel");' in pair
    assert "int rc = launch_locate_pair(c, plan, rows, out, bad, stream, &pl);" in heal
    assert "if (c->m == 1) return RSMI_OK;" in heal
    assert "if (c->m == 2) return launch_heal_named(c, plan, pl.fused, rows, pl.culprit, stream);" in heal
    assert "if (pl.fused != StripeLayout::kNeither) {" in heal
    assert "void* fn = stripe_kernel(heal_pair_kernels(), pl.fused, t);" in heal
    assert 'return tiles_launched(c, "heal_pair", pl.fused, t);' in heal
    assert ('return launch_heal_rows(c, plan, heal_pair_rows_kernel(), "rs_heal_pair_rows_kernel", rows, out, 2, '
            "stream);") in heal
    assert "const StripeLayout layout = rows.layout();" in scrub
    assert ("void* fn = plan.tiles.size() == 1 ? stripe_kernel(scrub_kernels(), layout, plan.tiles[0]) : nullptr;"
            in scrub)
    assert "if (!fn) {" in scrub
    assert 'return tiles_launched(c, "scrub_mfma", layout, tile);' in scrub
    # the entry points hand the caller's six numbers on unchanged, in the header's order, and
    # stripe_dev_call builds the rows from them in that order
    tail = ("d_data, data_shard_stride, data_block_stride, d_parity, parity_shard_stride, parity_block_stride, S, "
            "nblocks, ")
    with open(os.path.join(CSRC, "rsmi_impl.hpp")) as f:
        impl = " ".join(f.read().split())
    assert impl.count("return launch(*plan, StripeRows{d_data, data_shard_stride, data_block_stride, d_parity, "
                      "parity_shard_stride, parity_block_stride, S, nblocks});") == 1
    assert ("const uint8_t* data = nullptr; uint64_t data_rs = 0, data_bs = 0; const uint8_t* parity = nullptr; "
            "uint64_t parity_rs = 0, parity_bs = 0; uint64_t S = 0, nblocks = 0;") in impl
    for text, out, call in ((pair, "d_pair_out", "launch_locate_pair(c, plan, rows, d_pair_out, d_bad_out,"),
                            (heal, "d_pair_out", "launch_heal_pair(c, plan, rows, d_pair_out, d_bad_out,"),
                            (scrub, "d_bad_out && d_raw_out ? d_bad_out : nullptr",
                             "launch_scrub(c, plan, rows, d_bad_out, d_raw_out,")):
        assert text.count("return stripe_dev_call( c, " + tail + out +
                          ", [&](const Plan& plan, const StripeRows& rows) { return " + call) == 1, call
    for name, fill, mts in (("rs_pair_kernels.hip", "fill_pair", [3, 4]),
                            ("rs_heal_pair_kernels.hip", "fill_heal_pair", [3, 4]),
                            ("rs_scrub_kernels.hip", "fill_scrub", [1, 2, 3, 4])):
        ks = sorted(int(x) for x in re.findall(fill + r"_k<(\d+)>\(x\);", src[name]))
        assert ks == (SCRUB_KS if fill == "fill_scrub" else LOCATE_KS), (name, ks)
        assert sorted(int(x) for x in re.findall(fill + r"_km<K, (\d+)>\(t\);", src[name])) == mts, name


def _at(side, b, r):
    """The side whose row (0, 0) is side's row (b, r): put() of one row."""
    return side._replace(off=side.off + b * side.bs + r * side.rs)


def test_checker_rejects_simulated_slips():
    """RS(10,4), S = 1000, five geometries, rot 0 and 3: "got" buffers built on the CPU with every
    block healed and the two rows of the pair that spans the halves where a slip would have stored
    them (and their damage left where it was) are each rejected by check(), wherever the slip's
    address really differs from the right one; the right image, built the same way, passes."""
    k, m, S, i = 10, 4, 1000, 13
    c, j, _ = case_rows(k, m, i)
    assert (c, j) == (3, 1)
    R = round_up(S, 16)
    tried = skipped = 0
    for rot, gid in itertools.product((0, 3), ("A0", "A0m", "split-in", "phases", "interleaved")):
        sht = sheet(k, m, S, i, rot)
        assert sht.verdicts[rot].tolist() == [c, k + j]
        d, p = geometries(k, m, S, NB6)[gid]
        before, _ = before_of(k, m, S, sht, d, p)
        want = healed_of(k, sht, d, p, before)
        with pytest.raises(AssertionError):
            check(before, want, (gid, "nothing healed"))
        healed = [(rot, c, d, c), (rot, k + j, p, j)]   # (block, shard, side, row within the side)

        def stored(wrong):
            got = {a: v.copy() for a, v in before.items()}
            for b in range(NB6):
                if b != rot:
                    put(got, _at(d, b, 0), sht.image[b:b + 1, :k])
                    put(got, _at(p, b, 0), sht.image[b:b + 1, k:])
            for b, x, side, r in healed:
                put(got, _at(wrong.get(x, side), b, r), sht.image[b, x][None, None], clip=True)
            return got

        check(stored({}), want, (rot, gid, "good"))
        # slip -> the side each healed row is stored through
        slips = collections.OrderedDict([
            ("parity row at data_rs", {k + j: p._replace(rs=d.rs)}),
            ("parity row at data_bs", {k + j: p._replace(bs=d.bs)}),
            ("data row at parity_rs", {c: d._replace(rs=p.rs)}),
            ("data row at parity_bs", {c: d._replace(bs=p.bs)}),
            ("into the other allocation", {c: d._replace(alloc=p.alloc), k + j: p._replace(alloc=d.alloc)}),
            ("the second row through the first row's side", {k + j: d}),
        ])
        for name, wrong in slips.items():
            tried += 1
            differs = any((wrong[x].alloc, row_at(wrong[x], b, r)) != (side.alloc, row_at(side, b, r))
                          for b, x, side, r in healed if x in wrong)
            if not differs:
                skipped += 1
                assert (rot == 0 and name.endswith("_bs")) or gid == "interleaved", (rot, gid, name)
                continue
            with pytest.raises(AssertionError):
                check(stored(wrong), want, (rot, gid, name))
        # the rows' last chunk stored as 16 whole bytes: bytes S .. round_up(S, 16) change
        tried += 1
        got = {a: v.copy() for a, v in want.items()}
        for b, x, side, r in healed:
            o = row_at(side, b, r)
            got[side.alloc][o + S:o + R] = 0
        with pytest.raises(AssertionError):
            check(got, want, (rot, gid, "whole last chunk"))
    assert tried == 70 and skipped * 4 < tried, (tried, skipped)


# ---------------------------------------------------------------- GPU plumbing
SEEN = collections.Counter()
LEGS = set()
WALL = collections.OrderedDict()
SLOWEST = {}
ALL_LEGS = {(leg, prm) for leg in ("locate_pair", "heal_pair") for prm in DEVICE_PARAMS} | \
           {("later-blocks", prm) for prm in LATER_PARAMS}


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    rsmi = pytest.importorskip("rsmi")
    if not torch.cuda.is_available() or rsmi.device_count() == 0:
        pytest.skip("no GPU")
    assert (rsmi.LocateClean, rsmi.LocateUnknown) == (CLEAN, UNKNOWN)
    yield torch, rsmi
    for call, fams in FAMILIES.items():
        print("\npair layouts: %s calls run and asserted by label, per family:" % call,
              ", ".join("%s %d" % (f, SEEN[call, f]) for f in fams), end="")
    print("\npair layouts: wall seconds per leg:", ", ".join("%s %.2f" % kv for kv in WALL.items()))
    top = sorted(SLOWEST.items(), key=lambda kv: -kv[1])[:5]
    print("pair layouts: slowest tests, wall seconds:", ", ".join("%s %.3f" % kv for kv in top))
    if LEGS >= ALL_LEGS:  # the device legs ran whole
        for call, fams in FAMILIES.items():
            for f in fams:
                assert SEEN[call, f] > 0, (call, f)


class _leg:
    def __init__(self, name, test):
        self.name, self.test = name, "%s[%s]" % (name, test)

    def __enter__(self):
        self.t0 = time.perf_counter()

    def __exit__(self, *a):
        dt = time.perf_counter() - self.t0
        WALL[self.name] = WALL.get(self.name, 0.0) + dt
        SLOWEST[self.test] = dt


def _outputs(torch, m, nb=NB6):
    return (torch.full((2 * nb + 2,), POISON, dtype=torch.int32, device="cuda"),
            torch.full((nb * m + 2,), POISON, dtype=torch.int32, device="cuda"))


def _results(out, bad, m, flags, ctx, nb=NB6):
    """The verdicts (nb, 2) and the flags as bool (None when no pointer was given); the two words
    past each output's end, and the flags nobody asked for, are still poisoned."""
    out, bad = np.asarray(out), np.asarray(bad)
    assert (out[2 * nb:] == POISON).all() and (bad[nb * m:] == POISON).all(), ctx + ("wrote past its outputs",)
    if not flags:
        assert (bad == POISON).all(), ctx
        return out[:2 * nb].reshape(nb, 2), None
    return out[:2 * nb].reshape(nb, 2), bad[:nb * m].reshape(nb, m) != 0


def _scrub_label_ok(got, want, ctx):
    if want is None:
        assert got and not got.startswith("rs_scrub"), (got,) + ctx
    else:
        assert got == want, (got, want) + ctx


# ---------------------------------------------------------------- leg 1: rsmi_locate_pair_batch_dev
@pytest.mark.gpu
@pytest.mark.parametrize("k,m,part", DEVICE_PARAMS, ids=DEVICE_IDS)
def test_locate_pair_independent_layouts(gpu, k, m, part):
    """Every case through rsmi_locate_pair_batch_dev, with the flags pointer on even case indices
    and without on odd ones (the scratch copy is used, the caller's tensor stays poisoned): the
    label of the rule, two verdict words per block and the flags of the definition, the two words
    past each output poisoned, every allocation byte for byte as uploaded."""
    torch, rsmi = gpu
    h = torch.cuda.current_stream().cuda_stream
    with _leg("locate_pair", (k, m, part)), rsmi.Codec(k, m) as c:
        for i, gid, s, d, p, form in shape_cases(k, m, part):
            ctx = (k, m, gid, s, i)
            sht = sheet(k, m, s, i)
            host, _ = before_of(k, m, s, sht, d, p)
            dev = upload(torch, host)
            form_on_device(dev, d, p, s, form)
            label = pair_labels(k, m, form)[0]
            flags = i % 2 == 0
            out, bad = _outputs(torch, m)
            c.locate_pair_batch_dev(dptr(dev, d), d.rs, d.bs, dptr(dev, p), p.rs, p.bs, s, NB6, out.data_ptr(),
                                    bad.data_ptr() if flags else 0, h)
            torch.cuda.synchronize()
            assert c.last_kernel() == label, (c.last_kernel(), label) + ctx
            got, gbad = _results(out.cpu().numpy(), bad.cpu().numpy(), m, flags, ctx)
            assert np.array_equal(got, sht.verdicts), ctx + (got.tolist(), sht.verdicts.tolist())
            if flags:
                assert np.array_equal(gbad, sht.flags), ctx + (gbad.tolist(),)
            check(download(dev), host, ctx + ("locate_pair wrote to the shards",))
            SEEN["locate_pair", family(label)] += 1
    LEGS.add(("locate_pair", (k, m, part)))


# ---------------------------------------------------------------- leg 2: rsmi_heal_pair_batch_dev, rsmi_scrub_batch_dev
def _heal_case(torch, rsmi, c, k, m, gid, S, i, d, p, form, rot=0):
    """One rsmi_heal_pair_batch_dev and, behind it on the stream, one rsmi_scrub_batch_dev over the
    sheet of case i laid out by (d, p); returns (heal's label, scrub's label)."""
    ctx = (k, m, gid, S, i, rot)
    h = torch.cuda.current_stream().cuda_stream
    sht = sheet(k, m, S, i, rot)
    host, pads = before_of(k, m, S, sht, d, p)
    want = healed_of(k, sht, d, p, host)
    dev = upload(torch, host)
    form_on_device(dev, d, p, S, form)
    _, label, slabel = pair_labels(k, m, form)
    flags = i % 2 == 1
    out, bad = _outputs(torch, m)
    scr = Outputs(torch, NB6, k, m)
    c.heal_pair_batch_dev(dptr(dev, d), d.rs, d.bs, dptr(dev, p), p.rs, p.bs, S, NB6, out.data_ptr(),
                          bad.data_ptr() if flags else 0, h)
    healed_by = c.last_kernel()
    c.scrub_batch_dev(dptr(dev, d), d.rs, d.bs, dptr(dev, p), p.rs, p.bs, S, NB6, scr.bad_ptr, scr.raw_ptr, h)
    torch.cuda.synchronize()
    scrubbed_by = c.last_kernel()
    assert healed_by == label, (healed_by, label) + ctx
    _scrub_label_ok(scrubbed_by, slabel, ctx)
    got, gbad = _results(out.cpu().numpy(), bad.cpu().numpy(), m, flags, ctx)
    assert np.array_equal(got, sht.verdicts), ctx + (got.tolist(), sht.verdicts.tolist())
    if flags:
        assert np.array_equal(gbad, sht.flags), ctx + (gbad.tolist(),)
    after = download(dev)
    check(after, want, ctx)
    for a, o in pads:
        assert after[a][o] in (FILL_DATA ^ 0xFF, FILL_PARITY ^ 0xFF), ctx
    sflags, raws = scr.read()   # asserts the guard words
    assert np.array_equal(sflags, sht.image_flags), ctx + (sflags.tolist(),)
    assert np.array_equal(raws, sht.raws), ctx + (np.argwhere(raws != sht.raws)[:4].tolist(),)   # image_raws()
    return label, scrubbed_by


@pytest.mark.gpu
@pytest.mark.parametrize("k,m,part", DEVICE_PARAMS, ids=DEVICE_IDS)
def test_heal_pair_then_scrub_independent_layouts(gpu, k, m, part):
    """The same cases through rsmi_heal_pair_batch_dev (the flags pointer on odd case indices),
    then, with no host copy in between, rsmi_scrub_batch_dev on the same device buffers: the labels
    of the rule, the definition's verdicts and flags, and every allocation, whole, "before" with
    the image's rows put back at their own sides: guards, gaps, padding, the flipped padding bytes,
    the UNKNOWN block and the clean block unchanged.  The scrub's flags are exactly those of the
    image (set for the UNKNOWN block and for nothing else), its raws the CRC-16 of the image's
    rows, its outputs' guard words intact."""
    torch, rsmi = gpu
    with _leg("heal_pair", (k, m, part)), rsmi.Codec(k, m) as c:
        for i, gid, s, d, p, form in shape_cases(k, m, part):
            label, slabel = _heal_case(torch, rsmi, c, k, m, gid, s, i, d, p, form)
            SEEN["heal_pair", family(label)] += 1
            SEEN["scrub", scrub_family(slabel)] += 1
    LEGS.add(("heal_pair", (k, m, part)))


@pytest.mark.gpu
@pytest.mark.parametrize("k,m,group", LATER_PARAMS, ids=LATER_IDS)
def test_heal_pair_spanning_pair_in_a_later_block(gpu, k, m, group):
    """Leg 2b.  In the sheet as it stands the pair that spans the halves is in block 0, whose rows'
    addresses no block stride enters, so its parity row stored at b * data_block_stride would pass
    leg 2.  Every geometry once more with every block moved on by three: that pair in block 3.  Leg
    2's assertions."""
    torch, rsmi = gpu
    with _leg("later-blocks", (k, m, group)), rsmi.Codec(k, m) as c:
        for i, gid, S, d, p, form in once_per_geometry(k, m, group):
            _heal_case(torch, rsmi, c, k, m, gid, S, i, d, p, form, rot=3)
    LEGS.add(("later-blocks", (k, m, group)))


# ---------------------------------------------------------------- leg 3: the host entry points
HOST_K, HOST_M, HOST_S, HOST_I = 10, 4, 2049, 37   # case 37 of RS(10,4) is one of S = 2049: leg 0's sheet
HOST_TOTAL = NB6 * (HOST_K + HOST_M) * HOST_S
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


def _host_pair_call(fn, m, dptr_, dbs, pptr, pbs, S, nb, ctx):
    out = np.full(2 * nb + 2, POISON, dtype=np.int32)
    bad = np.full(nb * m + 2, POISON, dtype=np.uint32)
    fn(dptr_, dbs, pptr, pbs, S, nb, out.ctypes.data, bad.ctypes.data)
    return _results(out, bad, m, True, ctx, nb)


def _host_scrub_call(c, dptr_, dbs, pptr, pbs, S, nb, ctx):
    m, n = c.m, c.k + c.m
    bad = np.full(nb * m + 2, POISON, dtype=np.uint32)
    raw = np.full(nb * n + 2, POISON, dtype=np.uint32)
    c.scrub_batch_host_ptr(dptr_, dbs, pptr, pbs, S, nb, bad.ctypes.data, raw.ctypes.data)
    assert (bad[nb * m:] == POISON).all() and (raw[nb * n:] == POISON).all(), ctx + ("wrote past its outputs",)
    return bad[:nb * m].reshape(nb, m) != 0, raw[:nb * n].reshape(nb, n)


@pytest.mark.gpu
@pytest.mark.parametrize("parity_pinned", [True, False], ids=["parity-locked", "parity-pageable"])
@pytest.mark.parametrize("data_pinned", [True, False], ids=["data-locked", "data-pageable"])
@pytest.mark.parametrize("path", list(HOST_PATHS))
def test_host_mixed_memory(gpu, path, data_pinned, parity_pinned):
    """rsmi_locate_pair_batch_host, rsmi_heal_pair_batch_host and, on the healed arrays,
    rsmi_scrub_batch_host: RS(10,4), S = 2049, 6 blocks with gaps (dbs = k*S + 24, pbs = m*S + 40),
    64 guard bytes around each side, either side page-locked or pageable, on the in-place path, the
    small staged call (which stages only the pageable side, so the one kernel runs with the
    caller's block stride on one side and the staging's on the other, and small_done carries home
    the rows of the staged side alone) and the upload pipeline (which copies a healed row home at
    the caller's own block stride), the sheet as it stands and at rot = 3.  Both arrays whole,
    verdicts, flags and raws against the definition.  The label ends ",UA" exactly where one kernel
    reads the caller's rows or the staging at pitch S."""
    torch, rsmi = gpu
    k, m, S = HOST_K, HOST_M, HOST_S
    zero_copy, X = HOST_PATHS[path]
    one_kernel = small_path(zero_copy, data_pinned, parity_pinned, HOST_TOTAL, X)
    form = "ua" if one_kernel else "aligned"
    db = HostBuf(rsmi, k, S, k * S + 24, FILL_DATA, data_pinned, NB6)
    pb = HostBuf(rsmi, m, S, m * S + 40, FILL_PARITY, parity_pinned, NB6)
    try:
        with _leg("host", "-".join((path, str(data_pinned), str(parity_pinned)))), rsmi.Codec(k, m) as c:
            c.set_option("zero_copy", zero_copy)
            c.set_option("small_call_bytes", X)
            for rot in (0, 3):
                ctx = (path, data_pinned, parity_pinned, rot)
                sht = sheet(k, m, S, HOST_I, rot)
                assert sht.verdicts[rot].tolist() == [HOST_I % k, k + HOST_I % m]
                db.a[:] = FILL_DATA
                pb.a[:] = FILL_PARITY
                put({"h": db.a}, db.side, sht.sh[:, :k])
                put({"h": pb.a}, pb.side, sht.sh[:, k:])
                before = {"d": db.a.copy(), "p": pb.a.copy()}
                healed = {"d": db.a.copy(), "p": pb.a.copy()}
                put({"h": healed["d"]}, db.side, sht.image[:, :k])
                put({"h": healed["p"]}, pb.side, sht.image[:, k:])
                args = (db.ptr, db.side.bs, pb.ptr, pb.side.bs, S, NB6)
                for call, fn, want in (("locate_pair", c.locate_pair_batch_host_ptr, before),
                                       ("heal_pair", c.heal_pair_batch_host_ptr, healed)):
                    got, gbad = _host_pair_call(fn, m, *args, ctx + (call,))
                    label = "rs_%s_kernel<K=10,MT=4>%s" % (call, ",UA" if one_kernel else "")
                    assert label == pair_labels(k, m, form)[call == "heal_pair"]
                    assert c.last_kernel() == label, (c.last_kernel(), label) + ctx
                    assert np.array_equal(got, sht.verdicts), ctx + (call, got.tolist())
                    assert np.array_equal(gbad, sht.flags), ctx + (call,)
                    check({"d": db.a, "p": pb.a}, want, ctx + (call,))
                sflags, raws = _host_scrub_call(c, *args, ctx + ("scrub",))
                slabel = scrub_label(k, m, not one_kernel)
                assert c.last_kernel() == pair_labels(k, m, form)[2] == slabel, (c.last_kernel(), slabel) + ctx
                assert np.array_equal(sflags, sht.image_flags), ctx + (sflags.tolist(),)
                assert np.array_equal(raws, sht.raws), ctx + ("scrub", np.argwhere(raws != sht.raws)[:4].tolist())
                check({"d": db.a, "p": pb.a}, healed, ctx + ("scrub wrote to the shards",))
    finally:
        db.free()
        pb.free()


@pytest.mark.gpu
def test_host_pipeline_past_a_chunk_with_two_block_strides(gpu):
    """RS(2,3), S = 2049, pageable arrays with dbs = k*S + 24 != pbs = m*S + 40, small_call_bytes 0,
    chunk + 3 blocks (test_heal_pair.py::test_host_pipeline_pageable's sizing): the second chunk's
    rows are carried home from staging rows b - b0 to the caller's block b.  The sheet's pair damage
    in the first block, on both sides of the seam and in the last block, three of the five pairs
    across the halves: locate_pair names them and scrub flags them and both leave the arrays alone,
    heal_pair restores exactly the named rows, gaps and guards included."""
    torch, rsmi = gpu
    k, m, S = 2, 3, 2049
    n = k + m
    chunk = max(1, (64 << 20) // (n * rsmi.recommended_pitch(S)))
    nb = chunk + 3
    dside, pside = Side("d", 0, S, k * S + 24), Side("p", 0, S, m * S + 40)
    with _leg("host-seam", "2-3"):
        rng = np.random.default_rng(S + nb + 1)
        data = rng.integers(0, 256, size=(nb, k, S), dtype=np.uint8)
        parity = orc.encode_fast(k, m, data, threads=8)
        clean = blank(dside, pside, nb)

        def rows(buf, side, nrows):
            return np.lib.stride_tricks.as_strided(buf[GUARD:], shape=(nb, nrows, S), strides=(side.bs, side.rs, 1))

        rows(clean["d"], dside, k)[:] = data
        rows(clean["p"], pside, m)[:] = parity
        dirty = {a: x.copy() for a, x in clean.items()}
        hit = [0, chunk - 1, chunk, chunk + 1, nb - 1]
        pairs = [(0, k + 1), (0, 1), (1, k), (k, k + 2), (1, k + 2)]
        assert sorted(set(hit)) == hit and hit[-1] >= chunk
        for b, (x, y) in zip(hit, pairs):
            sh = np.concatenate([data[b], parity[b]])[None].copy()
            damage_pair(sh, 0, x, y)
            rows(dirty["d"], dside, k)[b] = sh[0, :k]
            rows(dirty["p"], pside, m)[b] = sh[0, k:]
        stored = np.concatenate([rows(dirty["d"], dside, k), rows(dirty["p"], pside, m)], axis=1)
        want = np.full((nb, 2), CLEAN, dtype=np.int32)
        want[hit] = want_pairs(k, m, stored[hit])
        assert want[hit].tolist() == [list(x) for x in pairs]
        full = np.concatenate([data, parity], axis=1)
        assert np.array_equal(want_image(k, m, stored[hit], want[hit]), full[hit])
        near = sorted({b for x in hit for b in (x - 1, x, x + 1) if 0 <= b < nb})   # the oracle's own encode there
        assert not want_flags(k, m, full[near]).any()
        flags = np.zeros((nb, m), dtype=bool)
        flags[hit] = want_flags(k, m, stored[hit])
        assert flags[hit].any(axis=1).all()
        work = {a: x.copy() for a, x in dirty.items()}
        args = (work["d"].ctypes.data + GUARD, dside.bs, work["p"].ctypes.data + GUARD, pside.bs, S, nb)
        with rsmi.Codec(k, m) as c:
            c.set_option("small_call_bytes", 0)
            for call, fn in (("locate_pair", c.locate_pair_batch_host_ptr), ("scrub", None),
                             ("heal_pair", c.heal_pair_batch_host_ptr)):
                ctx = ("seam", call)
                if fn is None:
                    gbad, raws = _host_scrub_call(c, *args, ctx)
                    assert c.last_kernel() == scrub_label(k, m, True) == pair_labels(k, m, "aligned")[2]
                    got_e, want_e = entries_of(rsmi, raws, S), want_entries(stored)
                    assert np.array_equal(got_e, want_e), (ctx, np.argwhere(got_e != want_e)[:4].tolist())
                    assert_raws(rsmi, raws[near], stored[near], ctx)
                else:
                    got, gbad = _host_pair_call(fn, m, *args, ctx)
                    assert c.last_kernel() == pair_labels(k, m, "aligned")[call == "heal_pair"] == \
                        "rs_%s_kernel<K=2,MT=3>" % call
                    assert np.array_equal(np.flatnonzero(got[:, 0] != CLEAN), np.array(hit)), ctx
                    assert np.array_equal(got, want), ctx
                assert np.array_equal(gbad, flags), ctx
                check(work, clean if call == "heal_pair" else dirty, ctx)


# ---------------------------------------------------------------- leg 4: fuzz
def draw(seed):
    """A shape dealt from test_heal_pair_fuzz's four, a size of its SIZES, each half from
    test_scrub_fuzz.draw_half with its own alignment draw, 12 blocks with test_heal_pair_fuzz's deal
    of 0 to 3 damaged shards and its extents."""
    rng = np.random.default_rng(0x9A12 + seed)
    k, m = FUZZ_SHAPES[seed % len(FUZZ_SHAPES)]
    S = SIZES[int(rng.integers(len(SIZES)))]
    d = Side("d", *draw_half(rng, k, S, bool(rng.integers(0, 2))))
    p = Side("p", *draw_half(rng, m, S, bool(rng.integers(0, 2))))
    deal = rng.permutation(DEAL)
    sh = stripes(k, m, S, len(deal)).copy()
    for b, nd in enumerate(deal):
        for x in rng.choice(k + m, size=int(nd), replace=False):
            lo = int(rng.integers(S))
            ext = int(min(S - lo, rng.choice([1, 1, 2, 17, 1100, S])))
            sh[b, x, lo:lo + ext] ^= rng.integers(1, 256, size=ext, dtype=np.uint8)
    return k, m, S, d, p, deal, sh


Fuzz = collections.namedtuple("Fuzz", "k m S d p deal sh want image flags")
_FUZZ = {}


def fuzz_case(seed):
    """The draw of a seed and the definition's verdicts, image and flags for it, computed once
    (leg 0 computes all 16) and read-only."""
    if seed not in _FUZZ:
        k, m, S, d, p, deal, sh = draw(seed)
        want = definition(k, m, sh)
        image = want_image(k, m, sh, want)
        check_deal(k, m, S, deal, sh, want, image)
        flags = want_flags(k, m, sh)
        for a in (sh, want, image, flags):
            a.setflags(write=False)
        _FUZZ[seed] = Fuzz(k, m, S, d, p, deal, sh, want, image, flags)
    return _FUZZ[seed]


def test_fuzz_draws_cover_the_halves():
    """The 16 draws have every mix of an aligned and an unaligned half and both forms with a pair
    kernel, every half is well formed, and the definition's answers for every seed are what the
    distance promises of the deal (test_heal_pair_fuzz.check_deal)."""
    mixes, forms, named = set(), set(), 0
    for seed in range(16):
        f = fuzz_case(seed)
        k, m, S, d, p = f[:5]
        assert d.rs >= S and p.rs >= S and d.bs >= k * d.rs and p.bs >= m * p.rs
        grid = [all(x % 16 == 0 for x in (GUARD + s.off, s.rs, s.bs)) for s in (d, p)]
        mixes.add(tuple(grid))
        forms.add(expected_form(GUARD + d.off, d.rs, d.bs, GUARD + p.off, p.rs, p.bs, S))
        assert sorted(f.deal.tolist()) == DEAL
        named += int(((f.want[:, 0] < k) & (f.want[:, 1] >= k)).sum())
    assert len(mixes) == 4 and forms == {"aligned", "ua"}, (mixes, forms)
    assert named >= 16, named   # pairs that span the halves


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(16))
def test_fuzz(gpu, seed):
    """locate_pair, then heal_pair, on the drawn halves: the definition's verdicts, both
    allocations whole against the definition's image, the label from expected_form of the two
    halves as they landed on the device."""
    torch, rsmi = gpu
    k, m, S, d, p, deal, sh, want, image, flags = fuzz_case(seed)
    nb = len(deal)
    host = blank(d, p, nb)
    put(host, d, sh[:, :k])
    put(host, p, sh[:, k:])
    healed = {a: x.copy() for a, x in host.items()}
    put(healed, d, image[:, :k])
    put(healed, p, image[:, k:])
    h = torch.cuda.current_stream().cuda_stream
    with _leg("fuzz", seed), rsmi.Codec(k, m) as c:
        dev = upload(torch, host)
        form = expected_form(dptr(dev, d), d.rs, d.bs, dptr(dev, p), p.rs, p.bs, S)
        labels = pair_labels(k, m, form)
        ctx = (seed, k, m, S, d, p, form)
        for call, fn, after in (("locate_pair", c.locate_pair_batch_dev, host),
                                ("heal_pair", c.heal_pair_batch_dev, healed)):
            out, bad = _outputs(torch, m, nb)
            fn(dptr(dev, d), d.rs, d.bs, dptr(dev, p), p.rs, p.bs, S, nb, out.data_ptr(), bad.data_ptr(), h)
            torch.cuda.synchronize()
            label = labels[call == "heal_pair"]
            assert c.last_kernel() == label, (c.last_kernel(), label) + ctx
            got, gbad = _results(out.cpu().numpy(), bad.cpu().numpy(), m, True, ctx + (call,), nb)
            assert np.array_equal(got, want), ctx + (call, got.tolist(), want.tolist())
            assert np.array_equal(gbad, flags), ctx + (call,)
            check(download(dev), after, ctx + (call,))
            SEEN[call, family(label)] += 1
