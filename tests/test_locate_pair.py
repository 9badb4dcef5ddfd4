"""rsmi_locate_pair on the GPU against the definition, computed with the CPU oracle, exactly.

A pair {x, y}, x < y, explains a dirty stripe when the stripe with rows x and y replaced by the
oracle's reconstruction of them from the other rows is clean.  The expected verdict of a block is
(-1, -1) clean, (x, -1) where the definition of rsmi_locate names shard x, (x, y) where no single
shard explains the stripe and exactly one pair does, else (-2, -2); it never comes from the
library, and there are no tolerances.  Codes wider than 24 shards use a numpy span test instead,
which test_locate_pair_abi.py shows equal to the oracle form.  Every aimed case asserts on the CPU
that the definition gives what the case is meant to produce before it touches the GPU.

  1  every pair in one call: same byte, across tiles, whole stale rows; both layouts
  2  the bit positions at the word seams
  3  padding and gaps
  4  one batch of clean blocks, single culprits, pairs and three damaged shards
  5  imitation at RS(4,4): three damaged shards whose only explanation is a disjoint pair
  6  ambiguity at RS(6,3): two pairs explain one byte column
  7  m <= 2: locate's verdicts, widened
  8  shapes without an rs_locate_pair_kernel: rs_locate_pair_rows_kernel, past a scratch chunk
  9  waves_per_cu = 1, scratch regrow, more streams than scratch entries
 10  stream order, with no host sync between the steps
 11  block offsets past 4 GiB
 12  host paths: page-locked rows in place, one block, the small call, the upload pipeline
 13  the route to repair: pair verdicts, then the mixed-batch reconstruct
"""
import ctypes
import os

import numpy as np
import pytest

import oracle_lib as orc
from test_locate import is_clean, verify_flags, want_verdict
from test_locate import label as locate_label
from test_verify import Lay, stripes, want_flags

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TILE = 1024
CLEAN, UNKNOWN = -1, -2
POISON = 0x5EED
ROWS = "rs_locate_pair_rows_kernel"
PAIR_KS = [1, 2, 3, 4, 5, 6, 8, 10, 12, 16]


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    rsmi = pytest.importorskip("rsmi")
    if not torch.cuda.is_available() or rsmi.device_count() == 0:
        pytest.skip("no GPU")
    return torch, rsmi


# ---------------------------------------------------------------- the definition
def pair_bit(n, x, y):
    return x * n - x * (x + 1) // 2 + (y - x - 1)


def all_pairs(n):
    return [(x, y) for x in range(n) for y in range(x + 1, n)]


_GF = {}


def gf_tables():
    """MUL[a, b] and INV[a] of the oracle's field, from its own multiply."""
    if not _GF:
        mul = orc.lib().rs_oracle_gal_mul
        exp = [1]
        for _ in range(254):
            exp.append(mul(exp[-1], 2))
        assert len(set(exp)) == 255
        log = np.zeros(256, dtype=np.int64)
        log[exp] = np.arange(255)
        e = np.array(exp * 2, dtype=np.uint8)
        M = e[log[:, None] + log[None, :]]
        M[0, :] = 0
        M[:, 0] = 0
        inv = np.zeros(256, dtype=np.uint8)
        inv[1:] = e[(255 - log[1:]) % 255]
        for a, b in ((3, 7), (0x8E, 0x53), (255, 255), (1, 200)):
            assert M[a, b] == mul(a, b)
        assert all(M[a, inv[a]] == 1 for a in range(1, 256))
        _GF["mul"], _GF["inv"] = M, inv
    return _GF["mul"], _GF["inv"]


def check_matrix(k, m):
    """H = [M | I]: column x is what an error in shard x adds to the syndromes."""
    return np.concatenate([orc.build_matrix(k, m)[k:], np.eye(m, dtype=np.uint8)], axis=1)


def in_span(A, cols):
    """Every column of cols (m, D) lies in the span of the columns of A (m, r): elimination over
    GF(2^8) on [A | cols], one vector step per pivot."""
    MUL, INV = gf_tables()
    r = A.shape[1]
    aug = np.concatenate([A, cols], axis=1).astype(np.uint8)
    row = 0
    for j in range(r):
        nz = np.flatnonzero(aug[row:, j])
        if not len(nz):
            continue
        p = row + nz[0]
        aug[[row, p]] = aug[[p, row]]
        aug[row] = MUL[INV[aug[row, j]], aug[row]]
        f = aug[:, j].copy()
        f[row] = 0
        aug ^= MUL[f[:, None], aug[row][None, :]]
        row += 1
    return not aug[row:, r:].any()


def want_pair_np(k, m, sh):
    """The definition as a span test on the syndromes: clean, the one shard, the one pair, or -2."""
    n = k + m
    syn = orc.encode(k, m, np.ascontiguousarray(sh[:k])) ^ sh[k:]
    if not syn.any():
        return CLEAN, CLEAN
    H = check_matrix(k, m)
    cols = np.unique(syn[:, syn.any(axis=0)], axis=1)
    one = [x for x in range(n) if in_span(H[:, [x]], cols)]
    if len(one) == 1:
        return one[0], CLEAN
    if one:
        return UNKNOWN, UNKNOWN
    two = [p for p in all_pairs(n) if in_span(H[:, list(p)], cols)]
    return two[0] if len(two) == 1 else (UNKNOWN, UNKNOWN)


def want_pair_oracle(k, m, sh):
    """The definition through the oracle's reconstruct, for one block sh (k + m, S) as stored."""
    if is_clean(k, m, sh):
        return CLEAN, CLEAN
    v = want_verdict(k, m, sh)
    if v >= 0:
        return v, CLEAN
    n = k + m
    hits = []
    for x, y in all_pairs(n):
        rc, rec = orc.reconstruct(k, m, sh, [i not in (x, y) for i in range(n)], False)
        if rc == 0 and is_clean(k, m, rec):
            assert all(np.array_equal(rec[i], sh[i]) for i in range(n) if i not in (x, y))
            hits.append((x, y))
    return hits[0] if len(hits) == 1 else (UNKNOWN, UNKNOWN)


def want_pair(k, m, sh):
    return want_pair_np(k, m, sh) if k + m > 24 else want_pair_oracle(k, m, sh)


def want_pairs(k, m, shards):
    return np.array([want_pair(k, m, shards[b]) for b in range(shards.shape[0])], dtype=np.int32).reshape(-1, 2)


def gf_solve(A, b):
    """x with A x = b over GF(2^8), A square, by the oracle's inverse and multiply."""
    A = np.ascontiguousarray(A, dtype=np.uint8)
    n = A.shape[0]
    inv = np.zeros((n, n), dtype=np.uint8)
    assert orc.lib().rs_oracle_invert(orc.ptr(A), orc.ptr(inv), n) == 0
    mul = orc.lib().rs_oracle_gal_mul
    out = []
    for r in range(n):
        v = 0
        for c in range(n):
            v ^= mul(int(inv[r, c]), int(b[c]))
        out.append(v)
    return out


# ---------------------------------------------------------------- GPU plumbing
def pair_label(lay):
    if lay.m <= 2:
        return locate_label(lay)
    return "rs_locate_pair_kernel<K=%d,MT=%d>%s" % (lay.k, lay.m, "" if lay.aligned else ",UA")


def run_dev(torch, c, lay, host, lab, flags=True):
    """rsmi_locate_pair_batch_dev over host's bytes: (verdicts (nb, 2), flags (nb, m) as bool or
    None).  Both outputs start poisoned, the buffer must come back byte for byte, the label must
    match."""
    d = torch.from_numpy(host.copy()).cuda()
    assert d.data_ptr() % 256 == 0
    out = torch.full((2 * lay.nb + 2,), POISON, dtype=torch.int32, device="cuda")
    bad = torch.full((lay.nb * lay.m + 2,), POISON, dtype=torch.int32, device="cuda")
    base = d.data_ptr() + lay.off
    c.locate_pair_batch_dev(base, lay.rs, lay.bs, base + lay.k * lay.rs, lay.rs, lay.bs, lay.S, lay.nb,
                            out.data_ptr(), bad.data_ptr() if flags else 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert c.last_kernel() == lab, (c.last_kernel(), lab)
    assert np.array_equal(d.cpu().numpy(), host), "locate_pair wrote to the shards"
    out, bad = out.cpu().numpy(), bad.cpu().numpy()
    assert (out[2 * lay.nb:] == POISON).all() and (bad[lay.nb * lay.m:] == POISON).all(), "wrote past its outputs"
    if not flags:
        assert (bad == POISON).all()
        return out[:2 * lay.nb].reshape(-1, 2), None
    return out[:2 * lay.nb].reshape(-1, 2), bad[:lay.nb * lay.m].reshape(lay.nb, lay.m) != 0


def check(torch, c, lay, sh, lab, want, host=None):
    """Pair-locate sh (nb, n, S) laid out by lay: the verdicts are want (the definition's), the
    flags are the oracle's and Verify's own."""
    host = lay.fill(sh) if host is None else host
    got, bad = run_dev(torch, c, lay, host, lab)
    assert np.array_equal(got, want), (lay.k, lay.m, lay.S, lay.aligned, got.tolist(), np.asarray(want).tolist())
    assert np.array_equal(bad, want_flags(lay.k, lay.m, sh))
    assert np.array_equal(bad, verify_flags(torch, c, lay, host))
    return got


# ---------------------------------------------------------------- 1: every pair in one call
PLACES = ("same", "cross", "stale")
_WANT1 = {}


def pair_stripes(k, m, S, pairs, place):
    """One block per pair and a clean one.  same: x and y damaged in the same three byte columns; cross: x only
    in tile 0 and y only in tile 1 (each tile alone names a single shard); stale: both rows random."""
    rng = np.random.default_rng(1000 * k + 10 * m + len(place))
    sh = stripes(k, m, S, len(pairs) + 1).copy()
    for b, (x, y) in enumerate(pairs):
        if place == "same":  # three columns: at m = 3 one column alone is often explained by a second pair
            for i, (ex, ey) in enumerate(((0x21, 0x9C), (0x47, 0x0B), (0xD3, 0x65))):
                pos = (b * 37 + 5 + i * 400) % S
                sh[b, x, pos] ^= ex
                sh[b, y, pos] ^= ey
        elif place == "cross":
            sh[b, x, (b * 11) % TILE] ^= 1 << (b % 8)
            sh[b, y, TILE + b % (S - TILE)] ^= 0x80 >> (b % 8)
        else:
            sh[b, x] = rng.integers(0, 256, size=S, dtype=np.uint8)
            sh[b, y] = rng.integers(0, 256, size=S, dtype=np.uint8)
    return sh


def pair_case(k, m, S, pairs, place):
    """(shards, want) of pair_stripes, the definition computed once and shared by both layouts; the
    case is meant to produce every pair, which the definition must confirm on the CPU."""
    key = (k, m, S, tuple(pairs), place)
    if key not in _WANT1:
        sh = pair_stripes(k, m, S, pairs, place)
        want = want_pairs(k, m, sh)
        assert want.tolist() == [list(p) for p in pairs] + [[CLEAN, CLEAN]], (key[:3], place, want.tolist())
        _WANT1[key] = (sh, want)
    return _WANT1[key]


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
@pytest.mark.parametrize("k,m,S,place", [(k, m, S, p) for k, m, S in ((10, 4, 1041), (6, 3, 1041), (16, 4, 48))
                                         for p in PLACES if p != "cross" or S > TILE])
def test_every_pair(gpu, k, m, S, place, aligned):
    """All C(n,2) pairs of RS(10,4) (91), RS(6,3) (36) and RS(16,4) (190) in one call.  S = 1041:
    two tiles with a partial last chunk, split: an overlapping last window; S = 48 is one tile, so it
    has no cross-tile placement.  At m = 4 the distance
    guarantees the pair; at m = 3 the definition confirms it for these draws."""
    torch, rsmi = gpu
    pairs = all_pairs(k + m)
    sh, want = pair_case(k, m, S, pairs, place)
    lay = Lay(rsmi, k, m, S, len(pairs) + 1, aligned)
    with rsmi.Codec(k, m) as c:
        check(torch, c, lay, sh, pair_label(lay), want)


# ---------------------------------------------------------------- 2: bit positions
@pytest.mark.gpu
@pytest.mark.parametrize("k,m", [(10, 4), (16, 4)])
def test_bit_positions_at_word_seams(gpu, k, m):
    """The pairs whose bit index is 0, 31, 32, 63, 64 and C(n,2) - 1 (and 127, 128 where they
    exist), each beside a clean block."""
    torch, rsmi = gpu
    n, S = k + m, 1041
    idx = {pair_bit(n, x, y): (x, y) for x, y in all_pairs(n)}
    assert sorted(idx) == list(range(n * (n - 1) // 2))
    bits = [b for b in (0, 31, 32, 63, 64, 127, 128, n * (n - 1) // 2 - 1) if b in idx]
    pairs = [idx[b] for b in bits]
    assert pairs[0] == (0, 1) and pairs[-1] == (n - 2, n - 1)
    sh, want = pair_case(k, m, S, pairs, "same")
    lay = Lay(rsmi, k, m, S, len(pairs) + 1, True)
    with rsmi.Codec(k, m) as c:
        check(torch, c, lay, sh, pair_label(lay), want)


# ---------------------------------------------------------------- 3: padding and gaps
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
def test_padding_and_gaps(gpu, aligned):
    """The padding byte behind each culprit row flipped (aligned) and the gap bytes around the
    blocks changed: the verdicts do not move.  Every byte that is not a row byte is a sentinel."""
    torch, rsmi = gpu
    k, m, S = 10, 4, 1041
    pairs = [(0, 1), (3, k), (k + 1, k + 3), (9, 13)]
    sh, want = pair_case(k, m, S, pairs, "cross")
    lay = Lay(rsmi, k, m, S, len(pairs) + 1, aligned)
    host = lay.fill(sh)
    if aligned:
        assert lay.rs > S
        for b, (x, y) in enumerate(pairs):
            for r in (x, y):
                host[lay.off + b * lay.bs + r * lay.rs + S] ^= 0xFF
        host[lay.off + lay.bs - 1] ^= 0xFF  # the gap behind block 0
    else:
        host[0] ^= 0xFF
        host[lay.off + lay.nb * lay.bs] ^= 0xFF
    assert np.array_equal(lay.rows(host), sh)
    with rsmi.Codec(k, m) as c:
        check(torch, c, lay, sh, pair_label(lay), want, host=host)


# ---------------------------------------------------------------- 4: a mixed batch
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
def test_mixed_batch(gpu, aligned):
    """Clean blocks, single culprits (equal to rsmi_locate's output for the same buffer), pairs and
    a block with three damaged shards, RS(10,4), S = 4099 (5 tiles)."""
    torch, rsmi = gpu
    k, m, S, nb = 10, 4, 4099, 8
    key = ("mixed", k, m, S)
    if key not in _WANT1:
        sh = stripes(k, m, S, nb).copy()
        sh[1, 4, 4098] ^= 0x01                                   # a single data shard
        sh[2, k + 2, 100:3100] ^= 0xFF                           # a single parity shard, stale
        sh[3, 2, 17] ^= 0x40
        sh[3, 7, 3000] ^= 0x04                                   # two data shards, different tiles
        sh[4, 5, 2048] ^= 0x11
        sh[4, k, 2048] ^= 0x22                                   # data and parity 0, one byte
        sh[5, 0, 1] ^= 0x01
        sh[5, 6, 2000] ^= 0x02
        sh[5, k + 3, 4000] ^= 0x03                               # three damaged shards
        sh[7, k + 1, 5] ^= 0x80
        sh[7, k + 3, 4097] ^= 0x08                               # two parity shards
        want = want_pairs(k, m, sh)
        assert want.tolist() == [[CLEAN, CLEAN], [4, CLEAN], [k + 2, CLEAN], [2, 7], [5, k], [UNKNOWN, UNKNOWN],
                                 [CLEAN, CLEAN], [k + 1, k + 3]], want.tolist()
        _WANT1[key] = (sh, want)
    sh, want = _WANT1[key]
    lay = Lay(rsmi, k, m, S, nb, aligned)
    with rsmi.Codec(k, m) as c:
        host = lay.fill(sh)
        got = check(torch, c, lay, sh, pair_label(lay), want)
        d = torch.from_numpy(host).cuda()
        cul = torch.full((nb,), POISON, dtype=torch.int32, device="cuda")
        base = d.data_ptr() + lay.off
        c.locate_batch_dev(base, lay.rs, lay.bs, base + k * lay.rs, lay.rs, lay.bs, S, nb, cul.data_ptr(), 0,
                           torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        cul = cul.cpu().numpy()
        single = got[:, 1] == CLEAN
        assert np.array_equal(cul[single], got[single, 0]) and (cul[~single] == UNKNOWN).all()


# ---------------------------------------------------------------- 5: imitation
def imitation_rs44():
    """RS(4,4): the five columns h_0, h_2, h_5 and h_1, h_6 of H are dependent with every
    coefficient non-zero, so errors lam_0 e, lam_2 e, e in shards 0, 2, 5 of one byte column give
    a syndrome in span{h_1, h_6}."""
    k, m = 4, 4
    H = check_matrix(k, m)
    three, pair = (0, 2, 5), (1, 6)
    lam = gf_solve(H[:, [0, 2, 1, 6]], H[:, 5])
    assert all(lam)
    return k, m, three, pair, lam[:2]


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
def test_imitation_names_the_unique_pair(gpu, aligned):
    """Three damaged shards whose syndromes are those of a disjoint pair: replacing that pair
    cleans the stripe and nothing else does, so the definition says the pair, and so does the
    library.  A property of the code, pinned here."""
    torch, rsmi = gpu
    k, m, three, pair, lam = imitation_rs44()
    mul = orc.lib().rs_oracle_gal_mul
    S, nb = 1040, 3
    sh = stripes(k, m, S, nb).copy()
    for b, (e, pos) in enumerate([(0x01, 7), (0xC3, 1033)]):
        sh[b, three[0], pos] ^= mul(lam[0], e)
        sh[b, three[1], pos] ^= mul(lam[1], e)
        sh[b, three[2], pos] ^= e
    want = want_pairs(k, m, sh)
    assert not set(three) & set(pair)
    assert want.tolist() == [list(pair), list(pair), [CLEAN, CLEAN]], want.tolist()
    lay = Lay(rsmi, k, m, S, nb, aligned)
    with rsmi.Codec(k, m) as c:
        check(torch, c, lay, sh, pair_label(lay), want)


# ---------------------------------------------------------------- 6: ambiguity at m = 3
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
def test_ambiguity_at_m3(gpu, aligned):
    """RS(6,3): the planes span{h_1, h_4} and span{h_2, h_7} of the three-dimensional syndrome
    space meet in a line; errors in shards 1 and 4 of one byte column chosen on that line are
    explained by {2, 7} as well, so the verdict is (-2, -2)."""
    torch, rsmi = gpu
    k, m, S, nb = 6, 3, 1040, 3
    H = check_matrix(k, m)
    mul = orc.lib().rs_oracle_gal_mul
    lam = gf_solve(H[:, [1, 4, 2]], H[:, 7])   # h_7 = lam_1 h_1 + lam_4 h_4 + lam_2 h_2
    assert all(lam)
    sh = stripes(k, m, S, nb).copy()
    for b, (e, pos) in enumerate([(0x01, 3), (0x5D, 1039)]):
        sh[b, 1, pos] ^= mul(lam[0], e)
        sh[b, 4, pos] ^= mul(lam[1], e)
    cols = (orc.encode(k, m, np.ascontiguousarray(sh[0, :k])) ^ sh[0, k:])[:, [3]]
    assert in_span(H[:, [1, 4]], cols) and in_span(H[:, [2, 7]], cols)
    want = want_pairs(k, m, sh)
    assert want.tolist() == [[UNKNOWN, UNKNOWN], [UNKNOWN, UNKNOWN], [CLEAN, CLEAN]], want.tolist()
    lay = Lay(rsmi, k, m, S, nb, aligned)
    with rsmi.Codec(k, m) as c:
        check(torch, c, lay, sh, pair_label(lay), want)


# ---------------------------------------------------------------- 7: m <= 2
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
@pytest.mark.parametrize("k,m", [(4, 2), (2, 1)])
def test_m_le_2_names_no_pair(gpu, k, m, aligned):
    """RS(4,2) and RS(2,1) with two damaged shards, one damaged shard and a clean block: locate's
    verdicts widened, (-2, -2) for the two, and the label is locate's (no pair kernel runs)."""
    torch, rsmi = gpu
    S, nb = 1041, 4
    sh = stripes(k, m, S, nb).copy()
    sh[0, 0, 5] ^= 0x10
    sh[0, k, 1030] ^= 0x01
    sh[1, 1, 1040] ^= 0x80
    sh[3, 0, 100] ^= 0x33
    sh[3, 1, 100] ^= 0x44
    want = want_pairs(k, m, sh)
    single = [1, CLEAN] if m == 2 else [UNKNOWN, UNKNOWN]
    assert [want[0].tolist(), want[1].tolist(), want[2].tolist()] == [[UNKNOWN, UNKNOWN], single, [CLEAN, CLEAN]]
    assert want[3].tolist() == [UNKNOWN, UNKNOWN] or want[3, 1] == CLEAN  # two in one column may imitate a third
    lay = Lay(rsmi, k, m, S, nb, aligned)
    assert pair_label(lay).startswith("rs_locate_kernel" if m == 2 else "rs_verify_kernel")
    with rsmi.Codec(k, m) as c:
        check(torch, c, lay, sh, pair_label(lay), want)


# ---------------------------------------------------------------- 8: fallback shapes
def fallback_case(k, m, S, nb=6):
    key = ("fb", k, m, S)
    if key not in _WANT1:
        sh = stripes(k, m, S, nb).copy()
        sh[0, 0, S - 1] ^= 0x10
        sh[0, k - 1, 0] ^= 0x01                                   # two data shards (one at k = 1)
        sh[1, k - 1, S // 2] ^= 0x33
        sh[1, k, S // 2] ^= 0x44                                  # data and parity 0, one byte column
        sh[2, k + 1, 1] ^= 0x02
        sh[2, k + m - 1, S - 2] ^= 0x20                           # two parity shards
        sh[3, k + m - 1, S // 3] ^= 0x08                          # a single parity shard
        sh[5, 0, 2] ^= 0x01
        sh[5, k, 3] ^= 0x02
        sh[5, k + 2, 4] ^= 0x03                                   # three damaged shards
        _WANT1[key] = (sh, want_pairs(k, m, sh))
    return _WANT1[key]


@pytest.mark.gpu
@pytest.mark.parametrize("k,m,S,aligned", [(20, 4, 333, True), (7, 3, 1025, True), (5, 5, 1040, True),
                                           (5, 5, 1040, False), (10, 4, 7, False), (64, 64, 48, True)],
                         ids=["20-4", "7-3", "5-5", "5-5-split", "10-4-S7-pitch7", "64-64"])
def test_fallback_shapes(gpu, k, m, S, aligned):
    """K > 16, K without an instantiation, m > 4 (two launch tiles), unaligned rows shorter than 16
    bytes at an odd pitch, and RS(64,64) against the numpy definition (8128 pairs): pairs of every
    kind, a single culprit, a clean block and three damaged shards in one call."""
    torch, rsmi = gpu
    sh, want = fallback_case(k, m, S)
    assert want[3].tolist() == [k + m - 1, CLEAN] and want[4].tolist() == [CLEAN, CLEAN]
    if m >= 4:  # the distance promises the pairs
        assert want[:3].tolist() == [[0, k - 1], [k - 1, k], [k + 1, k + m - 1]]
    lay = Lay(rsmi, k, m, S, sh.shape[0], aligned)
    assert aligned or lay.rs == S
    assert S != 7 or (lay.rs % 2 == 1 and lay.off % 2 == 1)
    with rsmi.Codec(k, m) as c:
        check(torch, c, lay, sh, ROWS, want)


@pytest.mark.gpu
def test_fallback_past_a_scratch_chunk(gpu):
    """RS(1,4), S = 15 at pitch 15 from an odd base, 2^20 + 3 blocks (the layout of
    test_verify_matrix.py): the fallback's scratch chunk is exactly 2^20 blocks and each chunk's
    grid wraps 16 times.  Two damaged shards on each side of the grid's first wrap, of the chunk
    seam and at both ends; the pair rotates over all ten."""
    torch, rsmi = gpu
    from test_verify_matrix import SEAM_HIT, seam_stripes
    k, m = 1, 4
    lay, full, fill = seam_stripes(rsmi)
    pairs = all_pairs(k + m)
    sh = full.copy()
    want = np.full((lay.nb, 2), CLEAN, dtype=np.int32)
    for i, b in enumerate(SEAM_HIT):
        x, y = pairs[(3 * i) % len(pairs)]
        sh[b, x, (i * 7) % lay.S] ^= 1 << (i % 8)
        sh[b, y, (i * 5 + 1) % lay.S] ^= 0x80 >> (i % 8)
        want[b] = want_pair(k, m, sh[b])
        assert want[b].tolist() == [x, y], (b, want[b])
    for b in (1, 65533, 2 ** 20 - 2):
        assert want_pair(k, m, sh[b]) == (CLEAN, CLEAN)
    host = fill(sh)
    with rsmi.Codec(k, m) as c:
        got, bad = run_dev(torch, c, lay, host, ROWS)
        assert np.array_equal(np.flatnonzero(got[:, 0] != CLEAN), np.array(SEAM_HIT))
        assert np.array_equal(got, want), (got[SEAM_HIT], want[SEAM_HIT])
        assert np.array_equal(np.flatnonzero(bad.any(axis=1)), np.array(SEAM_HIT))
        assert np.array_equal(bad[SEAM_HIT], want_flags(k, m, sh[SEAM_HIT]))
        got2, none = run_dev(torch, c, lay, host, ROWS, flags=False)
        assert none is None and np.array_equal(got2, got)


# ---------------------------------------------------------------- 9: strided walk and scratch
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
def test_waves_per_cu_1(gpu, aligned):
    """RS(10,4), S = 4099 (5 tiles a block) with option waves_per_cu = 1 and more tiles than the
    capped grid has waves, so every wave strides to further tiles: the pair rotates over the
    blocks, every fifth block is clean."""
    torch, rsmi = gpu
    k, m, S = 10, 4, 4099
    n = k + m
    waves = max(1, torch.cuda.get_device_properties(0).multi_processor_count // 4) * 4
    nb = max(40, waves // 5 + 8)
    assert nb * 5 > waves
    pairs = all_pairs(n)
    sh = stripes(k, m, S, nb).copy()
    want = np.full((nb, 2), CLEAN, dtype=np.int32)
    for b in range(nb):
        if b % 5 == 4:
            continue
        x, y = pairs[(7 * b) % len(pairs)]
        sh[b, x, (b * 101) % S] ^= 0x10
        sh[b, y, S - 1 - (b * 53) % S] ^= 0x01
        want[b] = (x, y)
    for b in (0, 1, 4, nb - 2, nb - 1):  # the definition on a sample: the distance promises the rest
        assert want_pair(k, m, sh[b]) == tuple(want[b])
    lay = Lay(rsmi, k, m, S, nb, aligned)
    with rsmi.Codec(k, m) as c:
        c.set_option("waves_per_cu", 1)
        check(torch, c, lay, sh, pair_label(lay), want)


@pytest.mark.gpu
@pytest.mark.parametrize("k,m,fused", [(5, 3, True), (7, 3, False)], ids=["fused", "fallback"])
def test_scratch_regrow(gpu, k, m, fused):
    """One context, one stream: 3 blocks at S = 1025, 40 blocks at S = 65541 (the stream's scratch
    is freed and reallocated behind the first call), then 3 blocks again in the larger scratch with
    no flags pointer.  One pair per call, at a different block."""
    torch, rsmi = gpu
    with rsmi.Codec(k, m) as c:
        for S, nb, (b, x, y), with_flags in ((1025, 3, (1, 0, k + 1), True), (65541, 40, (38, 2, 3), True),
                                             (1025, 3, (2, k, k + 2), False)):
            lay = Lay(rsmi, k, m, S, nb, True)
            sh = stripes(k, m, S, nb).copy()
            sh[b, x, S - 1] ^= 0x20
            sh[b, y, 0] ^= 0x02
            want = np.full((nb, 2), CLEAN, dtype=np.int32)
            want[b] = want_pair(k, m, sh[b])
            assert want[b].tolist() == [x, y]
            got, bad = run_dev(torch, c, lay, lay.fill(sh), pair_label(lay) if fused else ROWS, flags=with_flags)
            assert np.array_equal(got, want), (S, nb, got[b])
            if with_flags:
                assert np.array_equal(bad, want_flags(k, m, sh))


@pytest.mark.gpu
def test_more_streams_than_scratch_entries(gpu):
    """One context, pair locate on 34 distinct streams in turn, each with its own pair: the 33rd
    stream makes stream_scratch() drain the device and free every stream's scratch.  Then the first
    stream once more.  34 small calls: the evict-and-reallocate path, not a stress loop."""
    torch, rsmi = gpu
    from test_locate_matrix import KEPT_STREAMS, N_STREAMS, _hip_runtime
    k, m, S, nb = 4, 3, 1025, 3
    n = k + m
    hip = _hip_runtime()
    hip.hipStreamCreateWithFlags.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
    hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
    pairs = all_pairs(n)
    assert N_STREAMS > KEPT_STREAMS + 1
    own = []
    try:
        for _ in range(N_STREAMS):
            h = ctypes.c_void_p()
            assert hip.hipStreamCreateWithFlags(ctypes.byref(h), 1) == 0
            own.append(h)
        streams = [torch.cuda.ExternalStream(h.value) for h in own]
        lay = Lay(rsmi, k, m, S, nb, True)
        full = stripes(k, m, S, nb)
        with rsmi.Codec(k, m) as c:
            for i, st in enumerate(streams + streams[:1]):
                x, y = pairs[i % len(pairs)]
                b = i % nb
                sh = full.copy()
                sh[b, x, (i * 37) % S] ^= 1 << (i % 8)
                sh[b, y, (i * 91 + 3) % S] ^= 0x80 >> (i % 8)
                want = np.full((nb, 2), CLEAN, dtype=np.int32)
                want[b] = want_pair(k, m, sh[b])
                d = torch.from_numpy(lay.fill(sh)).cuda()
                out = torch.empty(2 * nb, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                with torch.cuda.stream(st):
                    out.fill_(0x0BAD)
                    c.locate_pair_batch_dev(d.data_ptr(), lay.rs, lay.bs, d.data_ptr() + k * lay.rs, lay.rs, lay.bs, S,
                                            nb, out.data_ptr(), 0, st.cuda_stream)
                st.synchronize()
                assert c.last_kernel() == pair_label(lay)
                assert np.array_equal(out.cpu().numpy().reshape(-1, 2), want), (i, out.cpu().numpy())
    finally:
        torch.cuda.synchronize()
        for h in own:
            hip.hipStreamDestroy(h)


# ---------------------------------------------------------------- 10: stream order
@pytest.mark.gpu
@pytest.mark.parametrize("k,m", [(10, 4), (7, 3)], ids=["fast", "fallback"])
def test_stream_order(gpu, k, m):
    """Pair locate, two torch ops that damage one byte each in two shards, pair locate again into a
    second output, all on one side stream with one sync at the end: the first verdicts are clean,
    the second name the pair.  The second call passes no flags pointer.  The outputs are poisoned
    on that stream, so a memset or a kernel issued on another stream shows."""
    torch, rsmi = gpu
    S, nb = 4099, 3
    rs = rsmi.recommended_pitch(S)
    bs = (k + m) * rs
    full = stripes(k, m, S, nb)
    host = np.full(nb * bs, 0x11, dtype=np.uint8)
    rows = np.lib.stride_tricks.as_strided(host, shape=(nb, k + m, S), strides=(bs, rs, 1))
    rows[:] = full
    pinned = torch.from_numpy(host).pin_memory()
    st = torch.cuda.Stream()
    with rsmi.Codec(k, m) as c:
        for warm in (True, False):  # the first pass builds the plans and the scratch; the second is the test
            d = torch.empty(nb * bs, dtype=torch.uint8, device="cuda")
            out1 = torch.empty(2 * nb, dtype=torch.int32, device="cuda")
            out2 = torch.empty(2 * nb, dtype=torch.int32, device="cuda")
            bad1 = torch.empty(nb * m, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                h = st.cuda_stream
                d.copy_(pinned, non_blocking=True)
                out1.fill_(0x0BAD)
                out2.fill_(0x0BAD)
                bad1.fill_(0x0BAD)
                c.locate_pair_batch_dev(d.data_ptr(), rs, bs, d.data_ptr() + k * rs, rs, bs, S, nb, out1.data_ptr(),
                                        bad1.data_ptr(), h)
                d[1 * bs + 3 * rs + 1024] ^= 0x08
                d[1 * bs + (k + 1) * rs + 7] ^= 0x80
                c.locate_pair_batch_dev(d.data_ptr(), rs, bs, d.data_ptr() + k * rs, rs, bs, S, nb, out2.data_ptr(), 0, h)
            st.synchronize()
            got = d.cpu().numpy()
            grow = np.lib.stride_tricks.as_strided(got, shape=(nb, k + m, S), strides=(bs, rs, 1))
            second = [[CLEAN, CLEAN], [3, k + 1], [CLEAN, CLEAN]]
            assert want_pairs(k, m, grow).tolist() == second  # the flips ran
            assert out1.cpu().numpy().tolist() == [CLEAN] * (2 * nb), warm
            assert not bad1.cpu().numpy().any(), warm
            assert out2.cpu().numpy().reshape(-1, 2).tolist() == second, warm


# ---------------------------------------------------------------- 11: far offsets
@pytest.mark.gpu
def test_offsets_past_4gib(gpu):
    """Two blocks at block_stride = 2^32 + 256, the pair in the far block, aligned and shifted by
    one byte (the UA kernel): a row offset truncated to 32 bits would read the near block, which is
    clean."""
    torch, rsmi = gpu
    if torch.cuda.mem_get_info()[0] < 8 << 30:
        pytest.skip("needs 8 GiB of free device memory")
    k, m, S, nb = 4, 3, 1040, 2
    bs = 2 ** 32 + 256
    full = stripes(k, m, S, nb)
    try:
        with rsmi.Codec(k, m) as c:
            d = torch.empty(2 ** 32 + 2 ** 20, dtype=torch.uint8, device="cuda")
            assert 1 + bs + (k + m) * S <= d.numel()
            for off, (x, y) in ((0, (1, 2)), (0, (0, k)), (1, (3, k + 2)), (1, (k + 1, k + 2))):
                sh = full.copy()
                sh[1, x, 1033] ^= 0x10
                sh[1, y, 3] ^= 0x02
                assert want_pairs(k, m, sh).tolist() == [[CLEAN, CLEAN], [x, y]]
                for b in range(nb):
                    for i in range(k + m):
                        o = off + b * bs + i * S
                        d[o:o + S].copy_(torch.from_numpy(sh[b, i]))
                out = torch.full((2 * nb + 2,), POISON, dtype=torch.int32, device="cuda")
                base = d.data_ptr() + off
                c.locate_pair_batch_dev(base, S, bs, base + k * S, S, bs, S, nb, out.data_ptr(), 0,
                                        torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                assert c.last_kernel() == "rs_locate_pair_kernel<K=4,MT=3>" + ("" if off == 0 else ",UA")
                assert out.cpu().numpy().tolist() == [CLEAN, CLEAN, x, y, POISON, POISON]
                for b in range(nb):
                    for i in range(k + m):
                        o = off + b * bs + i * S
                        assert np.array_equal(d[o:o + S].cpu().numpy(), sh[b, i]), (off, b, i)
            del d
    finally:
        torch.cuda.empty_cache()


# ---------------------------------------------------------------- 12: host paths
def _host_pair(c, data, dbs, parity, pbs, S, nb, flags=True):
    out = np.full(2 * nb, POISON, dtype=np.int32)
    bad = np.full(nb * c.m, POISON, dtype=np.uint32)
    c.locate_pair_batch_host_ptr(data, dbs, parity, pbs, S, nb, out.ctypes.data, bad.ctypes.data if flags else 0)
    if not flags:
        assert (bad == POISON).all()
        return out.reshape(-1, 2), None
    return out.reshape(-1, 2), bad.reshape(nb, c.m) != 0


@pytest.mark.gpu
def test_host_page_locked_in_place(gpu):
    """Data and parity in one rsmi_host_alloc allocation, zero_copy 1: the kernels read them in
    place over PCIe at pitch S, the unaligned-window form."""
    torch, rsmi = gpu
    k, m, S, nb = 4, 3, 2049, 5
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
            for damage in (None, ((3, 2, 2048), (3, k + 1, 0)), ((4, 0, 5), (4, 1, 1030))):
                rows[:] = full
                for spot in damage or ():
                    rows[spot] ^= 0x20
                want = want_pairs(k, m, rows)
                assert (want[:, 1] >= 0).sum() == (damage is not None)
                before = buf.copy()
                got, bad = _host_pair(c, p, bs, p + k * S, bs, S, nb, flags=damage is not None)
                assert c.last_kernel() == "rs_locate_pair_kernel<K=4,MT=3>,UA"
                assert np.array_equal(buf, before)
                assert np.array_equal(got, want), (damage, got)
                if bad is not None:
                    assert np.array_equal(bad, want_flags(k, m, rows))
    finally:
        L.rsmi_host_free(p)


@pytest.mark.gpu
def test_small_call_and_one_block(gpu):
    """A small pageable batch and rsmi_locate_pair of one pageable block go through the page-locked
    staging; Erasure.locate_pair on the golden RS(10,4) vectors, clean and with two shards swapped
    (two damaged shards: at m = 4 the swap is named)."""
    torch, rsmi = gpu
    k, m, S, nb = 10, 4, 4099, 3
    full = stripes(k, m, S)
    assert nb * (k + m) * S * 2 <= (2 << 20)
    with rsmi.Codec(k, m) as c:
        sh = full.copy()
        sh[1, k + 2, 4098] ^= 0x02
        sh[1, 4, 0] ^= 0x02
        sh[2, 0, 0] ^= 0x80
        data, par = np.ascontiguousarray(sh[:, :k]), np.ascontiguousarray(sh[:, k:])
        got, bad = _host_pair(c, data.ctypes.data, k * S, par.ctypes.data, m * S, S, nb)
        assert c.last_kernel() == "rs_locate_pair_kernel<K=10,MT=4>,UA"
        assert got.tolist() == want_pairs(k, m, sh).tolist() == [[CLEAN, CLEAN], [4, k + 2], [0, CLEAN]]
        assert np.array_equal(bad, want_flags(k, m, sh))
        assert np.array_equal(data, sh[:, :k]) and np.array_equal(par, sh[:, k:])
        one = bytearray(full[0].tobytes())
        assert c.locate_pair(one, S) == (CLEAN, CLEAN)
        one[5 * S + 17] ^= 0x01
        assert c.locate_pair(one, S) == (5, CLEAN)
        one[(k + 3) * S + S - 1] ^= 0x01
        assert c.locate_pair(one, S) == (5, k + 3) == want_pair(k, m, np.frombuffer(bytes(one), dtype=np.uint8).reshape(k + m, S))
    z = np.load(os.path.join(GOLDEN, "vectors_k10_m4.npz"))
    shards = [bytes(r.tobytes()) for r in z["shards_4099"]]
    e = rsmi.NewErasure(10, 4, 4099)
    assert e.locate_pair(shards) == (CLEAN, CLEAN)
    sw = list(shards)
    sw[3], sw[12] = sw[12], sw[3]
    assert want_pair(10, 4, np.stack([np.frombuffer(s, dtype=np.uint8) for s in sw])) == (3, 12)
    assert e.locate_pair(sw) == (3, 12)
    e._codec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("S,past_chunk", [(2048, False), (2049, False), (2049, True)],
                         ids=["2d-copy", "odd", "odd-past-64MiB"])
def test_host_pipeline_pageable(gpu, S, past_chunk):
    """RS(2,3), pageable buffers, small_call_bytes 0: the upload pipeline, with 2D copies and with
    linear copies and the repitch kernel (odd S); the last case has more blocks than one 64 MiB
    chunk holds, with pairs on both sides of the seam."""
    torch, rsmi = gpu
    k, m = 2, 3
    chunk = max(1, (64 << 20) // (5 * rsmi.recommended_pitch(S)))
    nb = chunk + 3 if past_chunk else 9
    rng = np.random.default_rng(S + nb)
    data = rng.integers(0, 256, size=(nb, k, S), dtype=np.uint8)
    parity = orc.encode_fast(k, m, data, threads=8)
    hit = sorted({0, nb - 1, chunk - 1, chunk, chunk + 1} if past_chunk else {0, 4, nb - 1})
    pairs = all_pairs(k + m)
    want = np.full((nb, 2), CLEAN, dtype=np.int32)
    for i, b in enumerate(hit):
        x, y = pairs[(3 * i + 1) % len(pairs)]
        for r, pos in ((x, (i * 211) % S), (y, (i * 17 + 1) % S)):
            (data if r < k else parity)[b, r % k if r < k else r - k, pos] ^= 1 << (i % 8)
        want[b] = want_pair(k, m, np.concatenate([data[b], parity[b]]))
        assert want[b].tolist() in ([x, y], [UNKNOWN, UNKNOWN])  # m = 3: the definition decides
    assert (want[hit, 1] >= 0).any()
    with rsmi.Codec(k, m) as c:
        c.set_option("small_call_bytes", 0)
        d0, p0 = data.copy(), parity.copy()
        got, bad = _host_pair(c, data.ctypes.data, k * S, parity.ctypes.data, m * S, S, nb)
        assert c.last_kernel() == "rs_locate_pair_kernel<K=2,MT=3>"
        assert np.array_equal(data, d0) and np.array_equal(parity, p0)
        assert np.array_equal(np.flatnonzero(got[:, 0] != CLEAN), np.array(hit))
        assert np.array_equal(got, want)
        assert np.array_equal(np.flatnonzero(bad.any(axis=1)), np.array(hit))
        got, bad = _host_pair(c, data.ctypes.data, k * S, parity.ctypes.data, m * S, S, nb, flags=False)
        assert np.array_equal(got, want)


# ---------------------------------------------------------------- 13: the route to repair
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
def test_pair_then_mixed_reconstruct(gpu, aligned):
    """Pair verdicts read back, present and required masks built from them (a single culprit and a
    pair alike), one rsmi_reconstruct_mixed_batch_dev: every buffer equals the undamaged original
    and Verify is clean."""
    torch, rsmi = gpu
    k, m, S, nb = 10, 4, 4099, 6
    n = k + m
    full = stripes(k, m, S, nb)
    sh = full.copy()
    sh[0, 2, 100:3100] ^= 0xFF
    sh[0, 9, :] ^= 0x5A                                           # two stale data rows
    sh[1, 5, 4098] ^= 0x01                                        # a single culprit
    sh[3, 0, 0] ^= 0x80
    sh[3, k + 3, 2000:2100] ^= 0x33                               # data and parity
    sh[4, k, 1024] ^= 0x04
    sh[4, k + 1, 1023] ^= 0x40                                    # two parity rows
    want = [[2, 9], [5, CLEAN], [CLEAN, CLEAN], [0, k + 3], [k, k + 1], [CLEAN, CLEAN]]
    assert want_pairs(k, m, sh).tolist() == want
    lay = Lay(rsmi, k, m, S, nb, aligned)
    host = lay.fill(sh)
    with rsmi.Codec(k, m) as c:
        got, _ = run_dev(torch, c, lay, host, pair_label(lay))
        assert got.tolist() == want
        present = np.ones((nb, n), dtype=np.uint8)
        for b in range(nb):
            for x in got[b]:
                if x >= 0:
                    present[b, x] = 0
        required = (1 - present).astype(np.uint8)
        d = torch.from_numpy(host).cuda()
        base = d.data_ptr() + lay.off
        status = np.full(nb, POISON, dtype=np.int32)
        rc = rsmi.lib().rsmi_reconstruct_mixed_batch_dev(c._h, base, lay.rs, lay.bs, S, nb, present.ctypes.data,
                                                         required.ctypes.data, 0, status.ctypes.data,
                                                         torch.cuda.current_stream().cuda_stream)
        assert rc == 0 and (status == 0).all(), (rc, status)
        torch.cuda.synchronize()
        after = d.cpu().numpy()
        assert np.array_equal(after, lay.fill(full))
        assert not verify_flags(torch, c, lay, after).any()
