"""rsmi_locate on the GPU against the definition, computed with the CPU oracle, exactly.

A stripe is clean when every parity row is the oracle's encode of the data rows.  Shard x explains
a dirty stripe when the stripe with row x replaced by the oracle's reconstruction of it from the
other rows is clean.  The expected verdict is -1 (clean), x (exactly one shard explains) or -2; it
never comes from the library, and there are no tolerances.  The cases are a few MB each.

  1  clean stripes with every padding byte a sentinel, damage in padding and gaps, both layouts
  2  every shard as the culprit in one call, one flipped byte at the chunk and tile edges
  3  a stale shard: a whole row replaced (the AND across the tiles of a block)
  4  two damaged shards that disagree across tiles, lanes, bytes, and in one byte column: -2
  5  aliasing: two damaged shards that imitate a third one; the verdict is the third
  6  m = 1: dirty is -2, the launch is Verify's
  7  shapes without an rs_locate_kernel: Verify's flags, encode into scratch, rs_locate_rows_kernel
  8  waves_per_cu = 1: the grid-stride loop
  9  stream order, with no host sync between the steps; no flags pointer
 10  host paths: page-locked rows in place, the small call, the upload pipeline, Erasure.locate
 11  round trip: locate, rebuild the culprit, verify clean, bytes restored
 12  no side effects on the encode, reconstruct and verify of the same context
"""
import ctypes
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_lib as orc
from test_verify import Lay, stripes, want_flags

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TILE = 1024                    # 64 lanes x 16 bytes
CLEAN, UNKNOWN = -1, -2
ROWS = "rs_locate_rows_kernel"


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    rsmi = pytest.importorskip("rsmi")
    if not torch.cuda.is_available() or rsmi.device_count() == 0:
        pytest.skip("no GPU")
    assert (rsmi.LocateClean, rsmi.LocateUnknown) == (CLEAN, UNKNOWN)
    return torch, rsmi


def is_clean(k, m, sh):
    return np.array_equal(orc.encode(k, m, np.ascontiguousarray(sh[:k])), sh[k:])


def want_verdict(k, m, sh):
    """The definition for one block, sh (k + m, S) as stored.  Every oracle call builds the code's
    matrix anew, which dominates at k + m = 256, so wide codes try their shards on a few threads."""
    if is_clean(k, m, sh):
        return CLEAN
    n = k + m

    def explains(x):
        rc, rec = orc.reconstruct(k, m, sh, [i != x for i in range(n)], False)
        assert rc == 0
        assert all(np.array_equal(rec[i], sh[i]) for i in range(n) if i != x)
        return is_clean(k, m, rec)

    if n > 64:
        with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
            found = [x for x, e in enumerate(ex.map(explains, range(n))) if e]
    else:
        found = [x for x in range(n) if explains(x)]
    return found[0] if len(found) == 1 else UNKNOWN


def want_verdicts(k, m, shards):
    return np.array([want_verdict(k, m, shards[b]) for b in range(shards.shape[0])], dtype=np.int32)


def label(lay):
    if lay.m == 1:
        return "rs_verify_kernel<K=%d,MT=1>%s" % (lay.k, "" if lay.aligned else ",UA")
    return "rs_locate_kernel<K=%d,MT=%d>%s" % (lay.k, lay.m, "" if lay.aligned else ",UA")


def run_dev(torch, c, lay, host, lab, flags=True):
    """rsmi_locate_batch_dev over host's bytes: (verdicts (nb,), flags (nb, m) as bool or None).
    Both outputs start poisoned, the buffer must come back byte for byte, the label must match."""
    d = torch.from_numpy(host.copy()).cuda()
    assert d.data_ptr() % 256 == 0
    cul = torch.full((lay.nb + 2,), 0x5EED, dtype=torch.int32, device="cuda")
    bad = torch.full((lay.nb * lay.m + 2,), 0x5EED, dtype=torch.int32, device="cuda")
    base = d.data_ptr() + lay.off
    c.locate_batch_dev(base, lay.rs, lay.bs, base + lay.k * lay.rs, lay.rs, lay.bs, lay.S, lay.nb, cul.data_ptr(),
                       bad.data_ptr() if flags else 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert c.last_kernel() == lab, (c.last_kernel(), lab)
    assert np.array_equal(d.cpu().numpy(), host), "locate wrote to the shards"
    cul, bad = cul.cpu().numpy(), bad.cpu().numpy()
    assert (cul[lay.nb:] == 0x5EED).all() and (bad[lay.nb * lay.m:] == 0x5EED).all(), "wrote past its outputs"
    if not flags:
        assert (bad == 0x5EED).all()
        return cul[:lay.nb], None
    return cul[:lay.nb], bad[:lay.nb * lay.m].reshape(lay.nb, lay.m) != 0


def verify_flags(torch, c, lay, host):
    d = torch.from_numpy(host.copy()).cuda()
    bad = torch.full((lay.nb * lay.m,), 0x5EED, dtype=torch.int32, device="cuda")
    base = d.data_ptr() + lay.off
    c.verify_batch_dev(base, lay.rs, lay.bs, base + lay.k * lay.rs, lay.rs, lay.bs, lay.S, lay.nb, bad.data_ptr(),
                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return bad.cpu().numpy().reshape(lay.nb, lay.m) != 0


def check(torch, c, lay, sh, lab, want=None):
    """Locate sh (nb, n, S) laid out by lay: the verdicts are the definition's (or want, where the
    caller has them already) and the flags are the oracle's."""
    if want is None:
        want = want_verdicts(lay.k, lay.m, sh)
    got, bad = run_dev(torch, c, lay, lay.fill(sh), lab)
    assert np.array_equal(got, want), (lay.k, lay.m, lay.S, lay.aligned, got, want)
    assert np.array_equal(bad, want_flags(lay.k, lay.m, sh))
    return got


# ---------------------------------------------------------------- 1: clean stripes, the padding trap
SIZES_1 = [16, 17, 31, 1008, 1024, 1025, 1040, 4099]


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
@pytest.mark.parametrize("k,m", [(2, 1), (2, 2), (4, 2), (10, 4), (16, 4)])
def test_clean_stripes_and_padding(gpu, k, m, aligned):
    torch, rsmi = gpu
    nb = 3
    with rsmi.Codec(k, m) as c:
        for S in SIZES_1:
            lay = Lay(rsmi, k, m, S, nb, aligned)
            full = stripes(k, m, S)
            assert all(is_clean(k, m, full[b]) for b in range(nb))
            host = lay.fill(full)
            got, bad = run_dev(torch, c, lay, host, label(lay))
            assert (got == CLEAN).all() and not bad.any(), (k, m, S, aligned, got, bad)
            # damage where no row byte is: the gap after a block and, aligned, the padding of a
            # data row and of a parity row at offset S
            spots = [lay.off + 1 * lay.bs + (k + m) * lay.rs] if aligned else [0, lay.off + nb * lay.bs]
            if aligned and lay.rs > S:
                spots += [lay.off + 1 * lay.bs + r * lay.rs + S for r in (0, k, k + m - 1)]
            for o in spots:
                h2 = host.copy()
                h2[o] ^= 0xFF
                assert np.array_equal(lay.rows(h2), full)
                got, bad = run_dev(torch, c, lay, h2, label(lay))
                assert (got == CLEAN).all() and not bad.any(), (k, m, S, aligned, o, got)


# ---------------------------------------------------------------- 2: every shard as the culprit
def culprit_stripes(k, m, S, pos, nb=None, flip=0x40):
    """nb (default n + 1) blocks: block i has byte pos of shard i % n flipped, the last is clean."""
    n = k + m
    nb = nb or n + 1
    sh = stripes(k, m, S, nb).copy()
    for i in range(nb - 1):
        sh[i, i % n, pos] ^= flip
    return sh


_WANT2 = {}


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
@pytest.mark.parametrize("S", [1025, 1040])
@pytest.mark.parametrize("k,m", [(4, 2), (10, 4), (16, 4)])
def test_every_shard_as_culprit(gpu, k, m, S, aligned):
    torch, rsmi = gpu
    n = k + m
    lay = Lay(rsmi, k, m, S, n + 1, aligned)
    with rsmi.Codec(k, m) as c:
        for pos in sorted({0, 15, 16, 1007, 1008, 1023, 1024, S - 1}):
            sh = culprit_stripes(k, m, S, pos)
            if (k, m, S, pos) not in _WANT2:
                _WANT2[k, m, S, pos] = want_verdicts(k, m, sh)
            want = _WANT2[k, m, S, pos]
            assert np.array_equal(want, np.array(list(range(n)) + [CLEAN])), want  # what the distance promises
            host = lay.fill(sh)
            got, bad = run_dev(torch, c, lay, host, label(lay))
            assert np.array_equal(got, want), (pos, got)  # block i names shard i: no neighbour leaks
            assert np.array_equal(bad, verify_flags(torch, c, lay, host)), pos
            assert np.array_equal(bad, want_flags(k, m, sh)), pos


# ---------------------------------------------------------------- 3: a stale shard
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
@pytest.mark.parametrize("k,m", [(10, 4), (4, 2)])
def test_stale_shard(gpu, k, m, aligned):
    """A whole row of random bytes, S = 4099 (5 tiles): every tile of the block is dirty and every
    one of them must name the same shard; a data row and a parity row, in different blocks."""
    torch, rsmi = gpu
    S, nb = 4099, 3
    lay = Lay(rsmi, k, m, S, nb, aligned)
    rng = np.random.default_rng(33)
    sh = stripes(k, m, S).copy()
    sh[0, k - 2] = rng.integers(0, 256, size=S, dtype=np.uint8)
    sh[2, k + m - 1] = rng.integers(0, 256, size=S, dtype=np.uint8)
    with rsmi.Codec(k, m) as c:
        got = check(torch, c, lay, sh, label(lay))
        assert got.tolist() == [k - 2, CLEAN, k + m - 1]


# ---------------------------------------------------------------- 4: two damaged shards
PLACES_4 = {"tiles": (100, 3000), "lanes": (100, 500), "bytes": (160, 165), "column": (777, 777)}


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
@pytest.mark.parametrize("place", sorted(PLACES_4))
def test_two_damaged_shards(gpu, place, aligned):
    """RS(10,4), m >= 2 * 2: two damaged shards are always -2.  The two sit in different tiles of
    the block (each tile alone names one shard), in different lanes of one tile, in different bytes
    of one lane's chunk, and in one byte column; block 0 holds two data shards, block 1 a data
    and a parity shard, block 2 two parity shards."""
    torch, rsmi = gpu
    k, m, S, nb = 10, 4, 4099, 4
    p0, p1 = PLACES_4[place]
    assert (p0 // TILE != p1 // TILE) == (place == "tiles")
    assert (p0 // 16 != p1 // 16) == (place in ("tiles", "lanes"))
    lay = Lay(rsmi, k, m, S, nb, aligned)
    sh = stripes(k, m, S, nb).copy()
    for b, (x0, x1) in enumerate([(2, 7), (3, k + 1), (k, k + 3)]):
        sh[b, x0, p0] ^= 0x21
        sh[b, x1, p1] ^= 0x9C
    with rsmi.Codec(k, m) as c:
        got = check(torch, c, lay, sh, label(lay))
        assert got.tolist() == [UNKNOWN, UNKNOWN, UNKNOWN, CLEAN]


# ---------------------------------------------------------------- 5: aliasing
def gf_solve2(a, b):
    """x with a x = b over GF(2^8), a 2 x 2, by the oracle's inverse and multiply."""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    inv = np.zeros((2, 2), dtype=np.uint8)
    assert orc.lib().rs_oracle_invert(orc.ptr(a), orc.ptr(inv), 2) == 0
    mul = orc.lib().rs_oracle_gal_mul
    return [mul(int(inv[r, 0]), int(b[0])) ^ mul(int(inv[r, 1]), int(b[1])) for r in range(2)]


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
def test_aliasing_names_the_unique_explanation(gpu, aligned):
    """RS(4,2), distance 3: errors e0, e1 in shards 0 and 1 of one byte column, chosen so that the
    syndromes are those of an error e in shard 2 alone (e0 M[:,0] + e1 M[:,1] = e M[:,2] over the
    two parity rows).  Replacing shard 2 then cleans the stripe and no other shard does, so the
    definition says 2, and so does the library.  A property of the code, pinned here."""
    torch, rsmi = gpu
    k, m, S, nb = 4, 2, 1040, 3
    P = orc.build_matrix(k, m)[k:]
    mul = orc.lib().rs_oracle_gal_mul
    lay = Lay(rsmi, k, m, S, nb, aligned)
    sh = stripes(k, m, S).copy()
    for b, (e, pos) in enumerate([(0x01, 5), (0xB7, 1029)]):
        e0, e1 = gf_solve2(P[:, :2], [mul(e, int(P[0, 2])), mul(e, int(P[1, 2]))])
        assert e0 and e1
        sh[b, 0, pos] ^= e0
        sh[b, 1, pos] ^= e1
    with rsmi.Codec(k, m) as c:
        got = check(torch, c, lay, sh, label(lay))
        assert got.tolist() == [2, 2, CLEAN]


# ---------------------------------------------------------------- 6: m = 1
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
def test_single_parity_is_unknown(gpu, aligned):
    """RS(2,1): every shard explains any damage, so a dirty stripe is -2 whichever shard it is in;
    the launch is Verify's own, followed by the verdict kernel."""
    torch, rsmi = gpu
    k, m, S, nb = 2, 1, 1025, 4
    lay = Lay(rsmi, k, m, S, nb, aligned)
    assert label(lay).startswith("rs_verify_kernel<K=2,MT=1>")
    sh = stripes(k, m, S, nb).copy()
    sh[0, 0, 1024] ^= 0x01
    sh[1, 2, 0] ^= 0x80
    sh[3, 1, 512] ^= 0x10
    with rsmi.Codec(k, m) as c:
        got = check(torch, c, lay, sh, label(lay))
        assert got.tolist() == [UNKNOWN, UNKNOWN, CLEAN, UNKNOWN]


# ---------------------------------------------------------------- 7: fallback shapes
@pytest.mark.gpu
@pytest.mark.parametrize("k,m,S,aligned", [(17, 3, 333, True), (5, 5, 1040, True), (5, 5, 1040, False),
                                           (10, 6, 1025, True), (7, 2, 1025, True), (4, 2, 5, False)],
                         ids=["17-3", "5-5", "5-5-split", "10-6", "7-2", "4-2-S5-pitch5"])
def test_fallback_shapes(gpu, k, m, S, aligned):
    """K > 16, m > 4 (two launch tiles), K without an instantiation, and unaligned rows shorter
    than 16 bytes: a data culprit, a parity culprit (the last row, across the tile seam), two
    damaged shards and a clean block in one call."""
    torch, rsmi = gpu
    nb = 5
    lay = Lay(rsmi, k, m, S, nb, aligned)
    assert aligned or lay.rs == S
    sh = stripes(k, m, S, nb).copy()
    sh[0, k - 1, S - 1] ^= 0x10
    sh[1, k + m - 1, 0] ^= 0x01
    sh[2, 0, S // 2] ^= 0x33
    sh[2, k, S // 2] ^= 0x44
    sh[4, 1] = np.random.default_rng(5).integers(0, 256, size=S, dtype=np.uint8)  # stale
    with rsmi.Codec(k, m) as c:
        got = check(torch, c, lay, sh, ROWS).tolist()
        assert got[:2] + got[3:] == [k - 1, k + m - 1, CLEAN, 1]
        assert m < 4 or got[2] == UNKNOWN  # m < 2 * 2: the definition alone decides (test 5)
        assert (check(torch, c, lay, stripes(k, m, S, nb), ROWS) == CLEAN).all()


@pytest.mark.gpu
@pytest.mark.parametrize("x", [31, 32, 255])
def test_fallback_mask_word_seams(gpu, x):
    """RS(200,56), S = 48: 256 candidates in 8 words; culprits 31 and 32 (a word seam) and 255 (the
    last bit of the last word, a parity shard), each beside a clean block.  The definition costs
    256 reconstructs of a 200 x 200 code per dirty block: the slowest cases here, seconds each."""
    torch, rsmi = gpu
    k, m, S, nb = 200, 56, 48, 2
    lay = Lay(rsmi, k, m, S, nb, True)
    sh = stripes(k, m, S, nb).copy()
    sh[1, x, x % S] ^= 0x5A
    with rsmi.Codec(k, m) as c:
        assert check(torch, c, lay, sh, ROWS).tolist() == [CLEAN, x]


# ---------------------------------------------------------------- 8: waves_per_cu = 1
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
@pytest.mark.parametrize("many", [False, True], ids=["40-blocks", "past-the-grid"])
def test_waves_per_cu_1(gpu, many, aligned):
    """Case 2 at RS(10,4), S = 4099 (5 tiles a block) with option waves_per_cu = 1: 40 blocks, and
    as many blocks as it takes for more tiles than the capped grid has waves (num_cu / 4
    workgroups of 4 waves), so that every wave strides to a second tile."""
    torch, rsmi = gpu
    k, m, S = 10, 4, 4099
    n, tpb = k + m, 5
    waves = max(1, torch.cuda.get_device_properties(0).multi_processor_count // 4) * 4
    nb = max(40, waves // tpb + 8) if many else 40
    assert not many or nb * tpb > waves
    lay = Lay(rsmi, k, m, S, nb, aligned)
    sh = culprit_stripes(k, m, S, 4098, nb)
    want = np.array([i % n for i in range(nb - 1)] + [CLEAN], dtype=np.int32)
    for b in (0, n - 1, nb - 2, nb - 1):  # the definition on a sample; the rest by the flags below
        assert want_verdict(k, m, sh[b]) == want[b]
    with rsmi.Codec(k, m) as c:
        c.set_option("waves_per_cu", 1)
        check(torch, c, lay, sh, label(lay), want)
        assert (check(torch, c, lay, stripes(k, m, S, nb), label(lay), np.full(nb, CLEAN, dtype=np.int32)) == CLEAN).all()


# ---------------------------------------------------------------- 9: stream order
@pytest.mark.gpu
@pytest.mark.parametrize("k,m", [(10, 4), (7, 2)], ids=["fast", "fallback"])
def test_stream_order(gpu, k, m):
    """locate, a torch op that damages one data byte, locate again into a second output, all on
    one side stream with one sync at the end: the first verdicts are all -1, the second name the
    shard.  The second call passes no flags pointer.  The outputs start poisoned on that stream,
    so a memset or a kernel issued on another stream shows."""
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
            cul1 = torch.empty(nb, dtype=torch.int32, device="cuda")
            cul2 = torch.empty(nb, dtype=torch.int32, device="cuda")
            bad1 = torch.empty(nb * m, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                h = st.cuda_stream
                d.copy_(pinned, non_blocking=True)
                cul1.fill_(0x0BAD)
                cul2.fill_(0x0BAD)
                bad1.fill_(0x0BAD)
                c.locate_batch_dev(d.data_ptr(), rs, bs, d.data_ptr() + k * rs, rs, bs, S, nb, cul1.data_ptr(),
                                   bad1.data_ptr(), h)
                d[1 * bs + 3 * rs + 1024] ^= 0x08
                c.locate_batch_dev(d.data_ptr(), rs, bs, d.data_ptr() + k * rs, rs, bs, S, nb, cul2.data_ptr(), 0, h)
            st.synchronize()
            got = d.cpu().numpy()
            grow = np.lib.stride_tricks.as_strided(got, shape=(nb, k + m, S), strides=(bs, rs, 1))
            assert want_verdicts(k, m, grow).tolist() == [CLEAN, 3, CLEAN]  # the flip ran
            assert cul1.cpu().numpy().tolist() == [CLEAN] * nb, warm
            assert not bad1.cpu().numpy().any(), warm
            assert cul2.cpu().numpy().tolist() == [CLEAN, 3, CLEAN], warm


# ---------------------------------------------------------------- 10: host paths
def _host_locate(c, data, dbs, parity, pbs, S, nb, flags=True):
    cul = np.full(nb, 0x5EED, dtype=np.int32)
    bad = np.full(nb * c.m, 0x5EED, dtype=np.uint32)
    c.locate_batch_host_ptr(data, dbs, parity, pbs, S, nb, cul.ctypes.data, bad.ctypes.data if flags else 0)
    if not flags:
        assert (bad == 0x5EED).all()
        return cul, None
    return cul, bad.reshape(nb, c.m) != 0


@pytest.mark.gpu
def test_host_page_locked_in_place(gpu):
    """Data and parity in one rsmi_host_alloc allocation, zero_copy 1: one kernel reads them in
    place over PCIe at pitch S, the unaligned-window form."""
    torch, rsmi = gpu
    k, m, S, nb = 4, 2, 2049, 5
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
            for damage in (None, (3, 2, 2048), (4, k + 1, 0)):
                rows[:] = full
                if damage:
                    rows[damage] ^= 0x20
                want = want_verdicts(k, m, rows)
                assert (want != CLEAN).any() == (damage is not None)
                before = buf.copy()
                got, bad = _host_locate(c, p, bs, p + k * S, bs, S, nb, flags=damage is not None)
                assert c.last_kernel() == "rs_locate_kernel<K=4,MT=2>,UA"
                assert np.array_equal(buf, before)
                assert np.array_equal(got, want), (damage, got)
                if bad is not None:
                    assert np.array_equal(bad, want_flags(k, m, rows))
    finally:
        L.rsmi_host_free(p)


@pytest.mark.gpu
def test_small_call_and_one_block(gpu):
    """A small pageable batch and rsmi_locate of one pageable block go through the page-locked
    staging; Erasure.locate on the golden RS(10,4) vectors, clean and with two shards swapped."""
    torch, rsmi = gpu
    k, m, S, nb = 10, 4, 4099, 3
    full = stripes(k, m, S)
    assert nb * (k + m) * S * 2 <= (2 << 20)
    with rsmi.Codec(k, m) as c:
        sh = full.copy()
        sh[1, k + 2, 4098] ^= 0x02
        sh[2, 0, 0] ^= 0x80
        data, par = np.ascontiguousarray(sh[:, :k]), np.ascontiguousarray(sh[:, k:])
        got, bad = _host_locate(c, data.ctypes.data, k * S, par.ctypes.data, m * S, S, nb)
        assert c.last_kernel() == "rs_locate_kernel<K=10,MT=4>,UA"
        assert got.tolist() == want_verdicts(k, m, sh).tolist() == [CLEAN, k + 2, 0]
        assert np.array_equal(bad, want_flags(k, m, sh))
        assert np.array_equal(data, sh[:, :k]) and np.array_equal(par, sh[:, k:])
        one = bytearray(full[0].tobytes())
        assert c.locate(one, S) == CLEAN
        one[5 * S + 17] ^= 0x01
        assert c.locate(one, S) == 5
        one[(k + 3) * S + S - 1] ^= 0x01
        assert c.locate(one, S) == UNKNOWN  # two damaged shards, m >= 4
        one[5 * S + 17] ^= 0x01
        assert c.locate(one, S) == k + 3
    z = np.load(os.path.join(GOLDEN, "vectors_k10_m4.npz"))
    shards = [bytes(r.tobytes()) for r in z["shards_4099"]]
    e = rsmi.NewErasure(10, 4, 4099)
    assert e.locate(shards) == CLEAN
    stale = list(shards)
    stale[12] = bytes(len(shards[12]))
    assert e.locate(stale) == 12 == want_verdict(10, 4, np.stack([np.frombuffer(s, dtype=np.uint8) for s in stale]))
    sw = list(shards)
    sw[3], sw[12] = sw[12], sw[3]
    assert e.locate(sw) == UNKNOWN
    e._codec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("S,past_chunk", [(2048, False), (2049, False), (2049, True)],
                         ids=["2d-copy", "odd", "odd-past-64MiB"])
def test_host_pipeline_pageable(gpu, S, past_chunk):
    """RS(2,2), pageable buffers, small_call_bytes 0: the upload pipeline, with 2D copies (S a
    multiple of 8) and with linear copies and the repitch kernel (odd S); the last case has more
    blocks than one 64 MiB chunk holds, with culprits on both sides of the seam."""
    torch, rsmi = gpu
    k, m = 2, 2
    chunk = max(1, (64 << 20) // (4 * rsmi.recommended_pitch(S)))
    nb = chunk + 3 if past_chunk else 9
    rng = np.random.default_rng(S + nb)
    data = rng.integers(0, 256, size=(nb, k, S), dtype=np.uint8)
    parity = orc.encode_fast(k, m, data, threads=8)
    hit = sorted({0, nb - 1, chunk - 1, chunk, chunk + 1} if past_chunk else {0, 4, nb - 1})
    want = np.full(nb, CLEAN, dtype=np.int32)
    for i, b in enumerate(hit):
        x = i % (k + m)
        (data if x < k else parity)[b, x % k, (i * 211) % S] ^= 1 << (i % 8)
        want[b] = want_verdict(k, m, np.concatenate([data[b], parity[b]]))
        assert want[b] == x
    with rsmi.Codec(k, m) as c:
        c.set_option("small_call_bytes", 0)
        d0, p0 = data.copy(), parity.copy()
        got, bad = _host_locate(c, data.ctypes.data, k * S, parity.ctypes.data, m * S, S, nb)
        assert c.last_kernel() == "rs_locate_kernel<K=2,MT=2>"
        assert np.array_equal(data, d0) and np.array_equal(parity, p0)
        assert np.array_equal(np.flatnonzero(got != CLEAN), np.array(hit)), np.flatnonzero(got != CLEAN)
        assert np.array_equal(got, want)
        assert np.array_equal(np.flatnonzero(bad.any(axis=1)), np.array(hit))
        got, bad = _host_locate(c, data.ctypes.data, k * S, parity.ctypes.data, m * S, S, nb, flags=False)
        assert np.array_equal(got, want)


# ---------------------------------------------------------------- 11: round trip
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "split"])
def test_locate_then_repair(gpu, aligned):
    """Locate, then reconstruct_rows_batch_dev with the culprit marked missing and required: Verify
    reports clean and the bytes are the original ones."""
    torch, rsmi = gpu
    k, m, S, nb = 10, 4, 4099, 2
    n = k + m
    lay = Lay(rsmi, k, m, S, nb, aligned)
    full = stripes(k, m, S, nb)
    h = torch.cuda.current_stream().cuda_stream
    with rsmi.Codec(k, m) as c:
        for x in (4, k + 1):
            sh = full.copy()
            sh[:, x, 100:3100] ^= 0xFF  # the same shard stale in both blocks: one erasure pattern
            host = lay.fill(sh)
            got, _ = run_dev(torch, c, lay, host, label(lay))
            assert got.tolist() == [x, x] == want_verdicts(k, m, sh).tolist()
            d = torch.from_numpy(host).cuda()
            base = d.data_ptr() + lay.off
            c.reconstruct_rows_batch_dev(base, lay.rs, lay.bs, S, nb, [i != x for i in range(n)],
                                         [i == x for i in range(n)], h)
            torch.cuda.synchronize()
            after = d.cpu().numpy()
            assert np.array_equal(after, lay.fill(full))
            assert not verify_flags(torch, c, lay, after).any()
            got, bad = run_dev(torch, c, lay, after, label(lay))
            assert (got == CLEAN).all() and not bad.any()


# ---------------------------------------------------------------- 12: no side effects
@pytest.mark.gpu
def test_no_side_effects_on_encode_reconstruct_verify(gpu):
    """The plan cache and the scratch are shared: after a locate (and after a fallback locate's
    scratch encode) the context's encode, reconstruct and verify still match the oracle and report
    their own labels."""
    torch, rsmi = gpu
    for k, m, S, llabel, vlabel, elabel, rlabel in (
            (10, 4, 4099, "rs_locate_kernel<K=10,MT=4>", "rs_verify_kernel<K=10,MT=4>",
             "rs_fast_kernel<K=10,MT=4,NT=1>", "rs_fast_kernel<K=10,MT=2,NT=2>"),
            (7, 2, 1025, ROWS, "rs_compare_rows_kernel", "rs_generic_kernel<K=7,MT=2>", "rs_generic_kernel<K=7,MT=2>")):
        nb = 3
        lay = Lay(rsmi, k, m, S, nb, True)
        full = stripes(k, m, S)
        sh = full.copy()
        sh[1, 2, 1000] ^= 0x77
        with rsmi.Codec(k, m) as c:
            assert check(torch, c, lay, sh, llabel).tolist() == [CLEAN, 2, CLEAN]
            host = lay.fill(full)
            lay.rows(host)[:, k:] = 0xEE
            d = torch.from_numpy(host).cuda()
            h = torch.cuda.current_stream().cuda_stream
            c.encode_batch_dev(d.data_ptr(), lay.rs, lay.bs, d.data_ptr() + k * lay.rs, lay.rs, lay.bs, S, nb, h)
            torch.cuda.synchronize()
            assert c.last_kernel() == elabel
            assert np.array_equal(d.cpu().numpy(), lay.fill(full))
            lost = [1, k + 1]
            host = lay.fill(full)
            lay.rows(host)[:, lost] = 0xEE
            d = torch.from_numpy(host).cuda()
            c.reconstruct_batch_dev(d.data_ptr(), lay.rs, lay.bs, S, nb, [i not in lost for i in range(k + m)],
                                    False, h)
            torch.cuda.synchronize()
            assert c.last_kernel() == rlabel
            assert np.array_equal(d.cpu().numpy(), lay.fill(full))
            host = lay.fill(sh)
            assert np.array_equal(verify_flags(torch, c, lay, host), want_flags(k, m, sh))
            assert c.last_kernel() == vlabel
            assert check(torch, c, lay, sh, llabel).tolist() == [CLEAN, 2, CLEAN]
