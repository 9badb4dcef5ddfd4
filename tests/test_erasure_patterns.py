"""Every erasure pattern of the shipped shapes, bit for bit.

A pattern (the set of lost rows) picks the k survivor rows, the k x k sub-matrix that is inverted,
the parity decode rows M[i] x inverse, and the in_row / out_row maps and v_perm tables of the
RsPlanDev that is uploaded for it.  The other modules run a handful of patterns per shape; this one
runs all of them, 1..m rows lost, for the shipped shapes RS(2,1), RS(4,2), RS(10,4), RS(16,4) and
the golden RS(5,5): 3 / 21 / 1470 / 6195 / 637 patterns.

CPU legs.  The reference is GF(2^8) restated in numpy inside this module (exp / log tables from
0x11D with generator 2, a 256 x 256 product table, matrix product, Gauss-Jordan inverse); it imports
nothing from the library or from oracle/.  Leg 1 pins the encode matrices of the library and of the
oracle to it, leg 2 every pattern's decode matrix, leg 3 the oracle's own reconstruct pattern by
pattern, and leg 4 asserts which coefficient values the sweep puts through which (output slot,
input column) of the kernels' per-coefficient tables: with data rows that hold every byte value the
device sweep is then a complete product-table test of the hot kernel.

GPU legs.  One block of S = 273 bytes per pattern (17 whole 16-byte chunks plus one byte), every
data row a permutation of 0..255 plus 17 more bytes, parity from the oracle; all patterns of a case
are slices of one device buffer, every launch is queued, and the whole buffer (guards and padding
included) is compared once per chunk of at most 512 patterns, each chunk on a fresh Codec because
a context's plan cache never evicts.  The expected bytes of a rebuilt row are the original row.

Everything is bit-exact: there are no tolerances.
"""
import ctypes
import functools
import itertools
import time

import numpy as np
import pytest

import oracle_lib as orc
from test_kernel_matrix import Layout, _stream, fast_label, generic_label, nt_of

SHIPPED = [(2, 1), (4, 2), (10, 4), (16, 4), (5, 5)]
COUNTS = {(2, 1): 3, (4, 2): 21, (10, 4): 1470, (16, 4): 6195, (5, 5): 637}
MATRIX_SHAPES = SHIPPED + [(20, 4), (64, 64), (200, 56), (255, 1), (1, 255)]
WIDE = [(20, 4, 300), (64, 64, 16)]     # (k, m, seeded patterns): K > 16 runs rs_generic_kernel
S_GPU = 273
S_WIDE = 37
CHUNK = 512                              # patterns per Codec: bounds the plan cache
FILL, GUARD = 0xEE, 0x5A


def _id(km):
    return "%d+%d" % (km[0], km[1])


# ---------------------------------------------------------------- GF(2^8) in numpy, independent
def _tables():
    exp = np.zeros(510, dtype=np.int64)
    log = np.zeros(256, dtype=np.int64)
    x = 1
    for i in range(255):
        exp[i] = x
        log[x] = i
        x <<= 1
        if x & 0x100:
            x ^= 0x11D
    exp[255:] = exp[:255]
    a = np.arange(256)
    mul = exp[log[a][:, None] + log[a][None, :]]
    mul[0, :] = 0
    mul[:, 0] = 0
    inv = np.zeros(256, dtype=np.uint8)
    inv[1:] = exp[(255 - log[1:]) % 255]
    return exp, log, mul.astype(np.uint8), inv


EXP, LOG, MUL, INV = _tables()


def gf_matmul(a, b):
    return np.bitwise_xor.reduce(MUL[a[:, :, None], b[None, :, :]], axis=1)


def gf_inv(a):
    """Gauss-Jordan on [a | I]; None when a is singular."""
    n = a.shape[0]
    w = np.concatenate([a, np.eye(n, dtype=np.uint8)], axis=1)
    for r in range(n):
        nz = np.flatnonzero(w[r:, r])
        if nz.size == 0:
            return None
        s = r + int(nz[0])
        if s != r:
            w[[r, s]] = w[[s, r]]
        w[r] = MUL[INV[w[r, r]], w[r]]
        f = w[:, r].copy()
        f[r] = 0
        w ^= MUL[f[:, None], w[r][None, :]]
    return w[:, n:].copy()


@functools.lru_cache(maxsize=None)
def ref_matrix(k, m):
    """Vandermonde (r^c, 0^0 = 1) of n x k times the inverse of its top square."""
    n = k + m
    r = np.arange(n)[:, None]
    c = np.arange(k)[None, :]
    vm = EXP[(LOG[r] * c) % 255].astype(np.uint8)
    vm[0, :] = 0
    vm[:, 0] = 1
    M = gf_matmul(vm, gf_inv(vm[:k]))
    M.setflags(write=False)
    return M


def patterns(k, m, lo=1, hi=None):
    n = k + m
    hi = m if hi is None else hi
    return [c for r in range(lo, hi + 1) for c in itertools.combinations(range(n), r)]


def first_present(n, k, lost):
    return [i for i in range(n) if i not in lost][:k]


@functools.lru_cache(maxsize=None)
def sweep(k, m):
    """Per pattern, from the numpy reference alone: (lost, used, dec, coef).  coef holds the rows the
    pattern's plan carries, in reconstruct_plan's order: dec[i] for the lost data rows ascending,
    then M[i] x dec for the lost parity rows ascending."""
    n = k + m
    M = ref_matrix(k, m)
    decs = {}
    out = []
    for lost in patterns(k, m):
        used = tuple(first_present(n, k, lost))
        if used not in decs:
            decs[used] = gf_inv(M[list(used)])
            assert decs[used] is not None, ("singular", k, m, lost)
        dec = decs[used]
        ld = [i for i in lost if i < k]
        lp = [i for i in lost if i >= k]
        coef = dec[ld]
        if lp:
            coef = np.concatenate([coef, gf_matmul(M[lp], dec)])
        out.append((lost, used, dec, coef))
    return out


def test_reference_tables():
    """The product table against shift-and-add multiplication modulo 0x11D, and the inverses."""
    a = np.arange(256)[:, None] * np.ones((1, 256), dtype=np.int64)
    b = a.T.copy()
    acc = np.zeros((256, 256), dtype=np.int64)
    for _ in range(8):
        acc ^= a * (b & 1)
        b >>= 1
        a <<= 1
        a ^= (a >> 8 & 1) * 0x11D
    assert np.array_equal(acc, MUL)
    assert (MUL[np.arange(1, 256), INV[1:]] == 1).all()
    assert MUL[3, 4] == 12 and MUL[7, 7] == 21 and MUL[23, 45] == 41  # upstream galMultiply answers


def test_pattern_counts():
    for km in SHIPPED:
        assert len(patterns(*km)) == COUNTS[km]


# ---------------------------------------------------------------- leg 1: encode matrices
@pytest.mark.parametrize("km", MATRIX_SHAPES, ids=_id)
def test_encode_matrix_against_numpy(km):
    import rsmi

    k, m = km
    M = ref_matrix(k, m)
    assert np.array_equal(M[:k], np.eye(k, dtype=np.uint8))
    assert np.array_equal(orc.build_matrix(k, m), M)
    with rsmi.Codec(k, m) as c:
        got = np.frombuffer(c.encode_matrix(), dtype=np.uint8).reshape(k + m, k)
    assert np.array_equal(got, M)


# ---------------------------------------------------------------- leg 2: every decode matrix
@pytest.mark.parametrize("km", SHIPPED, ids=_id)
def test_every_decode_matrix(km):
    """rsmi_decode_matrix for every pattern: RSMI_OK, used_rows the first k present indices, the
    matrix equal to rs_oracle_invert of those rows of M and to the numpy inverse, and
    M[used] x dec == I in the numpy field.  Every (or 50 seeded) m+1-loss pattern is refused."""
    import rsmi

    k, m = km
    n = k + m
    M = ref_matrix(k, m)
    eye = np.eye(k, dtype=np.uint8)
    sw = sweep(k, m)
    assert len(sw) == COUNTS[km]
    with rsmi.Codec(k, m) as c:
        for lost, used, dec, _ in sw:
            present = [i not in lost for i in range(n)]
            try:
                raw, got_used = c.decode_matrix(present)
            except rsmi.RsmiError as e:
                pytest.fail("rsmi_decode_matrix RS(%d,%d) lost %s: status %d" % (k, m, lost, e.code))
            assert got_used == list(used), (k, m, lost, got_used)
            got = np.frombuffer(raw, dtype=np.uint8).reshape(k, k)
            sub = np.ascontiguousarray(M[list(used)]).reshape(-1)
            inv = np.zeros(k * k, dtype=np.uint8)
            assert orc.lib().rs_oracle_invert(orc.ptr(sub), orc.ptr(inv), k) == 0, (k, m, lost)
            assert np.array_equal(got, inv.reshape(k, k)), ("library != oracle", k, m, lost)
            assert np.array_equal(gf_matmul(M[list(used)], got), eye), ("M[used] x dec != I", k, m, lost)
            assert np.array_equal(got, dec), ("library != numpy", k, m, lost)
        if km in ((2, 1), (4, 2)):
            few = patterns(k, m, m + 1, m + 1)
        else:
            rng = np.random.default_rng(200 + n)
            few = [tuple(sorted(int(x) for x in rng.choice(n, size=m + 1, replace=False))) for _ in range(50)]
        for lost in few:
            with pytest.raises(rsmi.RsmiError) as e:
                c.decode_matrix([i not in lost for i in range(n)])
            assert e.value.code == rsmi.ErrTooFewShards, (k, m, lost)


# ---------------------------------------------------------------- leg 3: the oracle's reconstruct
@pytest.mark.parametrize("km", SHIPPED, ids=_id)
def test_oracle_reconstruct_every_pattern(km):
    """rs_oracle_reconstruct at S = 5, both data_only modes, against rows computed in numpy: data
    rows dec[i] . survivors, parity rows (M[i] x dec) . survivors, everything else untouched."""
    k, m = km
    n = k + m
    S = 5
    M = ref_matrix(k, m)
    data = np.random.default_rng(300 + n).integers(0, 256, size=(k, S), dtype=np.uint8)
    full = np.concatenate([data, gf_matmul(M[k:], data)])
    assert np.array_equal(full[k:], orc.encode(k, m, data))
    for lost, used, dec, coef in sweep(k, m):
        present = [i not in lost for i in range(n)]
        erased = full.copy()
        erased[list(lost)] = FILL
        rebuilt = gf_matmul(coef, full[list(used)])     # rows in the order of sorted(lost)
        nd = sum(1 for i in lost if i < k)
        for data_only in (False, True):
            want = list(lost)[:nd] if data_only else list(lost)
            expect = erased.copy()
            expect[want] = rebuilt[:len(want)]
            rc, sh = orc.reconstruct(k, m, erased, present, data_only)
            assert rc == 0, (k, m, lost, data_only, rc)
            assert np.array_equal(sh, expect), (k, m, lost, data_only)
        assert np.array_equal(rebuilt, full[list(lost)]), ("numpy rebuild != original", k, m, lost)


# ---------------------------------------------------------------- leg 4: coefficient coverage
def _coverage(k, m):
    """cov[j, c, v]: some pattern's plan carries coefficient v at output slot j (row index mod 4
    within the plan's tiles) for input column c."""
    cov = np.zeros((4, k, 256), dtype=bool)
    cols = np.arange(k)
    for _, _, _, coef in sweep(k, m):
        for idx in range(coef.shape[0]):
            cov[idx % 4, cols, coef[idx]] = True
    return cov


def test_coverage_16_4_every_value_at_every_slot_and_column():
    cov = _coverage(16, 4)
    missing = np.argwhere(~cov[:, :, 1:])
    assert missing.size == 0, "(slot, column, value - 1) never coded: %s" % missing[:8].tolist()


def test_coverage_10_4_every_value_at_every_slot():
    cov = _coverage(10, 4)
    per_slot = cov.any(axis=1)
    missing = np.argwhere(~per_slot[:, 1:])
    assert missing.size == 0, "(slot, value - 1) never coded: %s" % missing[:8].tolist()


# ---------------------------------------------------------------- GPU plumbing
WALL = {}
NPAT = {}
MEM = {}


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    rsmi = pytest.importorskip("rsmi")
    if not torch.cuda.is_available() or rsmi.device_count() == 0:
        pytest.skip("no GPU")
    yield torch, rsmi
    print("\nerasure patterns: case, patterns, wall seconds:")
    for key in WALL:
        print("  %-28s %5d  %.2f" % (key, NPAT.get(key, 0), WALL[key]))
    for key, v in MEM.items():
        print("erasure patterns: free device memory taken by one %d-pattern chunk of %s: %d bytes" %
              (v[0], key, v[1]))


@functools.lru_cache(maxsize=None)
def _block(k, m, S):
    """One block: every data row a seeded permutation of 0..255 (where S allows) followed by seeded
    bytes, parity from the oracle.  Shared and read-only."""
    rng = np.random.default_rng(7000 + 100 * k + m)
    rows = []
    for _ in range(k):
        head = rng.permutation(256).astype(np.uint8)[:min(S, 256)]
        rows.append(np.concatenate([head, rng.integers(0, 256, size=S - head.size, dtype=np.uint8)]))
    data = np.stack(rows)
    full = np.concatenate([data, orc.encode(k, m, data)])
    full.setflags(write=False)
    return full


def _wanted(mode, k, n, lost, p):
    """(rows the call must rebuild, the call's `required` rows or None)."""
    if mode == "rows":
        lone = lost[p % len(lost)]
        here = [i for i in range(n) if i not in lost]
        return [lone], [lone, here[p % len(here)]]
    if mode == "data_only":
        return [i for i in lost if i < k], None
    return list(lost), None


def _label(k, nwant, ua, fast=True):
    last = (nwant - 1) % 4 + 1    # tiles of at most 4 output rows: the last one labels the call
    return fast_label(k, last, ua=ua) if fast else generic_label(k, last)


def _run_patterns(torch, rsmi, k, m, mode, pats, S, key, fast=True):
    n = k + m
    ua = mode == "split"
    full = _block(k, m, S)
    NPAT[key] = len(pats)
    t0 = time.perf_counter()
    for c0 in range(0, len(pats), CHUNK):
        chunk = pats[c0:c0 + CHUNK]
        nb = len(chunk)
        lay = Layout(rsmi, n, S, nb, ua, off=1 if ua else 0, rs=S if ua else None)
        lostmask = np.zeros((nb, n), dtype=bool)
        wantmask = np.zeros((nb, n), dtype=bool)
        calls = []
        for b, lost in enumerate(chunk):
            want, required = _wanted(mode, k, n, lost, c0 + b)
            lostmask[b, list(lost)] = True
            wantmask[b, want] = True
            calls.append((want, required))
        erased = lay.buffer(GUARD)
        lay.rows(erased)[:] = full
        lay.rows(erased)[lostmask] = FILL
        expect = erased.copy()
        lay.rows(expect)[wantmask] = np.broadcast_to(full, (nb, n, S))[wantmask]
        d = torch.from_numpy(erased).cuda()
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        with rsmi.Codec(k, m) as c:
            prev = c.last_kernel()
            for b, lost in enumerate(chunk):
                want, required = calls[b]
                present = [i not in lost for i in range(n)]
                base = d.data_ptr() + lay.off + b * lay.bs
                if mode == "rows":
                    c.reconstruct_rows_batch_dev(base, lay.rs, lay.bs, S, 1, present,
                                                 [i in required for i in range(n)], _stream(torch))
                else:
                    c.reconstruct_batch_dev(base, lay.rs, lay.bs, S, 1, present, mode == "data_only",
                                            _stream(torch))
                kern = c.last_kernel()
                if want:
                    assert kern == _label(k, len(want), ua, fast), (kern, k, m, mode, lost, want)
                else:   # parity-only loss with data_only: OK, no launch
                    assert kern == prev, (kern, prev, k, m, mode, lost)
                prev = kern
            torch.cuda.synchronize()
            if nb == CHUNK and key not in MEM:
                MEM[key] = (nb, free0 - torch.cuda.mem_get_info()[0])
            got = d.cpu().numpy()
        if not np.array_equal(got, expect):
            at = int(np.flatnonzero(got != expect)[0])
            b = min(max(at - lay.off, 0) // lay.bs, nb - 1)
            row, x = divmod(max(at - lay.off, 0) - b * lay.bs, lay.rs)
            pytest.fail("RS(%d,%d) %s: pattern %d lost %s wanted %s: byte %d (block %d row %d offset %d) is "
                        "0x%02x, expected 0x%02x" % (k, m, mode, c0 + b, chunk[b], calls[b][0], at, b, row, x,
                                                     got[at], expect[at]))
    WALL[key] = time.perf_counter() - t0


# ---------------------------------------------------------------- GPU: the exhaustive sweep
MODES = ["all", "split", "data_only", "rows"]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("km", SHIPPED, ids=_id)
def test_every_pattern_on_device(gpu, km, mode):
    """all: rsmi_reconstruct_batch_dev, data_only=0, aligned pitched rows.  split: the same with
    rows back to back at pitch S from a base misaligned by one byte (the ",UA" kernels).
    data_only: data_only=1, aligned; a parity-only loss is a no-op without a launch.  rows:
    rsmi_reconstruct_rows_batch_dev, aligned, required = the lost row lost[p % len(lost)] of
    pattern number p plus one present row.  Wanted lost rows come back as the original, lost rows
    not asked for keep their 0xEE fill, present rows, padding and guards are untouched, and the
    label's MT is the number of wanted rows (their last tile past 4)."""
    torch, rsmi = gpu
    k, m = km
    pats = patterns(k, m)
    assert len(pats) == COUNTS[km]
    _run_patterns(torch, rsmi, k, m, mode, pats, S_GPU, "%s %s" % (_id(km), mode))


# ---------------------------------------------------------------- GPU: verified degraded reads
@pytest.mark.gpu
@pytest.mark.parametrize("km", [(4, 2), (10, 4)], ids=_id)
def test_every_pattern_verified_read(gpu, km):
    """rsmi_reconstruct_batch_host_verify on one page-locked block for every pattern: the rebuild
    equals the original and raw16_in[c] folds to the oracle's CRC-16 of shard used[c], used = the
    first k present rows.  One block with coalesce_flag 1 is the one-base table launch."""
    torch, rsmi = gpu
    k, m = km
    n, S = k + m, S_GPU
    full = _block(k, m, S)
    crc = [orc.crc16_ibm(r.tobytes()) for r in full]
    pats = patterns(k, m)
    key = "%s verify" % _id(km)
    NPAT[key] = len(pats)
    L = rsmi.lib()
    p = L.rsmi_host_alloc(n * S)
    assert p
    t0 = time.perf_counter()
    try:
        sh = np.ctypeslib.as_array((ctypes.c_uint8 * (n * S)).from_address(p)).reshape(n, S)
        raw = np.zeros(k, dtype=np.uint32)
        for c0 in range(0, len(pats), CHUNK):
            with rsmi.Codec(k, m) as c:
                c.set_option("coalesce_flag", 1)
                for lost in pats[c0:c0 + CHUNK]:
                    present = [i not in lost for i in range(n)]
                    used = first_present(n, k, lost)
                    sh[:] = full
                    sh[list(lost)] = FILL
                    raw[:] = 0xDEAD0000
                    c.reconstruct_batch_host_verify_ptr(p, n * S, S, 1, present, False, raw.ctypes.data)
                    kern = c.last_kernel()
                    assert kern == ("rs_fused_mfma_kernel<K=%d,MT=%d,NT=%d>,UA,INL,TB" %
                                    (k, len(lost), nt_of(k, len(lost)))), (kern, lost)
                    assert np.array_equal(sh, full), (k, m, lost)
                    assert (raw < 0x10000).all(), (k, m, lost, raw)
                    got = [rsmi.crc16_entry(b"", int(x), S) for x in raw]
                    assert got == [crc[i] for i in used], (k, m, lost, used)
        del sh
    finally:
        L.rsmi_host_free(p)
    WALL[key] = time.perf_counter() - t0


# ---------------------------------------------------------------- GPU: wide shapes, sampled
@pytest.mark.gpu
@pytest.mark.parametrize("k,m,count", WIDE, ids=["20+4", "64+64"])
def test_sampled_patterns_wide_shapes(gpu, k, m, count):
    """K > 16 has no fast kernel: seeded patterns of 1..m lost rows through rs_generic_kernel (up
    to 16 tiles of 4 rows for RS(64,64)).  The only sampled leg."""
    torch, rsmi = gpu
    n = k + m
    rng = np.random.default_rng(9000 + n)
    pats = []
    for _ in range(count):
        r = int(rng.integers(1, m + 1))
        pats.append(tuple(sorted(int(x) for x in rng.choice(n, size=r, replace=False))))
    _run_patterns(torch, rsmi, k, m, "all", pats, S_WIDE, "%d+%d all (sampled)" % (k, m), fast=False)


# ---------------------------------------------------------------- GPU: too few shards
@pytest.mark.gpu
@pytest.mark.parametrize("km", SHIPPED + [(20, 4), (64, 64)], ids=_id)
def test_too_few_shards_on_device(gpu, km):
    """m + 1 rows lost: ErrTooFewShards from both device entry points, the buffer byte-identical
    and rsmi_last_kernel still the label of the valid call before."""
    torch, rsmi = gpu
    k, m = km
    n = k + m
    S = S_GPU if k <= 16 else S_WIDE
    full = _block(k, m, S)
    rng = np.random.default_rng(9500 + n)
    lost = sorted(int(x) for x in rng.choice(n, size=m + 1, replace=False))
    lay = Layout(rsmi, n, S, 1, False)
    host = lay.buffer(GUARD)
    lay.rows(host)[:] = full
    lay.rows(host)[0, lost] = FILL
    d = torch.from_numpy(host).cuda()
    with rsmi.Codec(k, m) as c:
        # a valid one-row rebuild first: the label to keep, and the row is lost again afterwards
        c.reconstruct_batch_dev(d.data_ptr(), lay.rs, lay.bs, S, 1, [i != lost[0] for i in range(n)], False,
                                _stream(torch))
        torch.cuda.synchronize()
        before = c.last_kernel()
        assert before == _label(k, 1, False, fast=k <= 16), before
        d.copy_(torch.from_numpy(host))
        present = [i not in lost for i in range(n)]
        with pytest.raises(rsmi.RsmiError) as e:
            c.reconstruct_batch_dev(d.data_ptr(), lay.rs, lay.bs, S, 1, present, False, _stream(torch))
        assert e.value.code == rsmi.ErrTooFewShards
        with pytest.raises(rsmi.RsmiError) as e:
            c.reconstruct_rows_batch_dev(d.data_ptr(), lay.rs, lay.bs, S, 1, present,
                                         [i == lost[0] for i in range(n)], _stream(torch))
        assert e.value.code == rsmi.ErrTooFewShards
        torch.cuda.synchronize()
        assert c.last_kernel() == before
    assert np.array_equal(d.cpu().numpy(), host), (k, m, lost)
