"""Seeded random-shape parity sweep on the GPU: random (k, m), shard sizes, batch sizes,
layouts (aligned pitches, padded strides, unaligned offsets) and erasure patterns, every
result compared byte for byte with the CPU oracle.  Complements the fixed grids of
test_gpu_parity.py with shapes nobody picked by hand.  The last part does the same for verify,
locate and heal: random shapes, sizes, independent data and parity layouts and damage per block,
against the definition."""
import numpy as np
import pytest

import oracle_lib as orc
import rsmi

CASES = 60


def _case(seed):
    r = np.random.default_rng(1000 + seed)
    k = int(r.choice([1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 16, 17, 20]))
    m = int(r.integers(1, min(8, 256 - k) + 1))
    S = int(r.choice([1, 2, 15, 16, 17, int(r.integers(1, 5000)), int(r.integers(5000, 70000))]))
    nb = int(r.integers(1, 9))
    layout = r.choice(["pitched", "padded", "unaligned"])
    nlost = int(r.integers(1, m + 1))
    lost = sorted(int(x) for x in r.choice(k + m, size=nlost, replace=False))
    data_only = bool(r.integers(0, 2))
    return k, m, S, nb, str(layout), lost, data_only, r


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(CASES))
def test_random_shape_encode_reconstruct(seed):
    import torch

    k, m, S, nb, layout, lost, data_only, r = _case(seed)
    n = k + m
    if layout == "pitched":
        rs, off = rsmi.recommended_pitch(S), 0
    elif layout == "padded":
        rs, off = (S + 15) // 16 * 16 + 48, 0
    else:
        rs, off = S + 3, 7
    bs = n * rs + (16 if layout == "padded" else 0)
    host = np.zeros(off + nb * bs + 64, dtype=np.uint8)
    data = r.integers(0, 256, size=(nb, k, S), dtype=np.uint8)
    for b in range(nb):
        for c in range(k):
            host[off + b * bs + c * rs:][:S] = data[b, c]
    d = torch.from_numpy(host).cuda()
    base = d.data_ptr() + off
    st = torch.cuda.current_stream().cuda_stream
    with rsmi.Codec(k, m) as c:
        c.encode_batch_dev(base, rs, bs, base + k * rs, rs, bs, S, nb, st)
        torch.cuda.synchronize()
        got = d.cpu().numpy()
        want = orc.encode_fast(k, m, data, threads=4)
        full = np.zeros((nb, n, S), dtype=np.uint8)
        full[:, :k] = data
        full[:, k:] = want
        for b in range(nb):
            for j in range(m):
                assert np.array_equal(got[off + b * bs + (k + j) * rs:][:S], want[b, j]), (b, j)
        # erase and rebuild
        for b in range(nb):
            for i in lost:
                d[off + b * bs + i * rs: off + b * bs + i * rs + S] = 0
        present = [i not in lost for i in range(n)]
        c.reconstruct_batch_dev(base, rs, bs, S, nb, present, data_only, st)
        torch.cuda.synchronize()
        got = d.cpu().numpy()
    for b in range(nb):
        for i in range(n):
            row = got[off + b * bs + i * rs:][:S]
            if i not in lost or i < k or not data_only:
                assert np.array_equal(row, full[b, i]), (k, m, S, layout, lost, data_only, b, i)
            else:
                assert not row.any()


GROUP_CASES = 16


def _group_case(seed):
    r = np.random.default_rng(5000 + seed)
    k, m = [(2, 1), (4, 2), (10, 4), (16, 4), (3, 2), (10, 4)][int(r.integers(0, 6))]
    B = int(r.choice([int(r.integers(1, 64)), int(r.integers(64, 5000)), int(r.integers(5000, 300000)),
                      262144, 1048576 + 14]))
    T = int(r.choice([2, 3, int(r.integers(4, 20)), int(r.integers(60, 70))]))
    crc = bool(r.integers(0, 2))
    nlost = int(r.integers(1, m + 1))
    lost = sorted(int(x) for x in r.choice(k + m, size=nlost, replace=False))
    data_only = bool(r.integers(0, 2))
    return k, m, B, T, crc, lost, data_only, r


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(GROUP_CASES))
def test_random_coalesced_groups(seed):
    """Seeded random coalesced groups (DagNode.Put / degraded Get from T goroutines at once,
    node.go:358-408 / :220-326) over page-locked buffers: random (k, m) among the table shapes and
    one without, block sizes from 1 byte to 1 MiB + 14 (rows under 16 bytes, aligned and odd
    shard sizes), 2..69 requests in one deterministic batch (one lane, coalesce_us; more than 64
    take two table launches), with and without CRC-16, then a random loss pattern rebuilt the same
    way.  Every shard, R(shard) and rebuilt row equals the oracle's; rows not asked for stay
    untouched."""
    import ctypes
    import threading

    k, m, B, T, crc, lost, data_only, r = _group_case(seed)
    n = k + m
    S = (B + k - 1) // k
    L = rsmi.lib()
    blocks = [bytes(r.integers(0, 256, size=B, dtype=np.uint8)) for _ in range(T)]
    want = []
    for b in blocks:
        w = orc.split(k, m, b)
        w[k:] = orc.encode(k, m, w[:k])
        want.append(w)
    ptrs = [L.rsmi_host_alloc(n * S) for _ in range(T)]
    assert all(ptrs)
    try:
        views = [np.ctypeslib.as_array((ctypes.c_uint8 * (n * S)).from_address(p)).reshape(n, S) for p in ptrs]
        raws = [(ctypes.c_uint32 * n)() for _ in range(T)]
        with rsmi.Codec(k, m) as c:
            c.set_option("coalesce_lanes", 1)
            c.set_option("coalesce_us", 100000)
            c.set_option("coalesce_max", T)
            for t in range(T):
                flat = views[t].reshape(-1)
                flat[:] = 0x5A
                flat[:B] = np.frombuffer(blocks[t], dtype=np.uint8)
            rcs = [None] * T

            def enc(t):
                rcs[t] = L.rsmi_encode_block_coalesced(c._h, ptrs[t], B, ptrs[t], raws[t] if crc else None)

            th = [threading.Thread(target=enc, args=(t,)) for t in range(T)]
            for x in th:
                x.start()
            for x in th:
                x.join()
            assert rcs == [0] * T, c.last_kernel()
            for t in range(T):
                assert np.array_equal(views[t], want[t]), (t, c.last_kernel())
                for i in range(n if crc else 0):
                    assert rsmi.crc16_entry(b"", raws[t][i], S) == orc.crc16_ibm(want[t][i].tobytes()), (t, i)
            present = (ctypes.c_uint8 * n)(*[0 if i in lost else 1 for i in range(n)])
            for t in range(T):
                views[t][lost] = 0xEE

            def rec(t):
                rcs[t] = L.rsmi_reconstruct_coalesced(c._h, ptrs[t], S, present, 1 if data_only else 0)

            th = [threading.Thread(target=rec, args=(t,)) for t in range(T)]
            for x in th:
                x.start()
            for x in th:
                x.join()
            assert rcs == [0] * T
            for t in range(T):
                for i in range(n):
                    if i in lost and data_only and i >= k:
                        assert (views[t][i] == 0xEE).all(), (t, i)
                    else:
                        assert np.array_equal(views[t][i], want[t][i]), (t, i, c.last_kernel())
    finally:
        for p in ptrs:
            L.rsmi_host_free(p)


LONE_CASES = 24


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(LONE_CASES))
def test_random_lone_in_place_calls(seed):
    """Seeded random one-block in-place host calls on page-locked memory -- a lone DagNode.Put,
    repair, degraded and verified read (node.go:358-408, :220-326, data_recovery.go:16-112) --
    which take the one-base table launches with completion flags where the shape has them and
    the plain launches and stream synchronisation where it does not (rows under 16 bytes, shapes
    without table kernels, 5+ lost rows): random (k, m), block sizes from 1 byte to 1 MiB + 14,
    random loss patterns, the option coalesce_flag on and off.  Shards, R(shard), rebuilt rows and
    the survivors' R(row) against the oracle."""
    import ctypes

    r = np.random.default_rng(9000 + seed)
    k, m = [(2, 1), (4, 2), (10, 4), (16, 4), (3, 2), (5, 5), (10, 4)][int(r.integers(0, 7))]
    B = int(r.choice([int(r.integers(1, 64)), int(r.integers(64, 5000)), int(r.integers(5000, 300000)),
                      262144, 1048576 + 14]))
    flag = int(r.integers(0, 2))
    n = k + m
    S = (B + k - 1) // k
    L = rsmi.lib()
    p = L.rsmi_host_alloc(n * S)
    assert p
    try:
        sh = np.ctypeslib.as_array((ctypes.c_uint8 * (n * S)).from_address(p)).reshape(n, S)
        block = r.integers(0, 256, size=B, dtype=np.uint8)
        full = orc.split(k, m, block.tobytes())
        full[k:] = orc.encode(k, m, full[:k])
        r16 = [orc.crc16_ibm(full[i].tobytes()) for i in range(n)]
        with rsmi.Codec(k, m) as c:
            c.set_option("coalesce_flag", flag)
            for rep in range(3):  # the flag slots reused
                sh[:] = 0x5A
                sh[:k] = full[:k]
                raw = np.zeros(n, dtype=np.uint32)
                c.encode_batch_host_crcs_ptr(p, n * S, p + k * S, n * S, S, 1, raw.ctypes.data, None)
                assert np.array_equal(sh, full), (k, m, B, rep)
                assert [rsmi.crc16_entry(b"", int(x), S) for x in raw] == r16, (k, m, B, rep)
                nlost = int(r.integers(1, m + 1))
                lost = sorted(int(x) for x in r.choice(n, size=nlost, replace=False))
                present = [i not in lost for i in range(n)]
                sh[lost] = 0xEE
                c.reconstruct_rows_batch_host_ptr(p, n * S, S, 1, present, [i in lost for i in range(n)])
                assert np.array_equal(sh, full), (k, m, B, lost)
                if any(i < k for i in lost):
                    sh[lost] = 0xEE
                    v16 = np.zeros(k, dtype=np.uint32)
                    c.reconstruct_batch_host_verify_ptr(p, n * S, S, 1, present, True, v16.ctypes.data)
                    for i in range(n):
                        if i < k or i not in lost:
                            assert np.array_equal(sh[i], full[i]), (k, m, B, lost, i)
                    used = [i for i in range(n) if present[i]][:k]
                    assert [rsmi.crc16_entry(b"", int(v16[j]), S) for j in range(k)] == [r16[i] for i in used]
    finally:
        L.rsmi_host_free(p)


# ---------------------------------------------------------------- verify, locate and heal
# Seeded random stripe checks: shapes and sizes nobody picked (K = 7, 17 and 20, m = 5..8, rows
# shorter than 16 bytes and just past a tile), the two sides in layouts drawn independently, in one
# allocation or two, and the damage of every block drawn from DAMAGE.  The expected flags, verdicts
# and image are the definition's (test_verify.want_flags, test_locate.want_verdicts,
# test_heal.want_image, all on the CPU oracle); the labels are test_stripe_layouts.stripe_labels'.
STRIPE_CASES = 48
STRIPE_KS = [1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 16, 17, 20]
STRIPE_MS = [1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4, 5, 6, 7, 8]
LAYOUTS = ["pitched", "padded", "odd", "packed"]
LAYOUT_P = [0.3, 0.3, 0.2, 0.2]
DAMAGE = ["none", "padding", "one-byte", "burst", "stale-row", "one-shard-tiles", "two-shards-column",
          "two-shards-tiles", "two-parity-rows"]
_STRIPE = {}


def _stripe_side(layout, alloc, rows, S, nb, base):
    """One side's rows from offset base (a multiple of 16) of its allocation's payload."""
    from test_layout_contract import Side

    R = (S + 15) // 16 * 16
    if layout == "pitched":      # rsmi.recommended_pitch from an aligned base
        rs = rsmi.recommended_pitch(S)
        return Side(alloc, base, rs, rows * rs)
    if layout == "padded":       # round_up(S, 16) + 48, a block gap of 16
        return Side(alloc, base, R + 48, rows * (R + 48) + 16)
    if layout == "odd":          # rs = S + 3 from offset 7
        return Side(alloc, base + 7, S + 3, rows * (S + 3))
    return Side(alloc, base, S, rows * S)   # rs = S, back to back


def _burst(S):
    """A run of bytes across a 16-byte and a 1024-byte boundary, as far as the row reaches."""
    if S >= 1030:
        return 1003, min(S, 1045)
    if S > 16:
        return max(0, 16 - 9), min(S, 16 + 9)
    return 0, S


def _damage(r, kind, sh, k, m, S):
    """Damage one block's rows sh (n, S) in place; "none" and "padding" leave them alone."""
    n = k + m

    def val(size=None):
        return r.integers(1, 256, size=size, dtype=np.uint8)

    far = [p for p in (5, 1030, 2100, 4200, 9000, 19000) if p < S] or [0]
    if kind == "one-byte":
        sh[int(r.integers(0, n)), int(r.integers(0, S))] ^= val()
    elif kind == "burst":
        lo, hi = _burst(S)
        sh[int(r.integers(0, n)), lo:hi] ^= val(hi - lo)
    elif kind == "stale-row":
        sh[int(r.integers(0, n))] = r.integers(0, 256, size=S, dtype=np.uint8)
    elif kind == "one-shard-tiles":
        x = int(r.integers(0, n))
        for p in far + [S - 1]:
            sh[x, p] ^= val()
    elif kind in ("two-shards-column", "two-shards-tiles"):
        x0, x1 = (int(x) for x in r.choice(n, size=2, replace=False))
        p0 = int(r.integers(0, S))
        p1 = p0 if kind == "two-shards-column" else (p0 + max(1, min(S - 1, 1024 + int(r.integers(0, 2000))))) % S
        sh[x0, p0] ^= val()
        sh[x1, p1] ^= val()
    elif kind == "two-parity-rows":
        js = r.choice(m, size=min(2, m), replace=False)
        p0 = int(r.integers(0, S))
        for j in js:
            sh[k + int(j), p0] ^= val()


def _stripe_case(seed):
    """Everything a case needs, the definition's answers included, computed once per seed."""
    if seed in _STRIPE:
        return _STRIPE[seed]
    from test_heal import want_image
    from test_layout_contract import GUARD, blank, expected_form, put, row_at
    from test_locate import want_verdicts
    from test_verify import want_flags

    r = np.random.default_rng(77000 + seed)
    k = int(r.choice(STRIPE_KS))
    m = int(r.choice(STRIPE_MS))
    # U(1, 16) is there for the rows shorter than 16 bytes: U(1, 5000) draws one in 300 cases
    S = int(r.choice([16, 17, 31, int(r.integers(1, 16)), int(r.integers(1, 5000)), int(r.integers(5000, 20001))]))
    nb = int(r.integers(1, 7))
    dlay, play = (str(x) for x in r.choice(LAYOUTS, size=2, p=LAYOUT_P))
    one_alloc = bool(r.integers(0, 2))
    wpc1 = bool(r.integers(0, 4) == 0)
    d = _stripe_side(dlay, "x" if one_alloc else "d", k, S, nb, 0)
    pbase = (d.off + nb * d.bs + 15) // 16 * 16 + 32 if one_alloc else 0
    p = _stripe_side(play, "x" if one_alloc else "p", m, S, nb, pbase)
    data = r.integers(0, 256, size=(nb, k, S), dtype=np.uint8)
    sh = np.concatenate([data, orc.encode_fast(k, m, data, threads=4)], axis=1)
    kinds = [str(x) for x in r.choice(DAMAGE, size=nb)]
    for b in range(nb):
        _damage(r, kinds[b], sh[b], k, m, S)
    before = blank(d, p, nb)
    put(before, d, sh[:, :k])
    put(before, p, sh[:, k:])
    for b in range(nb):
        if kinds[b] != "padding":
            continue
        # a byte that belongs to no row: after a row where the pitch leaves one, in the gap behind
        # a block, or in the guard in front of the side's first row
        spots = []
        for side, rows in ((d, k), (p, m)):
            if side.rs > S:
                spots.append((side.alloc, row_at(side, b, int(r.integers(0, rows))) + S))
            if side.bs > rows * side.rs:
                spots.append((side.alloc, row_at(side, b, 0) + rows * side.rs))
            spots.append((side.alloc, row_at(side, 0, 0) - 1))
        a, o = spots[int(r.integers(0, len(spots)))]
        before[a][o] ^= 0xFF
    verdicts = want_verdicts(k, m, sh)
    image = want_image(k, m, sh, verdicts)
    want = {a: x.copy() for a, x in before.items()}
    put(want, d, image[:, :k])
    put(want, p, image[:, k:])
    form = expected_form(GUARD + d.off, d.rs, d.bs, GUARD + p.off, p.rs, p.bs, S)  # from 16-byte-aligned allocations
    case = dict(k=k, m=m, S=S, nb=nb, d=d, p=p, wpc1=wpc1, kinds=kinds, sh=sh, before=before, want=want, form=form,
                verdicts=verdicts, flags=want_flags(k, m, sh), image_flags=want_flags(k, m, image))
    _STRIPE[seed] = case
    return case


def test_stripe_generator_coverage():
    """The committed seed range reaches what the fuzz is there for (conditions on the generator,
    not measurements): every family of heal's labels, rows shorter than 16 bytes, every damage
    kind, every kind of verdict as the definition gives it, and the two sides at different shard
    strides in at least half the cases."""
    import collections

    from test_locate import CLEAN, UNKNOWN
    from test_stripe_layouts import family, stripe_labels

    fam, kinds, verdicts = collections.Counter(), collections.Counter(), collections.Counter()
    short = differ = 0
    for seed in range(STRIPE_CASES):
        c = _stripe_case(seed)
        k, m, S, d, p = c["k"], c["m"], c["S"], c["d"], c["p"]
        assert d.rs >= S and p.rs >= S and d.bs >= k * d.rs and p.bs >= m * p.rs
        assert d.alloc != p.alloc or d.off + c["nb"] * d.bs <= p.off
        label = stripe_labels(k, m, c["form"])[2]
        fam["m=1" if m == 1 else family(label)] += 1
        short += S < 16
        differ += d.rs != p.rs
        kinds.update(c["kinds"])
        for v in c["verdicts"].tolist():
            verdicts["clean" if v == CLEAN else "unknown" if v == UNKNOWN else "data" if v < k else "parity"] += 1
        # an UNKNOWN block alone keeps flags in the image
        assert np.array_equal(c["image_flags"].any(axis=1), c["verdicts"] == UNKNOWN), seed
    print("\nstripe fuzz generator: families", dict(fam), "damage", dict(kinds), "verdicts", dict(verdicts),
          "S < 16:", short, "sides differ in shard stride:", differ)
    assert fam["fused"] >= 5 and fam["fused,UA"] >= 5 and fam["rows"] >= 5 and fam["m=1"] >= 2, dict(fam)
    assert short >= 2, short
    for kind in DAMAGE:
        assert kinds[kind] >= 6, (kind, dict(kinds))
    for v in ("clean", "data", "parity", "unknown"):
        assert verdicts[v] >= 10, (v, dict(verdicts))
    assert 2 * differ >= STRIPE_CASES, differ


_STRIPE_SEEN = {}


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(STRIPE_CASES))
def test_random_stripe_checks(seed):
    """On one context: verify (flags), locate (verdicts, flags, nothing written), heal (verdicts,
    flags, the whole buffers against the definition's image), and verify again on the healed
    device buffers (flags only where the verdict was UNKNOWN).  Every call's label is the rule's,
    evaluated on the pointers the call really got."""
    import collections

    import torch

    from test_layout_contract import check, download, dptr, expected_form, upload
    from test_locate import UNKNOWN
    from test_stripe_layouts import family, stripe_labels

    c = _stripe_case(seed)
    k, m, S, nb, d, p = c["k"], c["m"], c["S"], c["nb"], c["d"], c["p"]
    ctx = (seed, k, m, S, nb, tuple(d), tuple(p), c["wpc1"], c["kinds"])
    st = torch.cuda.current_stream().cuda_stream
    dev = upload(torch, c["before"])
    args = (dptr(dev, d), d.rs, d.bs, dptr(dev, p), p.rs, p.bs, S, nb)
    form = expected_form(dptr(dev, d), d.rs, d.bs, dptr(dev, p), p.rs, p.bs, S)
    assert form == c["form"], ctx
    vlabel, llabel, hlabel = stripe_labels(k, m, form)

    def outputs():
        return (torch.full((nb + 2,), 0x5EED, dtype=torch.int32, device="cuda"),
                torch.full((nb * m + 2,), 0x5EED, dtype=torch.int32, device="cuda"))

    def results(cul, bad):
        cul, bad = cul.cpu().numpy(), bad.cpu().numpy()
        assert (cul[nb:] == 0x5EED).all() and (bad[nb * m:] == 0x5EED).all(), ctx
        return cul[:nb], bad[:nb * m].reshape(nb, m) != 0

    with rsmi.Codec(k, m) as cd:
        if c["wpc1"]:
            cd.set_option("waves_per_cu", 1)
        cul, bad = outputs()
        cd.verify_batch_dev(*args, bad.data_ptr(), st)
        torch.cuda.synchronize()
        assert cd.last_kernel() == vlabel, (cd.last_kernel(), vlabel) + ctx
        assert np.array_equal(results(cul, bad)[1], c["flags"]), ctx

        cul, bad = outputs()
        cd.locate_batch_dev(*args, cul.data_ptr(), bad.data_ptr(), st)
        torch.cuda.synchronize()
        assert cd.last_kernel() == llabel, (cd.last_kernel(), llabel) + ctx
        got, gbad = results(cul, bad)
        assert np.array_equal(got, c["verdicts"]), ctx + (got.tolist(), c["verdicts"].tolist())
        assert np.array_equal(gbad, c["flags"]), ctx
        check(download(dev), c["before"], ctx + ("locate wrote to the shards",))

        cul, bad = outputs()
        vcul, vbad = outputs()
        cd.heal_batch_dev(*args, cul.data_ptr(), bad.data_ptr(), st)
        healed_by = cd.last_kernel()
        cd.verify_batch_dev(*args, vbad.data_ptr(), st)
        torch.cuda.synchronize()
        assert healed_by == hlabel, (healed_by, hlabel) + ctx
        assert cd.last_kernel() == vlabel, (cd.last_kernel(), vlabel) + ctx
        got, gbad = results(cul, bad)
        assert np.array_equal(got, c["verdicts"]), ctx + (got.tolist(), c["verdicts"].tolist())
        assert np.array_equal(gbad, c["flags"]), ctx
        check(download(dev), c["want"], ctx)
        after = results(vcul, vbad)[1]
        assert np.array_equal(after, c["image_flags"]), ctx + (after.tolist(),)
        assert np.array_equal(after.any(axis=1), c["verdicts"] == UNKNOWN), ctx
    _STRIPE_SEEN.setdefault("heal", collections.Counter())["m=1" if m == 1 else family(hlabel)] += 1
    _STRIPE.pop(seed, None)
    if seed == STRIPE_CASES - 1:
        print("\nstripe fuzz: heal calls run and asserted by label, per family:", dict(_STRIPE_SEEN["heal"]))


# ---------------------------------------------------------------- the mixed-batch reconstruct
# Seeded random mixed batches: every block draws its own loss count (0 .. m + 1) and rows, the
# batch draws shape, size, layout (test_mixed_layouts' one side through _stripe_side), required
# masks, data_only, waves_per_cu and the entry point.  Statuses and the whole buffer against
# test_mixed_reconstruct.definition, the label against test_mixed_layouts.expected_label on the
# pointer the call really got.
MIXED_CASES = 48
MIXED_SEED_BASE = 88000
MIXED_ENTRIES = ["dev", "dev-side-stream", "host-locked", "host-pageable", "host-upload"]
MIXED_ENTRY_P = [0.36, 0.28, 0.12, 0.12, 0.12]
MIXED_LAYOUT_P = [0.22, 0.22, 0.46, 0.1]    # over LAYOUTS: "odd" is the only UA layout with rs > S
MIXED_S_P = [0.08, 0.08, 0.08, 0.14, 0.3, 0.32]   # rows of several tiles: UA grids of 8 workgroups and more
MIXED_M_P = [1, 1, 1, 1, 1, 2, 2, 2, 3, 3, 3, 2, 2, 2, 2]   # over STRIPE_MS, before normalising
_MIXED = {}
_MIXED_DRAW = {}


def _mixed_draw(seed):
    """The parameters of a case: cheap, nothing of the oracle's."""
    if seed in _MIXED_DRAW:
        return _MIXED_DRAW[seed]
    from test_layout_contract import GUARD, Side
    from test_mixed_layouts import expected_form

    r = np.random.default_rng(MIXED_SEED_BASE + seed)
    k = int(r.choice(STRIPE_KS))
    m = int(r.choice(STRIPE_MS, p=np.array(MIXED_M_P) / float(sum(MIXED_M_P))))
    n = k + m
    S = int(r.choice([16, 17, 31, int(r.integers(1, 16)), int(r.integers(1, 5000)), int(r.integers(5000, 20001))],
                     p=MIXED_S_P))
    nb = int(r.integers(1, 65))
    entry = str(r.choice(MIXED_ENTRIES, p=MIXED_ENTRY_P))
    lay = str(r.choice(LAYOUTS, p=MIXED_LAYOUT_P))
    wpc1 = bool(r.integers(0, 4) == 0)
    # waves_per_cu = 1 leaves a 256-CU device 256 waves per launch: two such cases in three draw
    # long rows, many blocks and mostly one lost row, so that a class has more tiles than that and
    # the waves walk on (nb stays within 1..64)
    walk = wpc1 and bool(r.random() < 2.0 / 3)
    if walk:
        S, nb = int(r.integers(16000, 20001)), int(r.integers(48, 65))
    data_only = bool(r.random() < 0.35)
    present = np.ones((nb, n), dtype=bool)
    for b in range(nb):
        nl = 1 if walk and r.random() < 0.6 else int(r.integers(0, m + 2))
        present[b, r.choice(n, size=nl, replace=False)] = False
    required = (r.random(size=(nb, n)) < 0.6) if r.random() < 0.35 else None
    if entry.startswith("dev"):
        side = _stripe_side(lay, "x", n, S, nb, 0)
    else:  # host memory: rows at pitch S, a drawn block stride
        side = Side("x", 0, S, n * S + int(r.choice([0, int(r.integers(1, 40))])))
    # the layout launch_mixed sees: the caller's on the device and in page-locked memory, whole
    # blocks at pitch S in the staging of the other two
    seen = side if entry in ("dev", "dev-side-stream", "host-locked") else Side("x", 0, S, n * S)
    form = expected_form(GUARD + seen.off, seen.rs, seen.bs, S)   # from a 16-byte-aligned allocation
    d = dict(k=k, m=m, S=S, nb=nb, entry=entry, lay=lay, wpc1=wpc1, data_only=data_only, present=present,
             required=required, side=side, seen=seen, form=form, data_seed=int(r.integers(0, 2 ** 31)))
    _MIXED_DRAW[seed] = d
    return d


def _mixed_rows(d):
    from test_mixed_layouts import rows_rebuilt
    from test_mixed_reconstruct import wanted

    W = wanted(d["k"], d["present"], d["required"], d["data_only"])
    return W, rows_rebuilt(d["k"], d["present"], W)


def _mixed_case(seed):
    """The draw, the shards and the definition's answers, computed once per seed."""
    if seed in _MIXED:
        return _MIXED[seed]
    from test_mixed_reconstruct import definition, junk_unused_survivor, stored

    d = dict(_mixed_draw(seed))
    k, m, S, nb = d["k"], d["m"], d["S"], d["nb"]
    r = np.random.default_rng(d["data_seed"])
    data = r.integers(0, 256, size=(nb, k, S), dtype=np.uint8)
    sh = stored(np.concatenate([data, orc.encode_fast(k, m, data, threads=4)], axis=1), d["present"])
    junk_unused_survivor(k, sh, d["present"])
    W, rows = _mixed_rows(d)
    status, image = definition(k, m, sh, d["present"], W)
    d.update(sh=sh, W=W, rows=rows, status=status, image=image)
    _MIXED[seed] = d
    return d


def _mixed_grids(d, rows):
    """The workgroups of each class launch of an uncapped call, as launch_mixed sizes them."""
    cpb = (d["S"] + 15) // 16
    tpb = (cpb + 63) // 64
    return [(int((rows == mt).sum()) * tpb + 3) // 4 for mt in (1, 2, 3, 4) if (rows == mt).any()]


def test_mixed_generator_coverage():
    """The committed seed range reaches what the fuzz is there for (conditions on the generator,
    not measurements)."""
    import collections
    import os

    from test_kernel_matrix import KS
    from test_mixed_reconstruct import MIXED_CPP

    with open(MIXED_CPP) as f:
        src = " ".join(f.read().split())
    with open(os.path.join(os.path.dirname(MIXED_CPP), "rs_plan.hpp")) as f:
        plan = f.read()
    assert "const uint64_t cpb = (S + 15) / 16;" in src
    assert "const uint64_t tpb = (cpb + uint64_t(kWave) - 1) / uint64_t(kWave);" in src
    assert "constexpr int wpg = kFastWG / kWave;" in src
    assert "uint32_t ntiles = uint32_t(list[mt].size() * tpb);" in src
    assert ("const uint64_t wgs = std::min<uint64_t>((uint64_t(ntiles) + wpg - 1) / wpg, uint64_t(wg_cap));") in src
    assert "constexpr int kWave = 64;" in plan and "constexpr int kWG = 256;" in plan
    assert "constexpr int kFastWG = kWG;" in plan

    t = collections.Counter()
    class_blocks, class_cases = collections.Counter(), collections.Counter()
    for seed in range(MIXED_CASES):
        d = _mixed_draw(seed)
        k, m, S, nb, side, form = d["k"], d["m"], d["S"], d["nb"], d["side"], d["form"]
        n = k + m
        assert 1 <= nb <= 64 and side.rs >= S and side.bs >= n * side.rs
        W, rows = _mixed_rows(d)
        has_class = form != "generic" and k in KS
        work = rows > 0
        fast = work & (rows <= 4) & has_class
        for mt in (1, 2, 3, 4):
            cnt = int((fast & (rows == mt)).sum())
            class_blocks[mt] += cnt
            class_cases[mt] += cnt > 0
        t["three classes"] += len(set(rows[fast].tolist())) >= 3
        t["fallback: more than 4 rows"] += bool(has_class and (rows > 4).any())
        t["fallback: K without a kernel"] += bool(k not in KS and work.any())
        t["fallback: neither form"] += bool(form == "generic" and work.any())
        assert form != "generic" or S < 16
        t["fast and fallback"] += bool(fast.any() and (work & ~fast).any())
        few = (d["present"].sum(axis=1) < k) & W.any(axis=1)
        t["too few"] += bool(few.any())
        t["no work"] += bool((~W.any(axis=1)).any())
        t["required"] += d["required"] is not None
        t["data_only"] += d["data_only"]
        t["aligned"] += bool(form == "aligned" and work.any())
        t["UA, rs > S"] += bool(form == "ua" and d["seen"].rs > S and work.any())
        t["waves_per_cu = 1"] += d["wpc1"]
        # the cap of waves_per_cu = 1 on 256 CUs is 64 workgroups: a class launch with more tiles
        # than their 256 waves is walked
        walked = any(g > 64 for g in _mixed_grids(d, np.where(fast, rows, 0)))
        t["waves_per_cu = 1, walked"] += bool(d["wpc1"] and walked)
        t[d["entry"]] += 1
        if form == "ua" and fast.any() and not d["wpc1"]:
            grids = _mixed_grids(d, np.where(fast, rows, 0))
            t["UA grid % 8 == 0"] += any(g % 8 == 0 for g in grids)
            t["UA grid % 8 != 0"] += any(g % 8 != 0 for g in grids)
    print("\nmixed fuzz generator:", dict(t), "class blocks", dict(class_blocks), "class cases", dict(class_cases))
    for mt in (1, 2, 3, 4):
        assert class_blocks[mt] >= 10 and class_cases[mt] >= 5, (mt, dict(class_blocks), dict(class_cases))
    assert t["three classes"] >= 15, dict(t)
    for cause in ("more than 4 rows", "K without a kernel", "neither form"):
        assert t["fallback: " + cause] >= 3, (cause, dict(t))
    assert t["fast and fallback"] >= 3, dict(t)
    assert t["too few"] >= 8 and t["no work"] >= 8, dict(t)
    assert t["required"] >= 12 and t["data_only"] >= 12, dict(t)
    assert t["aligned"] >= 10 and t["UA, rs > S"] >= 10, dict(t)
    for entry in MIXED_ENTRIES:
        assert t[entry] >= 3, (entry, dict(t))
    assert t["UA grid % 8 == 0"] >= 3 and t["UA grid % 8 != 0"] >= 3, dict(t)
    assert t["waves_per_cu = 1, walked"] >= 3, dict(t)
    assert "if (c->opt_waves_per_cu > 0) wg_cap = std::max(1L, long(c->num_cu) * c->opt_waves_per_cu / wpg);" in src


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(MIXED_CASES))
def test_random_mixed_batches(seed):
    """One mixed call per case on a context of its own: the statuses, the whole buffer (guards,
    padding and gaps included) and the label, which is "" where no block has work."""
    import ctypes

    import torch

    from test_layout_contract import FILL_DATA, GUARD, put
    from test_mixed_layouts import buf_size, compare, expected_form, expected_label
    from test_mixed_reconstruct import u8

    d = _mixed_case(seed)
    k, m, S, nb, side, entry = d["k"], d["m"], d["S"], d["nb"], d["side"], d["entry"]
    n = k + m
    ctx = (seed, k, m, S, nb, entry, d["lay"], tuple(side), d["wpc1"], d["data_only"], d["required"] is not None)
    size = buf_size(side, n, S, nb)
    host = np.full(size, FILL_DATA, dtype=np.uint8)
    put({"x": host}, side, d["sh"])
    want = host.copy()
    put({"x": want}, side, d["image"])
    present, required = u8(d["present"]), None if d["required"] is None else u8(d["required"])
    L = rsmi.lib()
    pinned = None
    try:
        with rsmi.Codec(k, m) as c:
            if d["wpc1"]:
                c.set_option("waves_per_cu", 1)
            if entry.startswith("dev"):
                t = torch.from_numpy(host).cuda()
                assert t.data_ptr() % 16 == 0
                ptr = t.data_ptr() + GUARD + side.off
                form = expected_form(ptr, side.rs, side.bs, S)
                if entry == "dev":
                    got = c.reconstruct_mixed_batch_dev(ptr, side.rs, side.bs, S, nb, present, required, d["data_only"],
                                                        torch.cuda.current_stream().cuda_stream)
                else:
                    s = torch.cuda.Stream()
                    s.wait_stream(torch.cuda.current_stream())
                    got = c.reconstruct_mixed_batch_dev(ptr, side.rs, side.bs, S, nb, present, required, d["data_only"],
                                                        s.cuda_stream)
                torch.cuda.synchronize()
                out = t.cpu().numpy()
            else:
                if entry == "host-locked":
                    pinned = L.rsmi_host_alloc(size)
                    assert pinned and pinned % 16 == 0
                    out = np.ctypeslib.as_array((ctypes.c_uint8 * size).from_address(pinned))
                    out[:] = host
                    form = expected_form(pinned + GUARD, S, side.bs, S)
                else:
                    out = host.copy()
                    form = expected_form(0, S, n * S, S)
                    if entry == "host-upload":
                        c.set_option("small_call_bytes", 0)
                got = c.reconstruct_mixed_batch_host_ptr(out.ctypes.data + GUARD, side.bs, S, nb, present, required,
                                                         d["data_only"])
                out = out.copy()
            assert form == d["form"], ctx
            compare(got, out, c.last_kernel(), d["status"], want, expected_label(k, d["rows"], form) or "", ctx)
    finally:
        if pinned:
            L.rsmi_host_free(pinned)
    _MIXED.pop(seed, None)
