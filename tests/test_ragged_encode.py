"""rsmi_encode_ragged_batch_* on the GPU: one call over blocks that each have their own shard size
and their own rows, against oracle_lib.encode block by block.

Every buffer is compared whole against an image pre-filled with a sentinel (0xC3), so a write to
padding, to a gap, to a data row or past a row's S fails the case.  The legs:

  1  the seams in one call: the tile seam (1 024 bytes), the unit seam (4 096 bytes) and the UA
     last-window overlap, all aligned, all at pitch S, and the classes interleaved block by block
  2  independent halves: separate allocations with different strides and byte phases; parity below
     the data in one allocation
  3  RS(5,5) (two plan tiles), RS(7,2) and RS(20,4) (no rs_ragged_kernel: the fallback)
  4  equality with rsmi_encode_batch_dev on a batch of equal S
  5  waves_per_cu = 1 with 40 and with 1 280 blocks (the strided walk)
  6  launch_units_max set small: the segments, counted in split_launches
  7  the scratch grows and starts over on one stream, then three streams; past 32 caller streams
  8  stream order behind a gate, the descriptors overwritten the moment the call returns
  9  a data_off past 4 GiB
 10  the host paths: page-locked in place, pageable small, pageable past one chunk, mixed
 11  Erasure.encode_data_many
"""
import ctypes
import functools

import numpy as np
import pytest

import oracle_lib as orc

SENT = 0xC3
SEAMS = [1, 15, 16, 17, 31, 32, 1008, 1023, 1024, 1025, 1040, 4095, 4096, 4097, 4112, 5000]
RAGGED_KS = {1, 2, 3, 4, 5, 6, 8, 10, 12, 16}
ALIGNED, UA, FALLBACK = 0, 1, 2
UNIT_TILES = 4


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    rsmi = pytest.importorskip("rsmi")
    if not torch.cuda.is_available() or rsmi.device_count() == 0:
        pytest.skip("no GPU")
    return torch, rsmi


# ---------------------------------------------------------------- the reference, computed once
@functools.lru_cache(maxsize=None)
def stripe(k, m, S, v=0):
    """(data (k, S), parity (m, S)) of variant v of a block with shard size S; read-only."""
    data = orc.splitmix64_bytes(0xF11EDA6 ^ (S * 131 + v * 7919 + k), k * S).reshape(k, S)
    par = orc.encode(k, m, data)
    data.setflags(write=False)
    par.setflags(write=False)
    return data, par


def round16(x):
    return (x + 15) // 16 * 16


def ragged_label(K, MT, ua):
    return "rs_ragged_kernel<K=%d,MT=%d>%s" % (K, MT, ",UA" if ua else "")


class Batch:
    """A ragged batch over two byte images.  place() puts a block's rows into the images at the
    cursor of each half: kind "a": offsets and strides multiples of 16 with room for the last
    chunk; kind "u": the data rows at an odd phase, pitch S + extra."""

    def __init__(self, k, m, data_phase=0, parity_phase=0):
        self.k, self.m = k, m
        self.rows = []       # S, data_off, ds, parity_off, ps
        self.variant = []
        self.dcur, self.pcur = data_phase, parity_phase

    def add(self, S, doff, ds, poff, ps, v=0):
        self.rows.append([S, doff, ds, poff, ps])
        self.variant.append(v)
        self.dcur = max(self.dcur, doff + (self.k - 1) * ds + S)
        self.pcur = max(self.pcur, poff + (self.m - 1) * ps + S)

    def place(self, S, kind, v=0, gap=0, extra=0):
        if kind == "a":
            ds = ps = round16(S) + 16 * extra
            self.add(S, round16(self.dcur) + 16 * gap, ds, round16(self.pcur) + 16 * gap, ps, v)
        elif kind == "u":   # odd data phase, parity wherever the cursor stands
            self.add(S, round16(self.dcur) + 1 + 2 * (gap % 7), S + extra, self.pcur + gap, S + extra, v)
        else:               # "p": rows back to back at pitch S from the cursors as they stand
            bump = 1 if S % 16 == 0 and self.dcur % 16 == 0 and self.pcur % 16 == 0 else 0   # never aligned by accident
            self.add(S, self.dcur + bump, S, self.pcur, S, v)

    def blocks(self):
        return np.ascontiguousarray(np.array(self.rows, dtype=np.uint64).reshape(-1, 5))

    def images(self, tail=48):
        """(data image, parity image as stored, parity image as it must be after the call)."""
        k, m = self.k, self.m
        d = np.full(self.dcur + tail, SENT, dtype=np.uint8)
        p = np.full(self.pcur + tail, SENT, dtype=np.uint8)
        want = p.copy()
        for (S, doff, ds, poff, ps), v in zip(self.rows, self.variant):
            data, par = stripe(k, m, S, v)
            for c in range(k):
                d[doff + c * ds:doff + c * ds + S] = data[c]
            for j in range(m):
                want[poff + j * ps:poff + j * ps + S] = par[j]
        return d, p, want

    def classes(self, dbase, pbase):
        out = []
        for S, doff, ds, poff, ps in self.rows:
            al = all(x % 16 == 0 for x in (dbase + doff, pbase + poff, ds, ps)) and min(ds, ps) >= round16(S)
            out.append(FALLBACK if self.k not in RAGGED_KS or (not al and S < 16) else ALIGNED if al else UA)
        return out

    def units(self, dbase, pbase):
        return [0 if c == FALLBACK else ((r[0] + 1023) // 1024 + UNIT_TILES - 1) // UNIT_TILES
                for c, r in zip(self.classes(dbase, pbase), self.rows)]


def same_bytes(got, want, tag):
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError("%s: %d bytes differ, first at %d: got 0x%02x want 0x%02x" %
                             (tag, bad.size, bad[0], got[bad[0]], want[bad[0]]))


def expected_label(batch, classes):
    """The label of the call's last launch: the fallback's, else the UA class's, else the aligned."""
    k, m = batch.k, batch.m
    mt_last = (m - 1) % 4 + 1
    if FALLBACK in classes:
        return None
    return ragged_label(k, mt_last, UA in classes)


def run_dev(torch, c, batch, tag, label="auto", classes=None):
    """The device call on fresh copies of the batch's images; both buffers compared whole."""
    d_img, p_img, want = batch.images()
    d, p = torch.from_numpy(d_img).cuda(), torch.from_numpy(p_img).cuda()
    assert d.data_ptr() % 256 == 0 and p.data_ptr() % 256 == 0
    got_cls, got_tiles = c.encode_ragged_classify(d.data_ptr(), p.data_ptr(), batch.blocks())
    want_cls = batch.classes(0, 0)
    assert got_cls == want_cls, tag
    assert got_tiles == [0 if cl == FALLBACK else (r[0] + 1023) // 1024 for cl, r in zip(want_cls, batch.rows)], tag
    if classes is not None:
        assert set(want_cls) == set(classes), (tag, sorted(set(want_cls)))
    c.encode_ragged_batch_dev(d.data_ptr(), p.data_ptr(), batch.blocks(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    same_bytes(d.cpu().numpy(), d_img, str(tag) + ": the data rows")
    same_bytes(p.cpu().numpy(), want, str(tag) + ": the parity rows")
    if label == "auto":
        label = expected_label(batch, want_cls)
    if label is not None:
        assert c.last_kernel() == label, (tag, c.last_kernel(), label)


def seam_batch(k, m, mode, sizes=SEAMS, reps=1):
    b = Batch(k, m, *((1, 3) if mode == "pitch" else (0, 0)))
    for i, S in enumerate(list(sizes) * reps):
        kind = {"aligned": "a", "pitch": "p", "mixed": "au"[i % 2], "ua": "u"}[mode]
        b.place(S, kind, v=i % 3, gap=i % 3, extra=i % 2 if mode != "pitch" else 0)
    return b


# ---------------------------------------------------------------- 1: the seams in one call
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["aligned", "pitch", "mixed"])
@pytest.mark.parametrize("k,m", [(4, 2), (10, 4)])
def test_seams_in_one_call(gpu, k, m, mode):
    torch, rsmi = gpu
    want = {"aligned": {ALIGNED}, "pitch": {UA, FALLBACK}, "mixed": {ALIGNED, UA, FALLBACK}}[mode]
    with rsmi.Codec(k, m) as c:
        run_dev(torch, c, seam_batch(k, m, mode), (k, m, mode), classes=want)
        if mode == "mixed":   # the other interleaving: the classes change places
            b = Batch(k, m)
            for i, S in enumerate(SEAMS):
                b.place(S, "ua"[i % 2], v=(i + 1) % 3, gap=(i + 2) % 3)
            run_dev(torch, c, b, (k, m, "mixed, swapped"), classes=want)


# ---------------------------------------------------------------- 2: independent halves
@pytest.mark.gpu
@pytest.mark.parametrize("k,m", [(4, 2), (10, 4)])
def test_independent_halves(gpu, k, m):
    """Data and parity in separate allocations, each half with its own strides and phases: aligned
    data with unaligned parity, the reverse, both unaligned at different phases, both aligned with
    different strides.  Then one allocation with the parity rows below the data rows."""
    torch, rsmi = gpu
    b = Batch(k, m)
    for i, S in enumerate(SEAMS[2:] + [2047, 3000]):   # S >= 16: every block has a fast class
        form = i % 4
        doff, poff = round16(b.dcur) + 16, round16(b.pcur) + 32
        if form == 0:
            b.add(S, doff, round16(S) + 16, poff + 5, S + 3, i % 3)
        elif form == 1:
            b.add(S, doff + 9, S, poff, round16(S) + 32, i % 3)
        elif form == 2:
            b.add(S, doff + 3, S + 1, poff + 14, S + 6, i % 3)
        else:
            b.add(S, doff, round16(S) + 48, poff, round16(S), i % 3)
    with rsmi.Codec(k, m) as c:
        run_dev(torch, c, b, (k, m, "two allocations"), classes={ALIGNED, UA})
        # one allocation: [parity image | 64 bytes | data image], the parity base below the data base
        d_img, p_img, want = b.images()
        gap = round16(p_img.size) + 64 - p_img.size
        whole = np.concatenate([p_img, np.full(gap, SENT, dtype=np.uint8), d_img])
        expect = np.concatenate([want, np.full(gap, SENT, dtype=np.uint8), d_img])
        t = torch.from_numpy(whole).cuda()
        dbase = t.data_ptr() + p_img.size + gap
        assert t.data_ptr() < dbase and dbase % 16 == 0
        c.encode_ragged_batch_dev(dbase, t.data_ptr(), b.blocks(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        same_bytes(t.cpu().numpy(), expect, (k, m, "parity below the data"))


# ---------------------------------------------------------------- 3: two plan tiles; the fallback K
@pytest.mark.gpu
@pytest.mark.parametrize("k,m", [(5, 5), (7, 2), (20, 4)])
def test_plan_tiles_and_fallback_shapes(gpu, k, m):
    torch, rsmi = gpu
    sizes = [1, 15, 16, 17, 1023, 1025, 4096, 4097, 5000, 1040]
    with rsmi.Codec(k, m) as c:
        for mode in ("aligned", "pitch", "mixed"):
            b = seam_batch(k, m, mode, sizes)
            if k in RAGGED_KS:
                want = {"aligned": {ALIGNED}, "pitch": {UA, FALLBACK}, "mixed": {ALIGNED, UA, FALLBACK}}[mode]
            else:
                want = {FALLBACK}
            run_dev(torch, c, b, (k, m, mode), classes=want)
        if k == 5:   # RS(5,5): the second plan tile has one row
            run_dev(torch, c, seam_batch(k, m, "ua", [16, 1025, 4097]), (k, m, "ua"), label=ragged_label(5, 1, True))
            run_dev(torch, c, seam_batch(k, m, "aligned", [1, 1025]), (k, m, "a"), label=ragged_label(5, 1, False))


# ---------------------------------------------------------------- 4: the uniform call
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "ua"])
@pytest.mark.parametrize("k,m,S", [(10, 4, 1025), (4, 2, 4097), (16, 4, 1040), (5, 5, 17), (7, 2, 300)])
def test_equals_the_uniform_call(gpu, k, m, S, aligned):
    """A batch of equal S at uniform strides: the two buffers equal rsmi_encode_batch_dev's on a
    copy, byte for byte, padding and gaps included."""
    torch, rsmi = gpu
    nb = 7
    rs = round16(S) + 16 if aligned else S + 3
    off = 0 if aligned else 5
    b = Batch(k, m)
    for i in range(nb):
        b.add(S, off + i * (k * rs + 32), rs, off + i * (m * rs + 16), rs, i % 3)
    d_img, p_img, want = b.images()
    stream = torch.cuda.current_stream().cuda_stream
    with rsmi.Codec(k, m) as c:
        d1, p1 = torch.from_numpy(d_img).cuda(), torch.from_numpy(p_img).cuda()
        d2, p2 = torch.from_numpy(d_img).cuda(), torch.from_numpy(p_img).cuda()
        c.encode_batch_dev(d1.data_ptr() + off, rs, k * rs + 32, p1.data_ptr() + off, rs, m * rs + 16, S, nb, stream)
        uniform_label = c.last_kernel()
        c.encode_ragged_batch_dev(d2.data_ptr(), p2.data_ptr(), b.blocks(), stream)
        torch.cuda.synchronize()
        assert (c.last_kernel() != uniform_label) == (k in RAGGED_KS)   # the fallback is the uniform launch
        same_bytes(p2.cpu().numpy(), p1.cpu().numpy(), "parity against the uniform call")
        same_bytes(d2.cpu().numpy(), d1.cpu().numpy(), "data against the uniform call")
        same_bytes(p2.cpu().numpy(), want, "parity against the oracle")


# ---------------------------------------------------------------- 5: the strided walk
@pytest.mark.gpu
@pytest.mark.parametrize("reps", [40, 1280], ids=["40", "1280"])
def test_waves_per_cu_1(gpu, reps):
    """waves_per_cu = 1 caps the grid at a quarter of a workgroup per CU: 40 blocks stay below it
    on a large device, 1 280 blocks (about 1 500 units a class) make the workgroups stride."""
    torch, rsmi = gpu
    k, m = 10, 4
    sizes = [SEAMS[(i * 7) % len(SEAMS)] for i in range(reps)]
    with rsmi.Codec(k, m) as c:
        c.set_option("waves_per_cu", 1)
        for mode in ("aligned", "mixed"):
            run_dev(torch, c, seam_batch(k, m, mode, sizes), ("waves_per_cu", reps, mode))


# ---------------------------------------------------------------- 6: the segments
def segment_launches(units, classes, cap, plan_tiles):
    """launch_ragged's cut, restated: fast blocks join a segment while its units stay within the
    cap (a block of more units is a segment of its own); fallback blocks ride along (their
    launch_plan launches are the byte-granular kernel's, which split_launches does not count: the
    shapes with a coding kernel are the shapes with an rs_ragged_kernel); a segment launches once
    per non-empty class and tile."""
    launches, seg_units, seg_classes = 0, 0, set()
    for u, cl in zip(units, classes):
        if cl == FALLBACK:
            continue
        if seg_classes and seg_units + u > cap:
            launches += len(seg_classes) * plan_tiles
            seg_units, seg_classes = 0, set()
        seg_units += u
        seg_classes.add(cl)
    return launches + len(seg_classes) * plan_tiles


@pytest.mark.gpu
@pytest.mark.parametrize("k,m,cap", [(10, 4, 1), (10, 4, 3), (10, 4, 7), (5, 5, 4)])
def test_launch_units_max_small(gpu, k, m, cap):
    torch, rsmi = gpu
    b = seam_batch(k, m, "mixed", SEAMS + [9000, 20000, 16, 17])   # 9 000: 3 units, 20 000: 5 units
    classes, units = b.classes(0, 0), b.units(0, 0)
    tiles = (m + 3) // 4
    assert max(units) == 5 and sum(units) > 3 * cap
    with rsmi.Codec(k, m) as c:
        before = c.stat("split_launches")
        run_dev(torch, c, b, (k, m, "default cap"))
        assert c.stat("split_launches") - before == segment_launches(units, classes, (1 << 24) - 1, tiles)
        c.set_option("launch_units_max", cap)
        before = c.stat("split_launches")
        run_dev(torch, c, b, (k, m, "cap", cap))
        want = segment_launches(units, classes, cap, tiles)
        assert c.stat("split_launches") - before == want > 3 * tiles, (cap, want)
        c.set_option("launch_units_max", 0)


# ---------------------------------------------------------------- 7: the scratch
def tiled_batch(k, m, nb, S=16):
    """nb aligned blocks of S bytes back to back, three variants in turn: (batch, images)."""
    b = Batch(k, m)
    P = round16(S)
    rows = np.zeros((nb, 5), dtype=np.uint64)
    i = np.arange(nb, dtype=np.uint64)
    rows[:, 0], rows[:, 1], rows[:, 2] = S, i * np.uint64(k * P), P
    rows[:, 3], rows[:, 4] = i * np.uint64(m * P), P
    d = np.full((nb, k, P), SENT, dtype=np.uint8)
    p = np.full((nb, m, P), SENT, dtype=np.uint8)
    want = p.copy()
    for v in range(3):
        data, par = stripe(k, m, S, v)
        d[v::3, :, :S] = data
        want[v::3, :, :S] = par
    return rows, d.reshape(-1), p.reshape(-1), want.reshape(-1)


@pytest.mark.gpu
def test_scratch_regrow_and_streams(gpu):
    """One context, RS(4,2), no host sync inside a round: three small calls, then one whose
    descriptors and units (72 bytes a block) outgrow the scratch's first size (1 MiB: 20 000
    blocks), the same again (it no longer fits behind the first: the scratch starts over), two
    small ones; then the same round on each of three more streams.  Every call has its own parity
    buffer, compared after the round."""
    torch, rsmi = gpu
    k, m = 4, 2
    small, big = tiled_batch(k, m, 3000), tiled_batch(k, m, 20000)
    assert big[0].shape[0] * 72 > (1 << 20) > small[0].shape[0] * 72 * 3
    with rsmi.Codec(k, m) as c:
        for stream in [torch.cuda.current_stream()] + [torch.cuda.Stream() for _ in range(3)]:
            with torch.cuda.stream(stream):
                outs = []
                for rows, d_img, p_img, want in (small, small, small, big, big, small, small):
                    d, p = torch.from_numpy(d_img).cuda(), torch.from_numpy(p_img).cuda()
                    torch.cuda.current_stream().synchronize()   # the uploads; the calls below do not wait
                    outs.append((d, p, d_img, want))
                for (d, p, _, _), (rows, _, _, _) in zip(outs, (small, small, small, big, big, small, small)):
                    c.encode_ragged_batch_dev(d.data_ptr(), p.data_ptr(), rows, stream.cuda_stream)
                    assert c.last_kernel() == ragged_label(k, m, False)
            torch.cuda.synchronize()
            for i, (d, p, d_img, want) in enumerate(outs):
                same_bytes(p.cpu().numpy(), want, "call %d: parity" % i)
                same_bytes(d.cpu().numpy(), d_img, "call %d: data" % i)


@pytest.mark.gpu
def test_past_32_caller_streams(gpu):
    """One Codec(10, 4), one ragged call on each of 40 distinct streams, then the same over the
    streams in reverse, with no host sync between the calls: the scratch map drains the device
    and frees every stream's scratch on the way, twice.  All 80 parity buffers against the oracle."""
    from test_stream_order import _hip_runtime

    torch, rsmi = gpu
    k, m, PAST = 10, 4, 40
    streams, seen = [], set()

    def add(s):
        if s.cuda_stream not in seen:
            seen.add(s.cuda_stream)
            streams.append(s)

    add(torch.cuda.current_stream())
    add(torch.cuda.ExternalStream(0))
    for prio in (0, -1):
        for _ in range(64):
            add(torch.cuda.Stream(priority=prio))
    hip, own = None, []
    try:
        if len(streams) < PAST:
            hip = _hip_runtime()
            hip.hipStreamCreateWithFlags.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
            hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
            while len(streams) < PAST:
                h = ctypes.c_void_p()
                assert hip.hipStreamCreateWithFlags(ctypes.byref(h), 1) == 0  # hipStreamNonBlocking
                own.append(h)
                add(torch.cuda.ExternalStream(h.value))
        handles = [s.cuda_stream for s in streams[:PAST]]
        assert len(set(handles)) == PAST > 32
        variants = [seam_batch(k, m, mode, SEAMS[4:12]) for mode in ("aligned", "mixed", "ua")]
        images = [b.images() for b in variants]
        with rsmi.Codec(k, m) as c:
            warm = images[0]
            d0, p0 = torch.from_numpy(warm[0]).cuda(), torch.from_numpy(warm[1]).cuda()
            c.encode_ragged_batch_dev(d0.data_ptr(), p0.data_ptr(), variants[0].blocks(), handles[0])
            torch.cuda.synchronize()
            calls = []
            for i, h in enumerate(handles + handles[::-1]):
                d_img, p_img, want = images[i % 3]
                calls.append((torch.from_numpy(d_img).cuda(), torch.from_numpy(p_img).cuda(), i % 3, h))
            torch.cuda.synchronize()
            for d, p, v, h in calls:
                c.encode_ragged_batch_dev(d.data_ptr(), p.data_ptr(), variants[v].blocks(), h)
            torch.cuda.synchronize()
            for i, (d, p, v, h) in enumerate(calls):
                same_bytes(p.cpu().numpy(), images[v][2], "call %d" % i)
                same_bytes(d.cpu().numpy(), images[v][0], "call %d: data" % i)
    finally:
        torch.cuda.synchronize()
        for h in own:
            hip.hipStreamDestroy(h)


# ---------------------------------------------------------------- 8: stream order
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["aligned", "mixed"])
def test_stream_order_behind_a_gate(gpu, mode):
    """On a side stream behind a device-side delay: the data rows are produced in stream order
    (copied over a poisoned buffer), two ragged calls follow, each one's descriptor array
    overwritten the moment it returns, and a consumer clones the parity and refills it.  No host
    sync before the end; the gate is still closed when the calls have returned."""
    from test_stream_order import Gate

    torch, rsmi = gpu
    gate = Gate(torch)
    k, m = 10, 4
    bA, bB = seam_batch(k, m, mode), seam_batch(k, m, mode, SEAMS[::-1])
    imgA, imgB = bA.images(), bB.images()
    with rsmi.Codec(k, m) as c:
        bufs = []
        for b, (d_img, p_img, want) in ((bA, imgA), (bB, imgB)):
            src = torch.from_numpy(d_img).pin_memory()
            d = torch.full((d_img.size,), 0xEE, dtype=torch.uint8, device="cuda")
            p = torch.from_numpy(p_img).cuda()
            bufs.append((b.blocks().copy(), src, d, p))
        # plans, scratch and the allocator's blocks at their final sizes before the gate closes
        for rows, src, d, p in bufs:
            c.encode_ragged_batch_dev(d.data_ptr(), p.data_ptr(), rows, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for (rows, src, d, p), img in zip(bufs, (imgA, imgB)):
            p.copy_(torch.from_numpy(img[1]))
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        clones = []
        with torch.cuda.stream(side):
            gate()
            for rows, src, d, p in bufs:
                d.copy_(src, non_blocking=True)
                c.encode_ragged_batch_dev(d.data_ptr(), p.data_ptr(), (rows.ctypes.data, rows.shape[0]), side.cuda_stream)
                rows[:] = np.uint64(0xDEADBEEFDEADBEEF)
                clones.append(p.clone())
                p.fill_(0x33)
            assert not side.query(), "the gate opened before the calls were queued: nothing was ordered"
        torch.cuda.synchronize()
        for i, (cl, img, (rows, src, d, p)) in enumerate(zip(clones, (imgA, imgB), bufs)):
            same_bytes(cl.cpu().numpy(), img[2], "call %d: parity" % i)
            same_bytes(d.cpu().numpy(), img[0], "call %d: data" % i)
            assert bool((p == 0x33).all()), "a launch ran late"


# ---------------------------------------------------------------- 9: far offsets
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "ua"])
def test_data_off_past_4gib(gpu, aligned):
    """One block's data rows lie past 4 GiB from the data base (and its parity past 4 GiB from the
    parity base): the descriptors' 64-bit offsets survive.  The far rows are written and read on
    the device only; the buffer's first and last MiB are compared whole."""
    torch, rsmi = gpu
    k, m = 4, 2
    FAR = (1 << 32) + 4096 + (0 if aligned else 7)
    near = Batch(k, m)
    for i, S in enumerate([1025, 17, 4097]):
        near.place(S, "a" if aligned else "u", v=i)
    S = 1040 if aligned else 1031
    rs = round16(S) if aligned else S
    data, par = stripe(k, m, S, 1)
    span = FAR + (k + m) * rs + 64
    free, _ = torch.cuda.mem_get_info()
    if free < 2 * span + (1 << 28):
        pytest.fail("not enough free device memory for a buffer past 4 GiB: %d" % free)
    d_img, p_img, want = near.images()
    with rsmi.Codec(k, m) as c:
        D = torch.empty(span, dtype=torch.uint8, device="cuda")
        P = torch.empty(span, dtype=torch.uint8, device="cuda")
        for T, img in ((D, d_img), (P, p_img)):
            T[:img.size].copy_(torch.from_numpy(img))
            T[FAR - 64:].fill_(SENT)
        for r in range(k):
            D[FAR + r * rs:FAR + r * rs + S].copy_(torch.from_numpy(data[r].copy()))
        far_data = D[FAR - 64:].clone()
        rows = np.concatenate([near.blocks(), np.array([[S, FAR, rs, FAR, rs]], dtype=np.uint64)])
        c.encode_ragged_batch_dev(D.data_ptr(), P.data_ptr(), rows, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        same_bytes(P[:p_img.size].cpu().numpy(), want, "near parity")
        same_bytes(D[:d_img.size].cpu().numpy(), d_img, "near data")
        tail = np.full(span - (FAR - 64), SENT, dtype=np.uint8)
        for j in range(m):
            tail[64 + j * rs:64 + j * rs + S] = par[j]
        same_bytes(P[FAR - 64:].cpu().numpy(), tail, "far parity")
        assert torch.equal(D[FAR - 64:], far_data), "far data rows were written"
        del D, P, far_data
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- 10: the host paths
def run_host(torch, rsmi, c, batch, pin_data, pin_parity, tag):
    d_img, p_img, want = batch.images()
    L = rsmi.lib()
    ptrs = []
    try:
        views = []
        for img, pin in ((d_img, pin_data), (p_img, pin_parity)):
            if pin:
                ptr = L.rsmi_host_alloc(img.size)
                assert ptr
                ptrs.append(ptr)
                v = np.ctypeslib.as_array((ctypes.c_uint8 * img.size).from_address(ptr))
                v[:] = img
            else:
                v = img.copy()
            views.append(v)
        c.encode_ragged_batch_host_ptr(views[0].ctypes.data, views[1].ctypes.data, batch.blocks())
        same_bytes(views[0], d_img, str(tag) + ": the data rows")
        same_bytes(views[1], want, str(tag) + ": the parity rows")
    finally:
        for ptr in ptrs:
            L.rsmi_host_free(ptr)


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", [(10, 4), (5, 5), (7, 2)])
def test_host_paths(gpu, k, m):
    torch, rsmi = gpu
    with rsmi.Codec(k, m) as c:
        for mode in ("aligned", "pitch", "mixed"):
            b = seam_batch(k, m, mode)
            run_host(torch, rsmi, c, b, True, True, (k, m, mode, "page-locked in place"))
            if k in RAGGED_KS:
                want = ragged_label(k, (m - 1) % 4 + 1, mode != "aligned")
                if mode == "aligned":
                    assert c.last_kernel() == want
            run_host(torch, rsmi, c, b, False, False, (k, m, mode, "pageable, one chunk"))
            run_host(torch, rsmi, c, b, True, False, (k, m, mode, "data page-locked, parity pageable"))
            run_host(torch, rsmi, c, b, False, True, (k, m, mode, "data pageable, parity page-locked"))
        # past one chunk: small_call_bytes below the batch's rows, and below one block's
        c.set_option("small_call_bytes", 40000)
        b = seam_batch(k, m, "mixed", SEAMS, reps=2)
        assert sum((k + m) * round16(r[0]) for r in b.rows) > 8 * 40000 and (k + m) * 5008 > 40000
        run_host(torch, rsmi, c, b, False, False, (k, m, "pageable past one chunk"))
        run_host(torch, rsmi, c, b, False, True, (k, m, "mixed memory past one chunk"))
        c.set_option("zero_copy", 0)   # page-locked memory through the staging as well
        run_host(torch, rsmi, c, b, True, True, (k, m, "zero_copy 0"))


# ---------------------------------------------------------------- 11: Erasure.encode_data_many
@pytest.mark.gpu
@pytest.mark.parametrize("k,m", [(10, 4), (4, 2), (7, 2)])
def test_encode_data_many(gpu, k, m):
    torch, rsmi = gpu
    e = rsmi.NewErasure(k, m, 262144)
    lens = [1, 6, 4099, 262144, k * 16, 0, k * 16 + 1, 1, 0]
    blocks = [orc.splitmix64_bytes(1000 + i, n).tobytes() for i, n in enumerate(lens)]
    got = e.encode_data_many(blocks)
    want = [e.encode_data(b) for b in blocks]
    assert got == want
    assert got[5] == [None] * (k + m) and all(isinstance(x, bytes) for x in got[0])
    for b, shards in zip(blocks, got):   # and against the oracle's Split + Encode
        if b:
            sh = orc.split(k, m, b)
            sh[k:] = orc.encode(k, m, np.ascontiguousarray(sh[:k]))
            assert [bytes(x) for x in sh] == shards
    assert e.encode_data_many([]) == [] and e.encode_data_many([b""]) == [[None] * (k + m)]
