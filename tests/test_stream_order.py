"""The device entry points' stream order, without a host sync to hide behind.

include/rsmi.h promises that every *_dev entry point is stream-ordered and does not sync.  The
other GPU modules drain the device around every call, so a launch, memset or combine pass on the
wrong stream, or host-side state rewritten while an earlier launch still needs it, reads and
writes the same bytes as a correct one.  Here every call is queued on a side stream behind a
device-side delay (the gate), between a producer and a consumer that exist only in that stream:

  1. the buffers are poisoned (0xEE data, 0xDEAD raw outputs) and the device drained;
  2. on the side stream: torch.cuda._sleep of about 50 ms, then event e1;
  3. producer, behind the delay: the real input is copied from page-locked memory over the
     poisoned buffer, and the raw outputs are poisoned once more in stream order (a memset or a
     combine that ran early on another stream is then overwritten, not mistaken for the result);
  4. the library call or calls on that stream;
  5. consumer: the buffers are cloned, then filled with 0x33 / -1;
  6. e1 has not completed when the calls have returned (they did not wait; without this the
     case could not fail);
  7. after the stream is drained the clones equal the expected whole buffers (guards and padding
     included) and the oracle's checksums, and the buffers still hold the consumer's fill (a
     library launch that ran late elsewhere would have written over it).

Each case runs once ungated first, on the same Codec and stream, which builds plans, tables,
scratch and the allocator's blocks at their final sizes.  Everything is bit-exact against
oracle_lib and zlib: there are no tolerances.

Leg A: every device entry point, each case on two side streams in turn.  Leg B: back-to-back calls with nothing drained between them.
Leg C: scratch growth behind pending work.  Leg D: two streams interleaved from one thread.
Leg E: past the 32 caller streams whose scratch a context keeps.  Leg F (no gate): all-0xFF,
all-zero and single-bit rows for the two standalone CRC rows passes.
"""
import ctypes
import os
import re
import time
import zlib

import numpy as np
import pytest

import oracle_lib as orc
from test_kernel_matrix import Layout, fast_label, fused_label, fused_units, generic_label

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORE_CPP = os.path.join(ROOT, "filedag-storage_amd", "csrc", "rsmi_core.cpp")

M32 = 0xFFFFFFFF
POISON_D, POISON_RAW, FILL_D, FILL_RAW = 0xEE, 0xDEAD, 0x33, -1
GATE_MS, GATE_MAX_MS = 50.0, 100.0
KEPT_STREAMS = 32   # crc_scratch() evicts at stream_scratch.size() >= 32 (pinned by the CPU leg)
WALL = {}


def raw32(data: bytes) -> int:
    """R32(D) from zlib, as in test_crc32.py."""
    return ~zlib.crc32(data, M32) & M32


# ---------------------------------------------------------------- CPU leg: the eviction threshold
def test_eviction_threshold_matches_source():
    """crc_scratch() in rsmi_core.cpp drains the device and frees every caller stream's scratch
    once it keeps 32 of them: Leg E's 40 streams stay beyond that."""
    with open(CORE_CPP) as f:
        src = f.read()
    body = src[src.index("CrcScratch& crc_scratch("):src.index("int reserve_on(")]
    assert re.findall(r"stream_scratch\.size\(\)\s*>=\s*(\d+)", body) == [str(KEPT_STREAMS)]
    assert "hipDeviceSynchronize" in body and "stream_scratch.clear()" in body
    assert E_STREAMS > KEPT_STREAMS


# ---------------------------------------------------------------- GPU plumbing
class Gate:
    """The stream-ordered delay: torch.cuda._sleep, calibrated once to about GATE_MS and never
    longer than GATE_MAX_MS."""

    def __init__(self, torch):
        self.torch = torch
        probe = 1000000
        torch.cuda._sleep(probe)  # load the kernel
        ms = self._time(probe)
        assert ms > 0.01, "torch.cuda._sleep(%d) took %.4f ms: unusable as a delay" % (probe, ms)
        self.cycles = int(probe * GATE_MS / ms)
        self.ms = self._time(self.cycles)
        if self.ms > GATE_MAX_MS * 0.9:  # the probe ran at another clock: scale down once
            self.cycles = int(self.cycles * GATE_MS / self.ms)
            self.ms = self._time(self.cycles)
        assert 10.0 <= self.ms <= GATE_MAX_MS, self.ms

    def _time(self, cycles):
        torch = self.torch
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        torch.cuda._sleep(cycles)
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def __call__(self):
        self.torch.cuda._sleep(self.cycles)


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    rsmi = pytest.importorskip("rsmi")
    if not torch.cuda.is_available() or rsmi.device_count() == 0:
        pytest.skip("no GPU")
    gate = Gate(torch)
    print("\nstream order: gate of %d cycles = %.1f ms" % (gate.cycles, gate.ms))
    yield torch, rsmi, gate
    print("\nstream order: wall seconds per leg:", ", ".join("%s %.2f" % kv for kv in sorted(WALL.items())))


class _leg:
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.t0 = time.perf_counter()

    def __exit__(self, *a):
        WALL[self.name] = WALL.get(self.name, 0.0) + time.perf_counter() - self.t0


class Bytes:
    """A guarded byte buffer on the device, its input in page-locked memory and the whole
    buffer expected after the call."""
    poison, fillv = POISON_D, FILL_D

    def __init__(self, torch, inp, want):
        self.inp = torch.from_numpy(inp.copy()).pin_memory()
        self.want = want
        self.dev = torch.empty(inp.size, dtype=torch.uint8, device="cuda")

    def check(self, got, ctx):
        assert np.array_equal(got, self.want), ctx


class Raw:
    """A raw checksum output (uint32 slots): no input; check(values as int64, ctx)."""
    poison, fillv = POISON_RAW, FILL_RAW
    inp = None

    def __init__(self, torch, shape, check):
        self.dev = torch.empty(shape, dtype=torch.int32, device="cuda")
        self._check = check

    def check(self, got, ctx):
        self._check(got.astype(np.int64) & M32, ctx)


class Call:
    def __init__(self, name, codec, bufs, fn, label=None):
        self.name, self.codec, self.bufs, self.fn, self.label = name, codec, bufs, fn, label


def run_plan(torch, gate, plan, gated, must_not_wait=True, rendezvous=False):
    """plan: [(stream, Call)] in issue order.  Steps 1 to 7 of the module docstring, with one gate
    at the head of every distinct stream when gated.  rendezvous (several streams): every producer
    is queued first, then each stream waits for the producers of all the others, so the streams
    start their library launches together and those overlap.  Returns {stream: e1.query()} as
    read after the last call and the consumer were queued."""
    streams = []
    for st, _ in plan:
        if all(st is not s for s in streams):
            streams.append(st)
    bufs = [b for _, c in plan for b in c.bufs]
    for b in bufs:
        b.dev.fill_(b.poison)
    torch.cuda.synchronize()
    e1 = {}
    if gated:
        for st in streams:
            with torch.cuda.stream(st):
                gate()
                e1[id(st)] = torch.cuda.Event()
                e1[id(st)].record()

    def produce(c):
        for b in c.bufs:
            if b.inp is not None:
                b.dev.copy_(b.inp, non_blocking=True)
            else:
                b.dev.fill_(b.poison)

    if rendezvous:
        for st, c in plan:
            with torch.cuda.stream(st):
                produce(c)
        ready = []
        for st in streams:
            ready.append(torch.cuda.Event())
            ready[-1].record(st)
        for st in streams:
            for ev in ready:
                st.wait_event(ev)
    for st, c in plan:
        with torch.cuda.stream(st):
            if not rendezvous:
                produce(c)
            c.fn(st.cuda_stream)
        if c.label is not None:
            assert c.codec.last_kernel() == c.label, (c.name, c.codec.last_kernel(), c.label)
    snaps = []
    for st, c in plan:  # the consumer
        with torch.cuda.stream(st):
            snaps.append([b.dev.clone() for b in c.bufs])
            for b in c.bufs:
                b.dev.fill_(b.fillv)
    done = {k: e.query() for k, e in e1.items()}
    if gated and must_not_wait:
        assert not any(done.values()), "a call waited for the stream: the delay had ended when it returned"
    for st in streams:
        st.synchronize()
    for (st, c), sn in zip(plan, snaps):
        for i, b in enumerate(c.bufs):
            b.check(sn[i].cpu().numpy(), (c.name, i, "gated" if gated else "warm"))
            left = b.dev.cpu().numpy()
            assert (left == (b.fillv & 0xFF if left.dtype == np.uint8 else b.fillv)).all(), \
                (c.name, i, "written after the consumer's fill")
    del snaps
    return done


def warm_then_gated(torch, gate, plan, rendezvous=False):
    run_plan(torch, gate, plan, gated=False, rendezvous=rendezvous)
    return run_plan(torch, gate, plan, gated=True, rendezvous=rendezvous)


# ---------------------------------------------------------------- call builders
def _rows_data(rng, nb, K, S):
    return rng.integers(0, 256, size=(nb, K, S), dtype=np.uint8)


def _full(K, MT, data):
    return np.concatenate([data, orc.encode_fast(K, MT, data, threads=4)], axis=1)


def _layout(rsmi, n, S, nb, mode):
    """aligned: recommended_pitch(S) from offset 0; ua: pitch S + 3 from offset 7; split: pitch S
    from offset 1 (test_kernel_matrix.Layout: guard bytes all round)."""
    if mode == "split":
        return Layout(rsmi, n, S, nb, True, off=1, rs=S)
    return Layout(rsmi, n, S, nb, mode == "ua")


def _raw16_check(rsmi, want_r, S):
    """want_r[b][i] = crc16_ibm(row); slots past len(want_r[b]) keep the poison."""
    def check(r, ctx):
        for b in range(len(want_r)):
            for i in range(r.shape[1]):
                if i >= len(want_r[b]):
                    assert r[b, i] == POISON_RAW, ctx + (b, i)
                    continue
                assert r[b, i] < 0x10000, ctx + (b, i)
                assert rsmi.crc16_entry(b"", int(r[b, i]), S) == want_r[b][i], ctx + (b, i)
    return check


def _raw32_check(want_r):
    def check(r, ctx):
        for b in range(len(want_r)):
            for i in range(r.shape[1]):
                assert r[b, i] == (want_r[b][i] if i < len(want_r[b]) else POISON_RAW), ctx + (b, i)
    return check


def encode_call(torch, rsmi, c, S, nb, mode, rng, label, crc=False, option=None):
    """rsmi_encode_batch_dev / _crc of the Codec's RS(k, m); option: (key, value) set just before
    the call (an option changed between two queued launches)."""
    K, MT, n = c.k, c.m, c.n
    lay = _layout(rsmi, n, S, nb, mode)
    full = _full(K, MT, _rows_data(rng, nb, K, S))
    inp = lay.buffer(0x5A)
    lay.rows(inp)[:, :K] = full[:, :K]
    want = inp.copy()
    lay.rows(want)[:] = full
    d = Bytes(torch, inp, want)
    base = d.dev.data_ptr() + lay.off
    bufs = [d]
    if crc:
        raw = Raw(torch, (nb, n), _raw16_check(rsmi, [[orc.crc16_ibm(r.tobytes()) for r in blk] for blk in full], S))
        bufs.append(raw)

    def fn(h):
        if option:
            c.set_option(*option)
        if crc:
            c.encode_batch_dev_crc(base, lay.rs, lay.bs, base + K * lay.rs, lay.rs, lay.bs, S, nb,
                                   raw.dev.data_ptr(), h)
        else:
            c.encode_batch_dev(base, lay.rs, lay.bs, base + K * lay.rs, lay.rs, lay.bs, S, nb, h)

    return Call(("encode_crc" if crc else "encode", K, MT, S, nb, mode, option), c, bufs, fn, label)


def reconstruct_call(torch, rsmi, c, S, nb, mode, rng, lost, label, data_only=False, required=None):
    """rsmi_reconstruct_batch_dev in place, or rsmi_reconstruct_rows_batch_dev when required is
    given; lost rows hold 0xEE, and those not rebuilt must keep it."""
    K, MT, n = c.k, c.m, c.n
    lay = _layout(rsmi, n, S, nb, mode)
    full = _full(K, MT, _rows_data(rng, nb, K, S))
    present = [i not in lost for i in range(n)]
    inp = lay.buffer(0x5A)
    lay.rows(inp)[:] = full
    lay.rows(inp)[:, lost] = 0xEE
    for b in range(nb):  # the oracle's rebuild of every lost row is the encode's input and output
        rc, sh = orc.reconstruct(K, MT, np.ascontiguousarray(lay.rows(inp)[b]), present, False)
        assert rc == 0 and np.array_equal(sh, full[b])
    if required is not None:
        rebuilt = [i for i in lost if i in required]
    else:
        rebuilt = [i for i in lost if i < K or not data_only]
    want = inp.copy()
    lay.rows(want)[:, rebuilt] = full[:, rebuilt]
    d = Bytes(torch, inp, want)
    base = d.dev.data_ptr() + lay.off

    def fn(h):
        if required is not None:
            c.reconstruct_rows_batch_dev(base, lay.rs, lay.bs, S, nb, present, [i in required for i in range(n)], h)
        else:
            c.reconstruct_batch_dev(base, lay.rs, lay.bs, S, nb, present, data_only, h)

    return Call(("reconstruct", K, MT, S, nb, mode, tuple(lost), data_only, required), c, [d], fn, label)


def crc_rows_call(torch, rsmi, c, bits, fold, S, nb, aligned, rows):
    """rsmi_crc16_rows_dev / rsmi_crc32_rows_dev over rows (nb, nrows, S) at recommended_pitch(S)
    from offset 0, or at pitch S + 3 from offset 5; output stride nrows + 1: the extra slot keeps
    its poison.  fold: the option crc16_fold / crc32_fold, set just before the call."""
    nrows = rows.shape[1]
    pitch, off = (rsmi.recommended_pitch(S), 0) if aligned else (S + 3, 5)
    bs = nrows * pitch
    inp = np.full(off + nb * bs + 32, 0x5A, dtype=np.uint8)
    np.lib.stride_tricks.as_strided(inp[off:], shape=(nb, nrows, S), strides=(bs, pitch, 1))[:] = rows
    d = Bytes(torch, inp, inp.copy())
    if bits == 16:
        check = _raw16_check(rsmi, [[orc.crc16_ibm(r.tobytes()) for r in blk] for blk in rows], S)
        label = ("rs_crc16_rows_kernel,MFMA" + ("" if aligned else ",UA")) if fold else "rs_crc16_rows_kernel"
    else:
        check = _raw32_check([[raw32(r.tobytes()) for r in blk] for blk in rows])
        label = "rs_crc32_rows_kernel,MFMA" if fold else "rs_crc32_rows_kernel"
    zero = [(b, r) for b in range(nb) for r in range(nrows) if not rows[b, r].any()]

    def check_all(r, ctx):
        check(r, ctx)
        for b, i in zero:  # R(zeros) = 0, stated on its own
            assert r[b, i] == 0, ctx + (b, i, "zeros")

    raw = Raw(torch, (nb, nrows + 1), check_all)

    def fn(h):
        c.set_option("crc%d_fold" % bits, fold)
        f = c.crc16_rows_dev if bits == 16 else c.crc32_rows_dev
        f(d.dev.data_ptr() + off, pitch, bs, nrows, S, nb, raw.dev.data_ptr(), nrows + 1, h)

    return Call(("crc%d_rows" % bits, fold, S, nb, aligned), c, [d, raw], fn, label)


# ---------------------------------------------------------------- leg A: every device entry point
def _a_encode(torch, rsmi, rng, k, m, S, nb, mode, label):
    c = rsmi.Codec(k, m)
    return c, [encode_call(torch, rsmi, c, S, nb, mode, rng, label)]


def _a_encode_crc(torch, rsmi, rng, k, m, S, nb, mode, fold, label):
    c = rsmi.Codec(k, m)
    c.set_option("crc16_fused_fold", fold)
    return c, [encode_call(torch, rsmi, c, S, nb, mode, rng, label, crc=True)]


def _a_reconstruct(torch, rsmi, rng, k, m, S, lost, data_only, required, label):
    c = rsmi.Codec(k, m)
    return c, [reconstruct_call(torch, rsmi, c, S, 3, "aligned", rng, lost, label, data_only=data_only,
                                required=required)]


def _a_crc_rows(torch, rsmi, rng, bits, fold, aligned):
    c = rsmi.Codec(10, 4)
    return c, [crc_rows_call(torch, rsmi, c, bits, fold, 8193, 2, aligned, _rows_data(rng, 2, 3, 8193))]


assert 3 * fused_units(4097) <= 64 < 13 * fused_units(16385) == 65

LEG_A = {
    # rsmi_encode_batch_dev
    "encode-10-4-aligned-4097": (_a_encode, 10, 4, 4097, 3, "aligned", fast_label(10, 4)),
    "encode-4-2-ua-1025": (_a_encode, 4, 2, 1025, 3, "ua", fast_label(4, 2, ua=True)),
    "encode-20-4-generic-333": (_a_encode, 20, 4, 333, 3, "aligned", generic_label(20, 4)),
    "encode-5-5-two-tiles-1040": (_a_encode, 5, 5, 1040, 3, "aligned", fast_label(5, 1)),
    # rsmi_reconstruct_batch_dev, in place
    "reconstruct-10-4-lost-3-11": (_a_reconstruct, 10, 4, 4097, [3, 11], False, None, fast_label(10, 2)),
    "reconstruct-10-4-lost-0-12-data-only": (_a_reconstruct, 10, 4, 4097, [0, 12], True, None, fast_label(10, 1)),
    "reconstruct-5-5-two-tiles": (_a_reconstruct, 5, 5, 1040, [0, 2, 4, 6, 9], False, None, fast_label(5, 1)),
    # rsmi_reconstruct_rows_batch_dev: row 0 keeps its 0xEE
    "reconstruct-rows-10-4-required-12": (_a_reconstruct, 10, 4, 4097, [0, 12], False, [12], fast_label(10, 1)),
    # rsmi_encode_batch_dev_crc
    "crc-fused-inl-4097": (_a_encode_crc, 10, 4, 4097, 3, "aligned", 1, fused_label(10, 4, 4097, 3)),
    "crc-fused-two-launch-16385": (_a_encode_crc, 10, 4, 16385, 13, "aligned", 1, fused_label(10, 4, 16385, 13)),
    "crc-nibble-4097": (_a_encode_crc, 10, 4, 4097, 3, "aligned", 0, fast_label(10, 4, crc=True)),
    "crc-nibble-16385": (_a_encode_crc, 10, 4, 16385, 13, "aligned", 0, fast_label(10, 4, crc=True)),
    "crc-fused-split-4111": (_a_encode_crc, 10, 4, 4111, 3, "split", 1, fused_label(10, 4, 4111, 3, ua=True)),
    # ... falling back to the separate passes: coding launch, memset, two CRC rows passes
    "crc-fallback-20-4-333": (_a_encode_crc, 20, 4, 333, 3, "aligned", 1, generic_label(20, 4)),
    "crc-fallback-5-5-1040": (_a_encode_crc, 5, 5, 1040, 3, "aligned", 1, fast_label(5, 1)),
    "crc-fallback-4-2-ua-15": (_a_encode_crc, 4, 2, 15, 3, "ua", 1, generic_label(4, 2)),
}
for _bits in (16, 32):
    for _fold in (1, 0):
        for _al in (True, False):
            LEG_A["crc%d-rows-fold%d-%s" % (_bits, _fold, "aligned" if _al else "ua")] = (_a_crc_rows, _bits, _fold, _al)


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(LEG_A))
def test_entry_point_behind_late_producer(gpu, case):
    """Leg A: one entry point per case at the smallest shape that takes each launch path, on a side
    stream behind the gate, its input arriving in stream order just before it."""
    torch, rsmi, gate = gpu
    assert fused_label(10, 4, 4097, 3).endswith(",INL") and ",INL" not in fused_label(10, 4, 16385, 13)
    assert fused_label(10, 4, 4111, 3, ua=True).endswith(",UA,INL")
    build, args = LEG_A[case][0], LEG_A[case][1:]
    with _leg("A"):
        c, calls = build(torch, rsmi, np.random.default_rng(zlib.crc32(case.encode())), *args)
        with c:
            # twice, on two side streams: the runtime maps streams onto a few hardware queues, and
            # a launch on the wrong stream that lands in the caller's own queue runs in order by
            # accident (seen with a memset moved to the NULL stream: one side stream in four hid
            # it); two streams taken from the pool one after the other have not both hidden it
            sts = [torch.cuda.Stream(), torch.cuda.Stream()]
            assert len({s.cuda_stream for s in sts} | {torch.cuda.current_stream().cuda_stream}) == 3
            for st in sts:
                warm_then_gated(torch, gate, [(st, x) for x in calls])


# ---------------------------------------------------------------- leg B: back-to-back calls
B_PATTERNS = ([3, 11], [0, 12], [1, 4, 11, 13])
B_UNSEEN = ([2], [5, 7, 10], [0, 1, 12, 13])


def _leg_b_calls(torch, rsmi, c, rng, patterns, with_reconstruct=True):
    al = "aligned"
    inl = fused_label(10, 4, 4097, 3)
    calls = [
        encode_call(torch, rsmi, c, 16385, 13, al, rng, fused_label(10, 4, 16385, 13), crc=True),
        encode_call(torch, rsmi, c, 4097, 3, al, rng, inl, crc=True),
        # the same unit counters, another unit count and another Crc16Shift
        encode_call(torch, rsmi, c, 1040, 2, al, rng, fused_label(10, 4, 1040, 2), crc=True),
        encode_call(torch, rsmi, c, 4097, 3, al, rng, fast_label(10, 4, crc=True), crc=True,
                    option=("crc16_fused_fold", 0)),
        encode_call(torch, rsmi, c, 4097, 3, al, rng, inl, crc=True, option=("crc16_fused_fold", 1)),
    ]
    for bits in (32, 16):  # the second size replaces the cached shift while the first launch is pending
        for S in (8193, 1025):
            calls.append(crc_rows_call(torch, rsmi, c, bits, 1, S, 2, True, _rows_data(rng, 2, 3, S)))
    if with_reconstruct:
        for lost in patterns:
            calls.append(reconstruct_call(torch, rsmi, c, 4097, 3, al, rng, lost, fast_label(10, len(lost))))
    calls.append(encode_call(torch, rsmi, c, 4097, 3, al, rng, fast_label(10, 4)))
    return calls


@pytest.mark.gpu
def test_back_to_back_calls_one_stream(gpu):
    """Leg B: thirteen calls of one Codec(10, 4) queued on one side stream behind one gate, each
    with its own buffers: two-launch and in-kernel combine forms sharing the stream's records and
    counters, the fused fold switched off and on between queued launches, both CRC rows passes at
    two sizes, three reconstruct patterns and a plain encode.  None of them waits."""
    torch, rsmi, gate = gpu
    with _leg("B"), rsmi.Codec(10, 4) as c:
        st = torch.cuda.Stream()
        calls = _leg_b_calls(torch, rsmi, c, np.random.default_rng(0xB), B_PATTERNS)
        assert len(calls) == 13
        warm_then_gated(torch, gate, [(st, x) for x in calls])


@pytest.mark.gpu
def test_back_to_back_calls_first_use_plans(gpu):
    """Leg B, second variant: the three reconstruct patterns are new to the Codec, so their plans
    are built (hipMalloc, hipMemcpy) while the earlier kernels are pending.  Correctness only; the
    state of the gate after the last call is printed.  Observed on an MI355X: the delay was still
    running when the calls returned, so a first use did not wait for the caller's stream."""
    torch, rsmi, gate = gpu
    with _leg("B"), rsmi.Codec(10, 4) as c:
        st = torch.cuda.Stream()
        rng = np.random.default_rng(0xB2)
        run_plan(torch, gate, [(st, x) for x in _leg_b_calls(torch, rsmi, c, rng, (), with_reconstruct=False)],
                 gated=False)
        calls = _leg_b_calls(torch, rsmi, c, rng, B_UNSEEN)
        done = run_plan(torch, gate, [(st, x) for x in calls], gated=True, must_not_wait=False)
        print("\nstream order: first use of three reconstruct plans behind the gate: the delay had %s "
              "when the calls returned" % ("ended (a call waited)" if any(done.values()) else "not ended (no wait)"))


# ---------------------------------------------------------------- leg C: scratch growth
@pytest.mark.gpu
def test_scratch_growth_behind_pending_work(gpu):
    """Leg C: a fresh Codec behind one gate: a small in-kernel-combine encode, then a two-launch
    one whose records outgrow the stream's scratch (reserve_on drains the stream first), then an
    in-kernel-combine one with more blocks than unit counters (drain, free, allocate, zero).  The
    library may block here; every output is exact and nothing is written after the consumer."""
    torch, rsmi, gate = gpu
    with _leg("C"), rsmi.Codec(10, 4) as c:
        st = torch.cuda.Stream()
        rng = np.random.default_rng(0xC)
        calls = [encode_call(torch, rsmi, c, 1040, 2, "aligned", rng, fused_label(10, 4, 1040, 2), crc=True),
                 encode_call(torch, rsmi, c, 16385, 13, "aligned", rng, fused_label(10, 4, 16385, 13), crc=True),
                 encode_call(torch, rsmi, c, 4097, 5, "aligned", rng, fused_label(10, 4, 4097, 5), crc=True)]
        assert [",INL" in x.label for x in calls] == [True, False, True]
        done = run_plan(torch, gate, [(st, x) for x in calls], gated=True, must_not_wait=False)
        print("\nstream order: scratch growth behind the gate: the delay had %s when the calls returned"
              % ("ended (a call waited)" if any(done.values()) else "not ended"))


# ---------------------------------------------------------------- leg D: two streams, one thread
@pytest.mark.gpu
def test_two_streams_interleaved(gpu):
    """Leg D: one Codec, two gated side streams, six fused encodes alternating between them with
    different S, in-kernel and two-launch combines mixed, no host sync until the end: records and
    unit counters are per stream.  The inputs of all six arrive first, then each stream waits for
    the other's (an event, in stream order), so the two run their launches at the same time."""
    torch, rsmi, gate = gpu
    with _leg("D"), rsmi.Codec(10, 4) as c:
        sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
        assert len({sa.cuda_stream, sb.cuda_stream, torch.cuda.current_stream().cuda_stream}) == 3
        rng = np.random.default_rng(0xD)
        shapes = [(65552, 8), (16385, 13), (5000, 4), (4097, 3), (65537, 5), (1040, 2)]
        plan = []
        for i, (S, nb) in enumerate(shapes):
            call = encode_call(torch, rsmi, c, S, nb, "aligned", rng, fused_label(10, 4, S, nb), crc=True)
            plan.append(((sa, sb)[i % 2], call))
        assert [",INL" in x.label for _, x in plan] == [False, False, True, True, False, True]
        warm_then_gated(torch, gate, plan, rendezvous=True)


# ---------------------------------------------------------------- leg E: past 32 caller streams
E_STREAMS = 40


def _hip_runtime():
    """The HIP runtime this process already loaded (torch's)."""
    with open("/proc/self/maps") as f:
        paths = sorted(set(ln.split()[-1] for ln in f if "libamdhip64" in ln))
    assert paths, "no HIP runtime loaded"
    return ctypes.CDLL(paths[0])


@pytest.mark.gpu
def test_past_32_caller_streams(gpu):
    """Leg E: fused in-kernel-combine encodes of one Codec(4, 2) on 40 or more distinct streams
    (torch's two pools, the current and the NULL stream, hipStreamCreateWithFlags for the rest),
    then again over the same streams in reverse, with no host sync: crc_scratch() drains the
    device and frees every stream's scratch on the way, twice.  All outputs exact."""
    torch, rsmi, gate = gpu
    with _leg("E"):
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
            if len(streams) < E_STREAMS:
                hip = _hip_runtime()
                hip.hipStreamCreateWithFlags.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
                hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
                while len(streams) < E_STREAMS:
                    h = ctypes.c_void_p()
                    assert hip.hipStreamCreateWithFlags(ctypes.byref(h), 1) == 0  # hipStreamNonBlocking
                    own.append(h)
                    add(torch.cuda.ExternalStream(h.value))
            streams = streams[:max(E_STREAMS, min(len(streams), 48))]
            handles = [s.cuda_stream for s in streams]
            assert len(set(handles)) >= E_STREAMS > KEPT_STREAMS
            assert 0 in handles
            sizes = (5000, 1040, 4097)  # the largest first: the records of a stream never regrow
            rng = np.random.default_rng(0xE)
            with rsmi.Codec(4, 2) as c:
                order = list(range(len(streams))) + list(reversed(range(len(streams))))
                plan = []
                for i in order:
                    S = sizes[i % 3]
                    label = fused_label(4, 2, S, 2)
                    assert label.endswith(",INL")
                    plan.append((streams[i], encode_call(torch, rsmi, c, S, 2, "aligned", rng, label, crc=True)))
                assert len(plan) >= 2 * E_STREAMS
                run_plan(torch, gate, plan, gated=False)
        finally:
            torch.cuda.synchronize()
            for h in own:
                hip.hipStreamDestroy(h)


# ---------------------------------------------------------------- leg F: saturating and single-bit rows
F_SIZES = [8192, 8193, 16385, 65536, 73729]
F_POSITIONS = [0, 15, 16, 1023, 1024, 4095, 4096, 8191, 8192]


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "ua"])
@pytest.mark.parametrize("S", F_SIZES)
def test_rows_passes_saturating_rows(gpu, S, aligned):
    """Leg F: rows of all 0xFF (every count of the matrix-core folds at its maximum, over whole
    8 KiB groups and a partial last one) and of all zeros (R = 0) through rsmi_crc16_rows_dev and
    rsmi_crc32_rows_dev, fold 1 and fold 0; at S = 8193 also one row per position with the single
    byte 0x80, then 0x01, in a row of zeros.  Expected values from zlib and the CRC-16 oracle."""
    torch, rsmi, gate = gpu
    rows = [np.full(S, 0xFF, dtype=np.uint8), np.zeros(S, dtype=np.uint8)]
    if S == 8193:
        for v in (0x80, 0x01):
            for p in F_POSITIONS:
                r = np.zeros(S, dtype=np.uint8)
                r[p] = v
                rows.append(r)
    rows = np.stack(rows)
    rows = np.stack([rows, rows[::-1]])  # nb = 2, the second block in reverse row order
    assert raw32(bytes(S)) == 0
    with _leg("F"), rsmi.Codec(10, 4) as c:
        st = torch.cuda.Stream()
        plan = [(st, crc_rows_call(torch, rsmi, c, bits, fold, S, 2, aligned, rows))
                for bits in (16, 32) for fold in (1, 0)]
        run_plan(torch, gate, plan, gated=False)
