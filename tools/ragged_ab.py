#!/usr/bin/env python3
"""The ragged encode against the uniform call, one process, one GPU.

rsmi_encode_ragged_batch_dev classes the blocks on the host, uploads their descriptors and units
and launches rs_ragged_kernel once per class.  RS(10,4), 4096 blocks, device-resident, HIP-event
timed around the whole call: both legs run untimed for --settle-ms first (past the GPU's start-up
power transient), then per alternation 3 warm-up calls and the median of 20 calls, reference then
ragged, six alternations.  The reference is the same build's rsmi_encode_batch_dev, whose kernels
this change leaves as they were.

  (a) every block 256 KiB, rows at rsmi_recommended_pitch(S): the ragged call against one
      rsmi_encode_batch_dev -- the price of raggedness (not a gate); the ragged call's host wall
      time says how much of the difference is spent before its launch
  (b) block sizes drawn seeded from 1 B to 256 KiB, every block's rows 16-byte aligned at pitch
      roundup(S, 16): the ragged call against the loop over runs of equal sizes, one
      rsmi_encode_batch_dev per run -- the only way to encode such a batch before this call.
      Done when every ragged run is faster than every loop run in all alternations.
  (c) one 256 KiB block among 4095 blocks of 100 bytes: the host time of classing and upload, as
      host wall time of the call

TB/s counts the (k + m) * S payload bytes of every block.

  python tools/ragged_ab.py [--alternations 6] [--launches 20] [--warmup 3] [--settle-ms 500] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "filedag-storage_amd"))


def median_us(torch, fn, warmup, launches):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(launches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return statistics.median(times), min(times), max(times)


def host_us(torch, fn, alternations, launches, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    meds = []
    for _ in range(alternations):
        times = []
        for _ in range(launches):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times.append((time.perf_counter() - t0) * 1e6)
        meds.append(statistics.median(times))
    torch.cuda.synchronize()
    return statistics.median(meds), max(meds) - min(meds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=6)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle-ms", type=int, default=500)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch

    import rsmi

    assert torch.cuda.is_available(), "needs a GPU"
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    k, m, nb = 10, 4, 4096
    n = k + m
    emit("# ragged vs uniform encode, RS(%d,%d), %d blocks, device-resident, HIP events around the whole call, "
         "median of %d calls after %d warm-ups, %d alternations, %d ms settle; TB/s over (k+m)*S payload bytes"
         % (k, m, nb, args.launches, args.warmup, args.alternations, args.settle_ms))
    emit("# device: %s" % torch.cuda.get_device_name(0))
    stream = torch.cuda.current_stream().cuda_stream

    def layout(sizes, pitch):
        """Per block (S, offset, pitch): its k + m rows side by side; the buffer's size."""
        rows, off = [], 0
        for S in sizes:
            P = pitch(S)
            rows.append((S, off, P))
            off += n * P
        return rows, off

    def descriptors(rows):
        return np.ascontiguousarray(np.array([[S, off, P, off + k * P, P] for S, off, P in rows], dtype=np.uint64))

    with rsmi.Codec(k, m, 0) as c:
        def timed(case, rows, extra):
            """One case: the loop of uniform calls over runs of equal (S, pitch) against the ragged call."""
            size = rows[-1][1] + n * rows[-1][2]
            d = torch.randint(0, 256, (size,), dtype=torch.uint8, device="cuda")
            base = d.data_ptr()
            desc = descriptors(rows)
            runs, b = [], 0
            while b < len(rows):
                e = b + 1
                while e < len(rows) and rows[e][0] == rows[b][0] and rows[e][2] == rows[b][2]:
                    e += 1
                runs.append((rows[b][1], rows[b][0], rows[b][2], e - b))
                b = e
            payload = sum(n * S for S, _, _ in rows)

            def ref():
                for off, S, P, cnt in runs:
                    c.encode_batch_dev(base + off, P, n * P, base + off + k * P, P, n * P, S, cnt, stream)

            def rag():
                c.encode_ragged_batch_dev(base, base, desc, stream)

            ref()
            torch.cuda.synchronize()
            rlabel = c.last_kernel()
            good = d.clone()
            for S, off, P in rows[:64] + rows[-64:]:   # the parity rows' bytes are poisoned, then rebuilt
                d[off + k * P:off + k * P + S].fill_(0x5C)
            rag()
            torch.cuda.synchronize()
            glabel = c.last_kernel()
            assert torch.equal(d, good), "%s: the ragged call's bytes differ from the uniform calls'" % case
            t_end = time.perf_counter() + args.settle_ms / 1e3
            while time.perf_counter() < t_end:
                ref()
                rag()
                torch.cuda.synchronize()
            meds = {"ref": [], "ragged": []}
            lo_hi = {"ref": [], "ragged": []}
            for alt in range(args.alternations):
                row = dict(case=case, k=k, m=m, blocks=len(rows), alternation=alt, ref_calls=len(runs), ref_kernel=rlabel,
                           ragged_kernel=glabel, **extra)
                for what, fn in (("ref", ref), ("ragged", rag)):
                    med, lo, hi = median_us(torch, fn, args.warmup, args.launches)
                    meds[what].append(med)
                    lo_hi[what] += [lo, hi]
                    row[what + "_us"] = round(med, 2)
                    row[what + "_min_us"] = round(lo, 2)
                    row[what + "_max_us"] = round(hi, 2)
                    row[what + "_TBps"] = round(payload / med / 1e6, 3)
                row["ragged_over_ref"] = round(row["ragged_us"] / row["ref_us"], 4)
                emit(json.dumps(row))
            hcall, hspread = host_us(torch, rag, args.alternations, args.launches, args.warmup)
            emit(json.dumps({"case": case, "summary": {
                what: {"median_us": round(statistics.median(v), 2), "spread_us": round(max(v) - min(v), 2),
                       "spread_pct": round(100 * (max(v) - min(v)) / statistics.median(v), 2)}
                for what, v in meds.items()},
                "ragged_over_ref": round(statistics.median(meds["ragged"]) / statistics.median(meds["ref"]), 4),
                "ragged_host_call_us": round(hcall, 2), "ragged_host_call_spread_us": round(hspread, 2),
                "slowest_ragged_run_us": round(max(lo_hi["ragged"]), 2), "fastest_ref_run_us": round(min(lo_hi["ref"]), 2),
                "every_ragged_run_faster_than_every_ref_run": max(lo_hi["ragged"]) < min(lo_hi["ref"])}))
            assert torch.equal(d, good), "%s: wrong bytes after the timed calls" % case
            del d, good
            torch.cuda.empty_cache()

        # (a) every block 256 KiB at the recommended pitch
        S256 = ((256 << 10) + k - 1) // k
        rows, _ = layout([S256] * nb, rsmi.recommended_pitch)
        timed("a_equal_256KiB", rows, {"S": S256, "pitch": rsmi.recommended_pitch(S256)})
        # (b) seeded block sizes from 1 B to 256 KiB
        blocks = np.random.default_rng(0xB10C5).integers(1, (256 << 10) + 1, size=nb)
        sizes = [(int(B) + k - 1) // k for B in blocks]
        rows, _ = layout(sizes, lambda S: (S + 15) // 16 * 16)
        timed("b_seeded_sizes", rows, {"distinct_S": len(set(sizes)), "min_S": min(sizes), "max_S": max(sizes)})
        # (c) one large block among small ones: the host time of classing and upload
        sizes = [10] * nb
        sizes[nb // 2] = S256
        rows, size = layout(sizes, lambda S: (S + 15) // 16 * 16)
        d = torch.randint(0, 256, (size,), dtype=torch.uint8, device="cuda")
        desc = descriptors(rows)
        hcall, hspread = host_us(torch, lambda: c.encode_ragged_batch_dev(d.data_ptr(), d.data_ptr(), desc, stream),
                                 args.alternations, args.launches, args.warmup)
        emit(json.dumps({"case": "c_one_large_block", "blocks": nb, "kernel": c.last_kernel(),
                         "host_call_us": round(hcall, 2), "spread_us": round(hspread, 2),
                         "host_call_ns_per_block": round(1e3 * hcall / nb, 1)}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
