#!/usr/bin/env python3
"""Verify against locate of the same stripes, one process, one GPU.

rsmi_locate_batch_dev reads the k + m rows rsmi_verify_batch_dev reads and raises the same flags;
on a clean tile it adds one branch, on a dirty tile the candidate tests and one atomic AND, and
after the rows kernel a one-thread-per-block verdict kernel.  RS(10,4), 4096 blocks of 256 KiB,
device-resident rows at rsmi_recommended_pitch(S), HIP-event timed: both calls run untimed for
--settle-ms first (past the GPU's start-up power transient), then per alternation 3 warm-up
launches and the median of 20 launches, verify then locate, at least 3 alternations.

  (a) clean stripes: no flag raised, no candidate formed
  (b) the whole first data row of every block damaged: every wave of the launch raises its m
      flags and names the shard (the datanode that came back stale)

TB/s counts the (k + m) * S payload bytes of every block, for both calls.  locate_over_verify is
the ratio of the medians of one alternation; the spread of a leg is its medians' range over the
alternations.

  python tools/locate_ab.py [--alternations 3] [--launches 20] [--warmup 3] [--settle-ms 500] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle-ms", type=int, default=500)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    import rsmi

    assert torch.cuda.is_available(), "needs a GPU"
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    k, m, block, nb = 10, 4, 256 << 10, 4096
    S = (block + k - 1) // k
    rs = rsmi.recommended_pitch(S)
    n = k + m
    bs = n * rs
    payload = n * S * nb
    emit("# verify vs locate, RS(%d,%d) %d x %d KiB, device-resident, rows at rsmi_recommended_pitch, median of %d "
         "launches after %d warm-ups, %d alternations, %d ms settle; TB/s over (k+m)*S*blocks payload bytes"
         % (k, m, nb, block >> 10, args.launches, args.warmup, args.alternations, args.settle_ms))
    emit("# device: %s" % torch.cuda.get_device_name(0))
    d = torch.randint(0, 256, (nb * bs,), dtype=torch.uint8, device="cuda")
    bad = torch.zeros(nb * m, dtype=torch.int32, device="cuda")
    cul = torch.zeros(nb, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    with rsmi.Codec(k, m, 0) as c:
        def ver():
            c.verify_batch_dev(d.data_ptr(), rs, bs, d.data_ptr() + k * rs, rs, bs, S, nb, bad.data_ptr(), stream)

        def loc():
            c.locate_batch_dev(d.data_ptr(), rs, bs, d.data_ptr() + k * rs, rs, bs, S, nb, cul.data_ptr(),
                               bad.data_ptr(), stream)

        c.encode_batch_dev(d.data_ptr(), rs, bs, d.data_ptr() + k * rs, rs, bs, S, nb, stream)
        for case, damaged in (("a_clean", False), ("b_all_damaged", True)):
            if damaged:
                d.view(nb, bs)[:, :S] ^= 0x01  # every byte of data row 0 of every block: no clean tile
            ver()
            torch.cuda.synchronize()
            vlabel = c.last_kernel()
            assert int(bad.count_nonzero()) == (nb * m if damaged else 0)
            loc()
            torch.cuda.synchronize()
            llabel = c.last_kernel()
            assert int(bad.count_nonzero()) == (nb * m if damaged else 0)
            assert bool((cul == (0 if damaged else rsmi.LocateClean)).all()), "wrong verdicts"
            t_end = time.perf_counter() + args.settle_ms / 1e3
            while time.perf_counter() < t_end:
                ver()
                loc()
                torch.cuda.synchronize()
            meds = {"verify": [], "locate": []}
            for alt in range(args.alternations):
                row = {"case": case, "k": k, "m": m, "S": S, "pitch": rs, "blocks": nb, "alternation": alt,
                       "verify_kernel": vlabel, "locate_kernel": llabel}
                for what, fn in (("verify", ver), ("locate", loc)):
                    med, lo, hi = median_us(torch, fn, args.warmup, args.launches)
                    meds[what].append(med)
                    row[what + "_us"] = round(med, 2)
                    row[what + "_min_us"] = round(lo, 2)
                    row[what + "_max_us"] = round(hi, 2)
                    row[what + "_TBps"] = round(payload / med / 1e6, 3)
                row["locate_over_verify"] = round(row["locate_us"] / row["verify_us"], 4)
                emit(json.dumps(row))
            emit(json.dumps({"case": case, "summary": {
                what: {"median_us": round(statistics.median(v), 2), "spread_us": round(max(v) - min(v), 2),
                       "spread_pct": round(100 * (max(v) - min(v)) / statistics.median(v), 2)}
                for what, v in meds.items()},
                "locate_over_verify": round(statistics.median(meds["locate"]) / statistics.median(meds["verify"]), 4)}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
