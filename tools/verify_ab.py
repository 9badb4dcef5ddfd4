#!/usr/bin/env python3
"""Encode against verify of the same shape, one process, one GPU.

Verify (rsmi_verify_batch_dev) reads the k + m rows the encode (rsmi_encode_batch_dev) reads and
writes, so it moves the same HBM bytes, all of them loads.  Device-resident rows at
rsmi_recommended_pitch(S), HIP-event timed: per alternation, 3 warm-up launches and then the median
of 20 launches, encode then verify, at least 3 alternations.  Shapes: RS(10,4) 4096 x 256 KiB,
RS(2,1) 4096 x 256 KiB, RS(16,4) 256 x 4 MiB on clean stripes (no flag raised: a pure read
stream), and RS(10,4) once more with the whole first data row of every block damaged, so every
wave of the launch raises its m flags (the all-atomics case).

TB/s counts the (k + m) * S payload bytes of every block, for both calls.

  python tools/verify_ab.py [--alternations 3] [--launches 20] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "filedag-storage_amd"))

SHAPES = [
    ("rs10_4_256k", 10, 4, 256 << 10, 4096, False),
    ("rs2_1_256k", 2, 1, 256 << 10, 4096, False),
    ("rs16_4_4m", 16, 4, 4 << 20, 256, False),
    ("rs10_4_256k_all_damaged", 10, 4, 256 << 10, 4096, True),
]


def ceil_div(a, b):
    return (a + b - 1) // b


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
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    import rsmi

    assert torch.cuda.is_available(), "needs a GPU"
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# encode vs verify, device-resident, rows at rsmi_recommended_pitch, median of %d launches after %d "
         "warm-ups, %d alternations; TB/s over (k+m)*S*blocks payload bytes" % (args.launches, args.warmup,
                                                                              args.alternations))
    emit("# device: %s" % torch.cuda.get_device_name(0))
    for name, k, m, block, nb, damaged in SHAPES:
        S = ceil_div(block, k)
        rs = rsmi.recommended_pitch(S)
        n = k + m
        bs = n * rs
        d = torch.randint(0, 256, (nb * bs,), dtype=torch.uint8, device="cuda")
        bad = torch.zeros(nb * m, dtype=torch.int32, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        payload = n * S * nb
        with rsmi.Codec(k, m, 0) as c:
            def enc():
                c.encode_batch_dev(d.data_ptr(), rs, bs, d.data_ptr() + k * rs, rs, bs, S, nb, stream)

            def ver():
                c.verify_batch_dev(d.data_ptr(), rs, bs, d.data_ptr() + k * rs, rs, bs, S, nb, bad.data_ptr(), stream)

            enc()
            ver()
            torch.cuda.synchronize()
            vlabel = c.last_kernel()
            assert int(bad.count_nonzero()) == 0, "a fresh encode does not verify"
            if damaged:
                d.view(nb, bs)[:, :S] ^= 0x01  # every byte of data row 0 of every block: no clean tile
                ver()
                torch.cuda.synchronize()
                assert int(bad.count_nonzero()) == nb * m, "every flag of every block must be raised"
            for alt in range(args.alternations):
                row = {"shape": name, "k": k, "m": m, "S": S, "pitch": rs, "blocks": nb, "alternation": alt,
                       "verify_kernel": vlabel}
                for what, fn in (("encode", enc), ("verify", ver)):
                    if damaged and what == "encode":
                        continue  # the encode would repair the stripes
                    med, lo, hi = median_us(torch, fn, args.warmup, args.launches)
                    row[what + "_us"] = round(med, 2)
                    row[what + "_min_us"] = round(lo, 2)
                    row[what + "_max_us"] = round(hi, 2)
                    row[what + "_TBps"] = round(payload / med / 1e6, 3)
                if "encode_us" in row:
                    row["verify_over_encode"] = round(row["verify_us"] / row["encode_us"], 4)
                emit(json.dumps(row))
        del d, bad
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
