#!/usr/bin/env python3
"""The one-pass scrub against the two passes it replaces, one process, one GPU.

  two-pass  rsmi_verify_batch_dev, then rsmi_crc16_rows_dev over the data rows and over the parity
            rows, all on one stream: every row is read twice
  scrub     one rsmi_scrub_batch_dev: the same flags and raws from one read of the rows
  verify    rsmi_verify_batch_dev alone: what the fold costs the scrub on top of it

Device-resident rows at rsmi_recommended_pitch(S), HIP events around the whole route: per
alternation, 3 warm-ups and then the median of 20, the routes in turn, 6 alternations.  Shapes:
RS(10,4), RS(4,2) and RS(2,1) 4096 x 256 KiB and RS(16,4) 256 x 4 MiB on clean stripes, and RS(10,4)
once more with the whole first data row of every block damaged, so every tile raises its m flags.
Before timing, the two routes' flags and raws are compared whole.

TB/s counts the (k + m) * S payload bytes of every block once, for every route.

  python tools/scrub_ab.py [--alternations 6] [--launches 20] [--warmup 3] [--only SHAPE] [--out FILE]
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
    ("rs4_2_256k", 4, 2, 256 << 10, 4096, False),
    ("rs16_4_4m", 16, 4, 4 << 20, 256, False),
    ("rs2_1_256k", 2, 1, 256 << 10, 4096, False),
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
    ap.add_argument("--alternations", type=int, default=6)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", help="one shape by name")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    import rsmi

    assert torch.cuda.is_available(), "needs a GPU"
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# scrub vs verify + CRC-16 rows passes, device-resident, rows at rsmi_recommended_pitch, median of %d after "
         "%d warm-ups, %d alternations; TB/s over (k+m)*S*blocks payload bytes" %
         (args.launches, args.warmup, args.alternations))
    emit("# device: %s" % torch.cuda.get_device_name(0))
    for name, k, m, block, nb, damaged in SHAPES:
        if args.only and name != args.only:
            continue
        S = ceil_div(block, k)
        rs = rsmi.recommended_pitch(S)
        n = k + m
        bs = n * rs
        d = torch.randint(0, 256, (nb * bs,), dtype=torch.uint8, device="cuda")
        bad1 = torch.zeros(nb * m, dtype=torch.int32, device="cuda")
        raw1 = torch.zeros(nb * n, dtype=torch.int32, device="cuda")
        bad2 = torch.full((nb * m,), -1, dtype=torch.int32, device="cuda")
        raw2 = torch.full((nb * n,), -1, dtype=torch.int32, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        payload = n * S * nb
        dp, pp = d.data_ptr(), d.data_ptr() + k * rs
        with rsmi.Codec(k, m, 0) as c:
            def ver():
                c.verify_batch_dev(dp, rs, bs, pp, rs, bs, S, nb, bad1.data_ptr(), stream)

            def two_pass():
                ver()
                c.crc16_rows_dev(dp, rs, bs, k, S, nb, raw1.data_ptr(), n, stream)
                c.crc16_rows_dev(pp, rs, bs, m, S, nb, raw1.data_ptr() + 4 * k, n, stream)

            def scrub():
                c.scrub_batch_dev(dp, rs, bs, pp, rs, bs, S, nb, bad2.data_ptr(), raw2.data_ptr(), stream)

            c.encode_batch_dev(dp, rs, bs, pp, rs, bs, S, nb, stream)
            if damaged:
                d.view(nb, bs)[:, :S] ^= 0x01  # every byte of data row 0 of every block: no clean tile
            two_pass()
            scrub()
            torch.cuda.synchronize()
            label = c.last_kernel()
            assert int(bad1.count_nonzero()) == (nb * m if damaged else 0), "the stripes are not what the case says"
            assert torch.equal(bad1 != 0, bad2 != 0), "the two routes' flags differ"
            assert torch.equal(raw1, raw2), "the two routes' raws differ"
            routes = [("two_pass", two_pass), ("scrub", scrub), ("verify", ver)]
            for alt in range(args.alternations):
                row = {"shape": name, "k": k, "m": m, "S": S, "pitch": rs, "blocks": nb, "alternation": alt,
                       "scrub_kernel": label}
                for what, fn in routes:
                    med, lo, hi = median_us(torch, fn, args.warmup, args.launches)
                    row[what + "_us"] = round(med, 2)
                    row[what + "_min_us"] = round(lo, 2)
                    row[what + "_max_us"] = round(hi, 2)
                    row[what + "_TBps"] = round(payload / med / 1e6, 3)
                row["scrub_over_two_pass"] = round(row["scrub_us"] / row["two_pass_us"], 4)
                row["scrub_over_verify"] = round(row["scrub_us"] / row["verify_us"], 4)
                emit(json.dumps(row))
        del d, bad1, raw1, bad2, raw2
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
