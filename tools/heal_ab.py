#!/usr/bin/env python3
"""Locate against heal of the same stripes, one process, one GPU.

rsmi_heal_batch_dev is rsmi_locate_batch_dev's launches and, behind the verdict kernel on the
stream, rs_heal_kernel: on a block whose verdict names no shard a wave reads the verdict and
ends; on a block with a culprit it runs Verify's pipeline once more and stores the culprit row.
RS(10,4), 4096 blocks of 256 KiB, device-resident rows at rsmi_recommended_pitch(S), HIP-event
timed: both calls run untimed for --settle-ms first (past the GPU's start-up power transient),
then per alternation 3 warm-up launches and the median of 20 launches, locate then heal, six
alternations.  The baseline is the same build's rsmi_locate_batch_dev.

  (a) clean stripes: every verdict is clean, the heal kernel writes nothing
  (b) the whole first data row of every block stale: every block is healed.  A healed buffer is
      clean, so the row is damaged again before every launch, of both calls, outside the timed
      interval (the events are recorded behind the damage on the stream)

TB/s counts the (k + m) * S payload bytes of every block, for both calls.  heal_over_locate is
the ratio of the medians of one alternation; the spread of a leg is its medians' range over the
alternations.

  python tools/heal_ab.py [--alternations 6] [--launches 20] [--warmup 3] [--settle-ms 500] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "filedag-storage_amd"))


def median_us(torch, fn, prep, warmup, launches):
    for _ in range(warmup):
        prep()
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(launches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        prep()
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
    emit("# locate vs heal, RS(%d,%d) %d x %d KiB, device-resident, rows at rsmi_recommended_pitch, median of %d "
         "launches after %d warm-ups, %d alternations, %d ms settle; TB/s over (k+m)*S*blocks payload bytes"
         % (k, m, nb, block >> 10, args.launches, args.warmup, args.alternations, args.settle_ms))
    emit("# device: %s" % torch.cuda.get_device_name(0))
    d = torch.randint(0, 256, (nb * bs,), dtype=torch.uint8, device="cuda")
    bad = torch.zeros(nb * m, dtype=torch.int32, device="cuda")
    cul = torch.zeros(nb, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    row0 = d.view(nb, bs)[:, :S]
    with rsmi.Codec(k, m, 0) as c:
        def loc():
            c.locate_batch_dev(d.data_ptr(), rs, bs, d.data_ptr() + k * rs, rs, bs, S, nb, cul.data_ptr(),
                               bad.data_ptr(), stream)

        def heal():
            c.heal_batch_dev(d.data_ptr(), rs, bs, d.data_ptr() + k * rs, rs, bs, S, nb, cul.data_ptr(),
                             bad.data_ptr(), stream)

        c.encode_batch_dev(d.data_ptr(), rs, bs, d.data_ptr() + k * rs, rs, bs, S, nb, stream)
        torch.cuda.synchronize()
        good = row0.clone()
        stale = good ^ 0x01  # every byte of data row 0 of every block: no clean tile

        def nothing():
            pass

        def damage():
            row0.copy_(stale)

        for case, prep in (("a_clean", nothing), ("b_row0_stale", damage)):
            damaged = prep is damage
            prep()
            loc()
            torch.cuda.synchronize()
            llabel = c.last_kernel()
            assert int(bad.count_nonzero()) == (nb * m if damaged else 0)
            assert bool((cul == (0 if damaged else rsmi.LocateClean)).all()), "wrong verdicts"
            heal()
            torch.cuda.synchronize()
            hlabel = c.last_kernel()
            assert bool((cul == (0 if damaged else rsmi.LocateClean)).all()), "wrong verdicts"
            assert torch.equal(row0, good), "not healed"
            loc()
            torch.cuda.synchronize()
            assert bool((cul == rsmi.LocateClean).all()) and int(bad.count_nonzero()) == 0, "dirty after the heal"
            t_end = time.perf_counter() + args.settle_ms / 1e3
            while time.perf_counter() < t_end:
                prep()
                loc()
                prep()
                heal()
                torch.cuda.synchronize()
            meds = {"locate": [], "heal": []}
            for alt in range(args.alternations):
                row = {"case": case, "k": k, "m": m, "S": S, "pitch": rs, "blocks": nb, "alternation": alt,
                       "locate_kernel": llabel, "heal_kernel": hlabel}
                for what, fn in (("locate", loc), ("heal", heal)):
                    med, lo, hi = median_us(torch, fn, prep, args.warmup, args.launches)
                    meds[what].append(med)
                    row[what + "_us"] = round(med, 2)
                    row[what + "_min_us"] = round(lo, 2)
                    row[what + "_max_us"] = round(hi, 2)
                    row[what + "_TBps"] = round(payload / med / 1e6, 3)
                row["heal_over_locate"] = round(row["heal_us"] / row["locate_us"], 4)
                emit(json.dumps(row))
            emit(json.dumps({"case": case, "summary": {
                what: {"median_us": round(statistics.median(v), 2), "spread_us": round(max(v) - min(v), 2),
                       "spread_pct": round(100 * (max(v) - min(v)) / statistics.median(v), 2)}
                for what, v in meds.items()},
                "heal_over_locate": round(statistics.median(meds["heal"]) / statistics.median(meds["locate"]), 4)}))
            if damaged:
                assert torch.equal(row0, good), "the last heal left damage"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
