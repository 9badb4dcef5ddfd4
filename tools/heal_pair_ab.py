#!/usr/bin/env python3
"""Pair heal against pair locate, heal and the read-back route, one process, one GPU.

rsmi_heal_pair_batch_dev is rsmi_locate_pair_batch_dev's launches and, behind the pair verdict
kernel on the stream, rs_heal_pair_kernel: on a block whose verdict names no shard a wave reads the
verdict and ends, as rs_heal_kernel does; on a block with one or two named shards it runs Verify's
pipeline once more and stores the named rows.  RS(10,4), 4096 blocks of 256 KiB, device-resident
rows at rsmi_recommended_pitch(S), HIP-event timed, the method of tools/heal_ab.py: every call
runs untimed for --settle-ms first, then per alternation 3 warm-up launches and the median of 20
launches of every leg in turn, six alternations.  The baselines are the same build's
rsmi_locate_batch_dev, rsmi_heal_batch_dev and rsmi_locate_pair_batch_dev.

  (a) clean stripes: legs locate, heal, pair, heal_pair.  What heal_pair adds to pair is one
      early-exit launch, as what heal adds to locate is.  The condition: per alternation
      add_heal_pair = heal_pair - pair and add_heal = heal - locate; the median of the first may
      exceed the median of the second by no more than the larger of the two additions' spreads
      (the range of an addition over the alternations).
  (b) data rows 0 and 1 stale in 1 % of the blocks, (c) in every block: legs heal_pair and route,
      the read-back route timed end to end: rsmi_locate_pair_batch_dev, the verdicts copied to the
      host, present / required masks built there, rsmi_reconstruct_mixed_batch_dev.  The events
      bracket the whole route on the stream, the host's share included.  The rows are damaged
      again before every launch of either leg, outside the timed interval.  Reported, not gated.

  python tools/heal_pair_ab.py [--cases abc] [--alternations 6] [--launches 20] [--warmup 3]
                               [--settle-ms 500] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "filedag-storage_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from heal_ab import median_us  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="abc")
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

    k, m, block, nb = 10, 4, 256 << 10, 4096
    S = (block + k - 1) // k
    rs = rsmi.recommended_pitch(S)
    n = k + m
    bs = n * rs
    payload = n * S * nb
    emit("# locate / heal / locate_pair / heal_pair / read-back route, RS(%d,%d) %d x %d KiB, device-resident, rows at "
         "rsmi_recommended_pitch, median of %d launches after %d warm-ups, %d alternations, %d ms settle; TB/s over "
         "(k+m)*S*blocks payload bytes" % (k, m, nb, block >> 10, args.launches, args.warmup, args.alternations,
                                           args.settle_ms))
    emit("# device: %s" % torch.cuda.get_device_name(0))
    d = torch.randint(0, 256, (nb * bs,), dtype=torch.uint8, device="cuda")
    bad = torch.zeros(nb * m, dtype=torch.int32, device="cuda")
    cul = torch.zeros(nb, dtype=torch.int32, device="cuda")
    pair = torch.zeros(nb, 2, dtype=torch.int32, device="cuda")
    status = np.zeros(nb, dtype=np.int32)
    stream = torch.cuda.current_stream().cuda_stream
    rows01 = d.view(nb, bs)[:, :2 * rs]
    L = rsmi.lib()
    with rsmi.Codec(k, m, 0) as c:
        a = (d.data_ptr(), rs, bs, d.data_ptr() + k * rs, rs, bs, S, nb)

        def loc():
            c.locate_batch_dev(*a, cul.data_ptr(), bad.data_ptr(), stream)

        def heal():
            c.heal_batch_dev(*a, cul.data_ptr(), bad.data_ptr(), stream)

        def prs():
            c.locate_pair_batch_dev(*a, pair.data_ptr(), bad.data_ptr(), stream)

        def hpr():
            c.heal_pair_batch_dev(*a, pair.data_ptr(), bad.data_ptr(), stream)

        def route():
            prs()
            v = pair.cpu().numpy()  # the read-back: a copy and a stream sync
            present = np.ones((nb, n), dtype=np.uint8)
            for col in (0, 1):
                named = np.flatnonzero(v[:, col] >= 0)
                present[named, v[named, col]] = 0
            required = (1 - present).astype(np.uint8)
            rc = L.rsmi_reconstruct_mixed_batch_dev(c._h, d.data_ptr(), rs, bs, S, nb, present.ctypes.data,
                                                    required.ctypes.data, 0, status.ctypes.data, stream)
            assert rc == 0, rc

        c.encode_batch_dev(*a, stream)
        torch.cuda.synchronize()
        good = rows01.clone()
        stale = good.clone()
        stale[:, :S] ^= 0x01  # every byte of rows 0 and 1: no clean tile
        stale[:, rs:rs + S] ^= 0x02
        some = torch.arange(0, nb, 100, device="cuda")  # 1 % of the blocks, spread over the batch

        def nothing():
            pass

        def damage_some():
            rows01[some] = stale[some]

        def damage_all():
            rows01.copy_(stale)

        cases = {"a": ("a_clean", nothing, 0, (("locate", loc), ("heal", heal), ("pair", prs), ("heal_pair", hpr))),
                 "b": ("b_rows01_stale_1pct", damage_some, int(some.numel()), (("heal_pair", hpr), ("route", route))),
                 "c": ("c_rows01_stale_all", damage_all, nb, (("heal_pair", hpr), ("route", route)))}
        for key in args.cases:
            case, prep, dirty, legs = cases[key]
            rows01.copy_(good)
            labels = {}
            for what, fn in legs:
                prep()
                fn()
                torch.cuda.synchronize()
                labels[what + "_kernel"] = c.last_kernel()
                if what in ("pair", "heal_pair", "route"):
                    got = pair.cpu()
                    assert int((got[:, 0] == 0).sum()) == dirty and int((got[:, 1] == 1).sum()) == dirty, "wrong pairs"
                    assert int((got[:, 0] == -1).sum()) == nb - dirty, "wrong verdicts"
                if what in ("heal_pair", "route"):
                    assert torch.equal(rows01, good), what + " left damage"
            t_end = time.perf_counter() + args.settle_ms / 1e3
            while time.perf_counter() < t_end:
                for _, fn in legs:
                    prep()
                    fn()
                torch.cuda.synchronize()
            meds = {what: [] for what, _ in legs}
            for alt in range(args.alternations):
                row = {"case": case, "k": k, "m": m, "S": S, "pitch": rs, "blocks": nb, "dirty_blocks": dirty,
                       "alternation": alt}
                row.update(labels)
                for what, fn in legs:
                    med, lo, hi = median_us(torch, fn, prep, args.warmup, args.launches)
                    meds[what].append(med)
                    row[what + "_us"] = round(med, 2)
                    row[what + "_min_us"] = round(lo, 2)
                    row[what + "_max_us"] = round(hi, 2)
                    row[what + "_TBps"] = round(payload / med / 1e6, 3)
                emit(json.dumps(row))
            summ = {what: {"median_us": round(statistics.median(v), 2), "spread_us": round(max(v) - min(v), 2),
                           "spread_pct": round(100 * (max(v) - min(v)) / statistics.median(v), 2)}
                    for what, v in meds.items()}
            out = {"case": case, "summary": summ}
            if key == "a":
                add_hp = [x - y for x, y in zip(meds["heal_pair"], meds["pair"])]
                add_h = [x - y for x, y in zip(meds["heal"], meds["locate"])]
                allow = max(max(add_hp) - min(add_hp), max(add_h) - min(add_h))
                over = statistics.median(add_hp) - statistics.median(add_h)
                out["condition"] = {"heal_pair_minus_pair_us": round(statistics.median(add_hp), 2),
                                    "heal_pair_minus_pair_spread_us": round(max(add_hp) - min(add_hp), 2),
                                    "heal_minus_locate_us": round(statistics.median(add_h), 2),
                                    "heal_minus_locate_spread_us": round(max(add_h) - min(add_h), 2),
                                    "over_us": round(over, 2), "allowance_us": round(allow, 2),
                                    "met": bool(over <= allow)}
            else:
                out["heal_pair_over_route"] = round(statistics.median(meds["heal_pair"]) /
                                                    statistics.median(meds["route"]), 4)
            emit(json.dumps(out))
            assert torch.equal(rows01, good), "the last heal left damage"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
