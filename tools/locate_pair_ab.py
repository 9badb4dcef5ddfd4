#!/usr/bin/env python3
"""Pair locate against locate and heal of the same stripes, one process, one GPU.

rsmi_locate_pair_batch_dev is rsmi_locate_batch_dev's launches and, behind the verdict kernel on
the stream, rs_locate_pair_kernel and rs_locate_pair_verdict_kernel: on a block whose verdict is
not UNKNOWN a wave reads the verdict and ends, as rs_heal_kernel does on a block without a culprit;
on an UNKNOWN block it runs Verify's pipeline once more and the pair tests on every dirty tile.
RS(10,4), 4096 blocks of 256 KiB, device-resident rows at rsmi_recommended_pitch(S), HIP-event
timed, the method of tools/heal_ab.py: every call runs untimed for --settle-ms first, then per
alternation 3 warm-up launches and the median of 20 launches of locate, heal and pair in turn, six
alternations.  The baselines are the same build's rsmi_locate_batch_dev and rsmi_heal_batch_dev.

  (a) clean stripes: the pair kernel exits early everywhere
  (b) data row 0 of every block stale: locate names shard 0, the pair kernel exits early, heal
      rewrites the row; it is damaged again before every launch of every call, outside the timed
      interval
  (c) data rows 0 and 1 of every block stale: locate and heal say UNKNOWN, the pair kernel tests
      every tile of every block and names (0, 1)

The bar: in (a) and (b) the pair call may take no longer than heal's clean-stripe call (case (a))
plus the wider of the two legs' spreads of medians.  (c) is reported, not gated.

  python tools/locate_pair_ab.py [--cases abc] [--alternations 6] [--launches 20] [--warmup 3]
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
    emit("# locate vs heal vs locate_pair, RS(%d,%d) %d x %d KiB, device-resident, rows at rsmi_recommended_pitch, "
         "median of %d launches after %d warm-ups, %d alternations, %d ms settle; TB/s over (k+m)*S*blocks payload bytes"
         % (k, m, nb, block >> 10, args.launches, args.warmup, args.alternations, args.settle_ms))
    emit("# device: %s" % torch.cuda.get_device_name(0))
    d = torch.randint(0, 256, (nb * bs,), dtype=torch.uint8, device="cuda")
    bad = torch.zeros(nb * m, dtype=torch.int32, device="cuda")
    cul = torch.zeros(nb, dtype=torch.int32, device="cuda")
    pair = torch.zeros(nb, 2, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    row0 = d.view(nb, bs)[:, :S]
    row1 = d.view(nb, bs)[:, rs:rs + S]
    U = rsmi.LocateUnknown
    with rsmi.Codec(k, m, 0) as c:
        a = (d.data_ptr(), rs, bs, d.data_ptr() + k * rs, rs, bs, S, nb)

        def loc():
            c.locate_batch_dev(*a, cul.data_ptr(), bad.data_ptr(), stream)

        def heal():
            c.heal_batch_dev(*a, cul.data_ptr(), bad.data_ptr(), stream)

        def prs():
            c.locate_pair_batch_dev(*a, pair.data_ptr(), bad.data_ptr(), stream)

        c.encode_batch_dev(*a, stream)
        torch.cuda.synchronize()
        good0, good1 = row0.clone(), row1.clone()
        stale0, stale1 = good0 ^ 0x01, good1 ^ 0x02  # every byte of the row: no clean tile

        def nothing():
            pass

        def damage1():
            row0.copy_(stale0)

        def damage2():
            row0.copy_(stale0)
            row1.copy_(stale1)

        def restore():
            row0.copy_(good0)
            row1.copy_(good1)

        cases = {"a": ("a_clean", nothing, (-1, -1), -1), "b": ("b_row0_stale", damage1, (0, -1), 0),
                 "c": ("c_rows01_stale", damage2, (0, 1), U)}
        summary = {}
        for key in args.cases:
            case, prep, want_pair, want_cul = cases[key]
            restore()
            prep()
            prs()
            torch.cuda.synchronize()
            plabel = c.last_kernel()
            got = pair.cpu()
            assert bool((got[:, 0] == want_pair[0]).all()) and bool((got[:, 1] == want_pair[1]).all()), "wrong pairs"
            prep()
            loc()
            torch.cuda.synchronize()
            llabel = c.last_kernel()
            assert bool((cul == want_cul).all()), "wrong verdicts"
            t_end = time.perf_counter() + args.settle_ms / 1e3
            while time.perf_counter() < t_end:
                for fn in (loc, heal, prs):
                    prep()
                    fn()
                torch.cuda.synchronize()
            meds = {"locate": [], "heal": [], "pair": []}
            for alt in range(args.alternations):
                row = {"case": case, "k": k, "m": m, "S": S, "pitch": rs, "blocks": nb, "alternation": alt,
                       "locate_kernel": llabel, "pair_kernel": plabel}
                for what, fn in (("locate", loc), ("heal", heal), ("pair", prs)):
                    med, lo, hi = median_us(torch, fn, prep, args.warmup, args.launches)
                    meds[what].append(med)
                    row[what + "_us"] = round(med, 2)
                    row[what + "_min_us"] = round(lo, 2)
                    row[what + "_max_us"] = round(hi, 2)
                    row[what + "_TBps"] = round(payload / med / 1e6, 3)
                row["pair_over_locate"] = round(row["pair_us"] / row["locate_us"], 4)
                row["pair_over_heal"] = round(row["pair_us"] / row["heal_us"], 4)
                emit(json.dumps(row))
            summary[key] = {what: {"median_us": statistics.median(v), "spread_us": max(v) - min(v)}
                            for what, v in meds.items()}
            emit(json.dumps({"case": case, "summary": {
                what: {"median_us": round(s["median_us"], 2), "spread_us": round(s["spread_us"], 2),
                       "spread_pct": round(100 * s["spread_us"] / s["median_us"], 2)}
                for what, s in summary[key].items()},
                "pair_over_locate": round(summary[key]["pair"]["median_us"] / summary[key]["locate"]["median_us"], 4),
                "pair_over_heal": round(summary[key]["pair"]["median_us"] / summary[key]["heal"]["median_us"], 4)}))
        restore()
        if "a" in summary:
            ref = summary["a"]["heal"]
            for key in "ab":
                if key not in summary:
                    continue
                p = summary[key]["pair"]
                allow = max(ref["spread_us"], p["spread_us"])
                over = p["median_us"] - ref["median_us"]
                emit(json.dumps({"bar": cases[key][0], "pair_us": round(p["median_us"], 2),
                                 "heal_clean_us": round(ref["median_us"], 2), "over_us": round(over, 2),
                                 "allowance_us": round(allow, 2), "met": bool(over <= allow),
                                 "pair_minus_locate_us": round(p["median_us"] - summary[key]["locate"]["median_us"], 2),
                                 "heal_clean_minus_locate_clean_us": round(
                                     ref["median_us"] - summary["a"]["locate"]["median_us"], 2)}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
