#!/usr/bin/env python3
"""The mixed-batch reconstruct against the uniform call, one process, one GPU.

rsmi_reconstruct_mixed_batch_dev classes the blocks on the host, uploads the class lists and
launches rs_mixed_kernel once per class.  RS(10,4), 4096 blocks of 256 KiB, device-resident rows
at rsmi_recommended_pitch(S), HIP-event timed: both legs run untimed for --settle-ms first (past
the GPU's start-up power transient), then per alternation 3 warm-up calls and the median of 20
calls, reference then mixed, six alternations.  The reference is the same build's
rsmi_reconstruct_batch_dev, whose kernels this change leaves as they were.

  (a) every block loses data row 0: the mixed call against one rsmi_reconstruct_batch_dev
  (b) every block draws one of the 14 one-lost and 91 two-lost patterns (seeded): the mixed call
      against the loop over runs of equal masks, one rsmi_reconstruct_batch_dev per run -- the
      only way to rebuild such a batch in place without this call
  (c) every block intact but one: what the mixed call costs before its first launch (classing on
      the host, the upload), as host wall time of the call, and its share of (b)'s mixed median

TB/s counts the (k + m) * S payload bytes of every block.  mixed_over_ref is the ratio of the
medians of one alternation; the spread of a leg is its medians' range over the alternations.

  python tools/mixed_ab.py [--alternations 6] [--launches 20] [--warmup 3] [--settle-ms 500] [--out FILE]
"""
import argparse
import itertools
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
    emit("# mixed vs uniform reconstruct, RS(%d,%d) %d x %d KiB, device-resident, rows at rsmi_recommended_pitch, "
         "median of %d calls after %d warm-ups, %d alternations, %d ms settle; TB/s over (k+m)*S*blocks payload bytes"
         % (k, m, nb, block >> 10, args.launches, args.warmup, args.alternations, args.settle_ms))
    emit("# device: %s" % torch.cuda.get_device_name(0))
    d = torch.randint(0, 256, (nb * bs,), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    rows = d.view(nb, n, rs)
    with rsmi.Codec(k, m, 0) as c:
        c.encode_batch_dev(d.data_ptr(), rs, bs, d.data_ptr() + k * rs, rs, bs, S, nb, stream)
        torch.cuda.synchronize()
        good = d.clone()

        # (a) one pattern
        pa = np.ones((nb, n), dtype=np.uint8)
        pa[:, 0] = 0
        # (b) a seeded draw over the one-lost and two-lost patterns
        pats = [(i,) for i in range(n)] + list(itertools.combinations(range(n), 2))
        assert len(pats) == 14 + 91
        draw = np.random.default_rng(0xA11B).integers(0, len(pats), size=nb)
        pb = np.ones((nb, n), dtype=np.uint8)
        for b in range(nb):
            pb[b, list(pats[draw[b]])] = 0
        runs = []  # (first block, blocks, present flags) per run of equal masks
        b = 0
        while b < nb:
            e = b + 1
            while e < nb and draw[e] == draw[b]:
                e += 1
            runs.append((b, e - b, [bool(x) for x in pb[b]]))
            b = e
        # (c) one lossy block
        pc = np.ones((nb, n), dtype=np.uint8)
        pc[nb // 2, 3] = 0

        def mixed(p, data_only):
            return lambda: c.reconstruct_mixed_batch_dev(d.data_ptr(), rs, bs, S, nb, p.ctypes.data, None, data_only,
                                                         stream, status=False)

        def ref_a():
            c.reconstruct_batch_dev(d.data_ptr(), rs, bs, S, nb, [i != 0 for i in range(n)], True, stream)

        def ref_b():
            for b0, cnt, flags in runs:
                c.reconstruct_batch_dev(d.data_ptr() + b0 * bs, rs, bs, S, cnt, flags, False, stream)

        medians = {}
        for case, ref, mix, p in (("a_one_pattern", ref_a, mixed(pa, True), pa),
                                  ("b_105_patterns", ref_b, mixed(pb, False), pb)):
            # both legs rebuild the rows they are told are missing: damaged first, compared after
            for leg in (ref, mix):
                rows[:, :, :S][torch.from_numpy(p == 0).cuda()] = 0x5C
                leg()
                torch.cuda.synchronize()
                assert torch.equal(d, good), "%s: wrong bytes" % case
            mix()
            torch.cuda.synchronize()
            mlabel = c.last_kernel()
            ref()
            torch.cuda.synchronize()
            rlabel = c.last_kernel()
            t_end = time.perf_counter() + args.settle_ms / 1e3
            while time.perf_counter() < t_end:
                ref()
                mix()
                torch.cuda.synchronize()
            meds = {"ref": [], "mixed": []}
            for alt in range(args.alternations):
                row = {"case": case, "k": k, "m": m, "S": S, "pitch": rs, "blocks": nb, "alternation": alt,
                       "ref_calls": 1 if ref is ref_a else len(runs), "ref_kernel": rlabel, "mixed_kernel": mlabel}
                for what, fn in (("ref", ref), ("mixed", mix)):
                    med, lo, hi = median_us(torch, fn, args.warmup, args.launches)
                    meds[what].append(med)
                    row[what + "_us"] = round(med, 2)
                    row[what + "_min_us"] = round(lo, 2)
                    row[what + "_max_us"] = round(hi, 2)
                    row[what + "_TBps"] = round(payload / med / 1e6, 3)
                row["mixed_over_ref"] = round(row["mixed_us"] / row["ref_us"], 4)
                emit(json.dumps(row))
            medians[case] = statistics.median(meds["mixed"])
            emit(json.dumps({"case": case, "summary": {
                what: {"median_us": round(statistics.median(v), 2), "spread_us": round(max(v) - min(v), 2),
                       "spread_pct": round(100 * (max(v) - min(v)) / statistics.median(v), 2)}
                for what, v in meds.items()},
                "mixed_over_ref": round(statistics.median(meds["mixed"]) / statistics.median(meds["ref"]), 4)}))
            assert torch.equal(d, good), "%s: wrong bytes after the timed calls" % case

        # (c) host wall time of a call that classes 4096 blocks, uploads one entry and launches one tile row
        one = mixed(pc, False)
        for _ in range(args.warmup):
            one()
        torch.cuda.synchronize()
        meds = []
        for alt in range(args.alternations):
            times = []
            for _ in range(args.launches):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                one()
                times.append((time.perf_counter() - t0) * 1e6)
            meds.append(statistics.median(times))
        pre = statistics.median(meds)
        emit(json.dumps({"case": "c_one_lossy_block", "blocks": nb, "kernel": c.last_kernel(),
                         "host_call_us": round(pre, 2), "spread_us": round(max(meds) - min(meds), 2),
                         "share_of_b_mixed_pct": round(100 * pre / medians["b_105_patterns"], 2),
                         "share_of_a_mixed_pct": round(100 * pre / medians["a_one_pattern"], 2)}))
        torch.cuda.synchronize()
        assert torch.equal(d, good)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
