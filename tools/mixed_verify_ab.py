#!/usr/bin/env python3
"""The mixed reconstruct that checksums what it reads and writes against the two calls it replaces,
one process, one GPU.

rsmi_reconstruct_mixed_batch_dev_verify rebuilds a batch in which every block has its own erasure
pattern and returns R, the raw CRC-16, of every survivor it read and every row it rebuilt, from one
read of the survivors (rs_mixed_fused_kernel, the records' combine, the scatter).  The baseline is
what gives the same words without it: rsmi_reconstruct_mixed_batch_dev_crcs with raw16 alone (the
rebuild, then the named rows pass over the rebuilt rows), then rsmi_crc_named_rows_dev over each
block's k survivors, which reads every survivor a second time.

Device-resident rows at rsmi_recommended_pitch(S); every block draws one of the n one-lost and
n (n - 1) / 2 two-lost patterns (seeded), DESIGN.md §4.7 (b)'s mix.  Both routes' bytes and raws are
compared in full before anything is timed.  HIP events around the whole route: both run untimed for
--settle-ms first, then per alternation 3 warm-up calls and the median of 20, baseline then new,
six alternations.  The criterion is on the headline shape, RS(10,4) 4096 x 256 KiB: every one of the
new route's medians below every one of the baseline's.  RS(4,2) and RS(16,4) run 256 x 4 MiB.

  python tools/mixed_verify_ab.py [--alternations 6] [--launches 20] [--warmup 3] [--settle-ms 500]
                                  [--only headline|wide|pmc] [--out FILE]

--only pmc launches the plain mixed reconstruct (rs_mixed_kernel) and the new call three times each
on the headline batch and nothing else, for a counter run of its own with no tracing beside it:
  rocprofv3 --pmc FETCH_SIZE --output-format csv -d DIR -- python tools/mixed_verify_ab.py --only pmc
(WRITE_SIZE in a second run: the two do not fit one pass) and --pmc-csv FILE sums such a run's
counter per kernel.  FETCH_SIZE reports half the bytes of a wide streaming read on gfx950, so it is
also given doubled.
"""
import argparse
import csv
import itertools
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "filedag-storage_amd"))

SHAPES = {"headline": [(10, 4, 256 << 10, 4096)], "wide": [(4, 2, 4 << 20, 256), (16, 4, 4 << 20, 256)]}


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


def pmc_table(path, emit):
    """Per kernel of a rocprofv3 counter CSV: dispatches and the counters' sums over them."""
    per = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Kernel_Name") or row.get("Kernel Name") or ""
            key = name.split("(")[0]
            d = per.setdefault(key, {"ids": set()})
            d["ids"].add(row.get("Dispatch_Id") or row.get("Dispatch Id"))
            ctr = row.get("Counter_Name") or row.get("Counter Name")
            d[ctr] = d.get(ctr, 0.0) + float(row.get("Counter_Value") or row.get("Counter Value") or 0)
    for key in sorted(per):
        if not key.startswith("void rsmi::rs_") and "rs_" not in key:
            continue
        d = per[key]
        out = {"case": "pmc", "kernel": key, "dispatches": len(d["ids"])}
        for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
            if ctr in d:
                out[ctr + "_KiB_per_dispatch"] = round(d[ctr] / len(d["ids"]), 1)
        if "FETCH_SIZE" in d:
            out["FETCH_SIZE_doubled_KiB_per_dispatch"] = round(2 * d["FETCH_SIZE"] / len(d["ids"]), 1)
        emit(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=6)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle-ms", type=int, default=500)
    ap.add_argument("--only", default="", help="headline, wide or pmc")
    ap.add_argument("--pmc-csv", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def save():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write("\n".join(lines) + "\n")

    if args.pmc_csv:
        emit("# counters of %s: KiB per dispatch (the counters count in KiB on this part)" % os.path.basename(args.pmc_csv))
        pmc_table(args.pmc_csv, emit)
        save()
        return

    import numpy as np
    import torch

    import rsmi

    assert torch.cuda.is_available(), "needs a GPU"
    shapes = SHAPES["headline"] if args.only in ("headline", "pmc") else SHAPES["wide"] if args.only == "wide" else \
        SHAPES["headline"] + SHAPES["wide"]
    emit("# mixed reconstruct with checksums of the rows read and written: rsmi_reconstruct_mixed_batch_dev_verify "
         "against rsmi_reconstruct_mixed_batch_dev_crcs (raw16) + rsmi_crc_named_rows_dev over the k survivors; "
         "device-resident, rows at rsmi_recommended_pitch, seeded one- and two-lost patterns, median of %d calls after "
         "%d warm-ups, %d alternations, %d ms settle; TB/s over (k+m)*S*blocks payload bytes"
         % (args.launches, args.warmup, args.alternations, args.settle_ms))
    emit("# device: %s" % torch.cuda.get_device_name(0))
    stream = torch.cuda.current_stream().cuda_stream
    for k, m, block, nb in shapes:
        S = (block + k - 1) // k
        rs = rsmi.recommended_pitch(S)
        n = k + m
        bs = n * rs
        payload = n * S * nb
        d = torch.randint(0, 256, (nb * bs,), dtype=torch.uint8, device="cuda")
        rows = d.view(nb, n, rs)
        with rsmi.Codec(k, m, 0) as c:
            c.encode_batch_dev(d.data_ptr(), rs, bs, d.data_ptr() + k * rs, rs, bs, S, nb, stream)
            torch.cuda.synchronize()
            good = d.clone()
            pats = [(i,) for i in range(n)] + list(itertools.combinations(range(n), 2))
            draw = np.random.default_rng(0xA11B).integers(0, len(pats), size=nb)
            p = np.ones((nb, n), dtype=np.uint8)
            for b in range(nb):
                p[b, list(pats[draw[b]])] = 0
            surv = np.array([np.flatnonzero(p[b])[:k] for b in range(nb)], dtype=np.int32)
            d_surv = torch.from_numpy(surv.reshape(-1)).cuda()
            new_raw = torch.zeros(nb * n, dtype=torch.int32, device="cuda")
            old_raw = torch.zeros(nb * n, dtype=torch.int32, device="cuda")
            old_in = torch.zeros(nb * k, dtype=torch.int32, device="cuda")

            def new():
                c.reconstruct_mixed_batch_dev_verify(d.data_ptr(), rs, bs, S, nb, p.ctypes.data, None, False,
                                                     new_raw.data_ptr(), stream, status=False)

            def old():
                c.reconstruct_mixed_batch_dev_crcs(d.data_ptr(), rs, bs, S, nb, p.ctypes.data, None, False,
                                                   old_raw.data_ptr(), 0, stream, status=False)
                c.crc_named_rows_dev(d.data_ptr(), rs, bs, d.data_ptr() + k * rs, rs, bs, S, nb, d_surv.data_ptr(), k,
                                     old_in.data_ptr(), 0, stream)

            def plain():
                c.reconstruct_mixed_batch_dev(d.data_ptr(), rs, bs, S, nb, p.ctypes.data, None, False, stream,
                                              status=False)

            if args.only == "pmc":
                for leg in (plain, new):
                    for _ in range(3):
                        leg()
                    torch.cuda.synchronize()
                emit(json.dumps({"case": "pmc_run", "k": k, "m": m, "S": S, "blocks": nb, "kernel": c.last_kernel()}))
                continue

            # both routes rebuild the rows they are told are missing: damaged first, compared after
            labels = {}
            for name, leg in (("old", old), ("new", new)):
                rows[:, :, :S][torch.from_numpy(p == 0).cuda()] = 0x5C
                leg()
                torch.cuda.synchronize()
                labels[name] = c.last_kernel()
                assert torch.equal(d, good), "%s: wrong bytes" % name
            want = old_raw.cpu().numpy().reshape(nb, n).copy()
            np.put_along_axis(want, surv.astype(np.int64), old_in.cpu().numpy().reshape(nb, k), axis=1)
            got = new_raw.cpu().numpy().reshape(nb, n)
            assert np.array_equal(got, want), "the two routes' raws differ"
            assert (np.count_nonzero(want, axis=1) >= k).all()

            t_end = time.perf_counter() + args.settle_ms / 1e3
            while time.perf_counter() < t_end:
                old()
                new()
                torch.cuda.synchronize()
            meds = {"old": [], "new": []}
            for alt in range(args.alternations):
                row = {"case": "RS(%d,%d)" % (k, m), "S": S, "pitch": rs, "blocks": nb, "alternation": alt,
                       "old_last_kernel": labels["old"], "new_last_kernel": labels["new"]}
                for what, fn in (("old", old), ("new", new)):
                    med, lo, hi = median_us(torch, fn, args.warmup, args.launches)
                    meds[what].append(med)
                    row[what + "_us"] = round(med, 2)
                    row[what + "_min_us"] = round(lo, 2)
                    row[what + "_max_us"] = round(hi, 2)
                    row[what + "_TBps"] = round(payload / med / 1e6, 3)
                row["new_over_old"] = round(row["new_us"] / row["old_us"], 4)
                emit(json.dumps(row))
            emit(json.dumps({"case": "RS(%d,%d)" % (k, m), "summary": {
                what: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
                for what, v in meds.items()},
                "new_over_old": round(statistics.median(meds["new"]) / statistics.median(meds["old"]), 4),
                "every_new_below_every_old": max(meds["new"]) < min(meds["old"])}))
            assert torch.equal(d, good), "wrong bytes after the timed calls"
        del d, rows, good
        torch.cuda.empty_cache()
    save()


if __name__ == "__main__":
    main()
