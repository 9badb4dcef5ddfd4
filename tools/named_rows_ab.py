#!/usr/bin/env python3
"""The named rows pass against the routes the library had before it, one process, one GPU
(DESIGN.md §4.11).  RS(10,4), 4096 x 256 KiB, device-resident, rows at rsmi_recommended_pitch.

  (a) dense   every block names the same one row (slots 1): rsmi_crc_named_rows_dev against
              rsmi_crc16_rows_dev / rsmi_crc32_rows_dev with nrows = 1 over that row -- the same
              bytes, so the difference is what the named item source costs.  Gate: slower by at
              most three times the wider of the two ranges of the medians.
  (b) mixed   §4.7's seeded draw over the 14 one-lost and 91 two-lost patterns:
              rsmi_reconstruct_mixed_batch_dev_crcs (CRC-16) against rsmi_reconstruct_mixed_batch_dev
              followed by rsmi_crc16_rows_dev over all 14 rows.  Gate: every run of the new route
              faster than every run of the old one.
  (c) sparse  slots 2, one dirty block of 4096: the named pass alone, the price of walking 8 192
              entries.  No baseline, no gate.

HIP events around the whole route; per alternation 3 warm-ups and then the median of 20, the routes
in turn, 6 alternations.  The routes' outputs are compared whole before timing.

  python tools/named_rows_ab.py [--alternations 6] [--launches 20] [--warmup 3] [--only a|b|c|pmc] [--out FILE]

--only pmc launches the named CRC-16 pass of (b) alone, three times, for a counter run of its own
(rocprofv3 --pmc FETCH_SIZE -- python tools/named_rows_ab.py --only pmc).
"""
import argparse
import itertools
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "filedag-storage_amd"))


def timed(torch, fn, warmup, launches, before=None):
    """(median, min, max) in microseconds; before() runs outside the timed window of each launch."""
    for _ in range(warmup):
        if before:
            before()
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(launches):
        if before:
            before()
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
    ap.add_argument("--only", default="", help="a, b, c or pmc")
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
    n = k + m
    S = (block + k - 1) // k
    rs = rsmi.recommended_pitch(S)
    bs = n * rs
    emit("# named rows pass, RS(%d,%d) %d x %d KiB, S = %d at pitch %d, device-resident; median of %d after %d "
         "warm-ups, %d alternations" % (k, m, nb, block >> 10, S, rs, args.launches, args.warmup, args.alternations))
    emit("# device: %s" % torch.cuda.get_device_name(0))
    d = torch.randint(0, 256, (nb * bs,), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    dp, pp = d.data_ptr(), d.data_ptr() + k * rs
    ok = True
    with rsmi.Codec(k, m, 0) as c:
        c.encode_batch_dev(dp, rs, bs, pp, rs, bs, S, nb, stream)
        torch.cuda.synchronize()

        # ------------------------------------------------------------ (a) dense
        if args.only in ("", "a"):
            row = 3
            rows1 = torch.full((nb,), row, dtype=torch.int32, device="cuda")
            for bits in (16, 32):
                o_named = torch.full((nb,), -1, dtype=torch.int32, device="cuda")
                o_rows = torch.full((nb,), -2, dtype=torch.int32, device="cuda")

                def named():
                    c.crc_named_rows_dev(dp, rs, bs, pp, rs, bs, S, nb, rows1.data_ptr(), 1,
                                         o_named.data_ptr() if bits == 16 else 0,
                                         o_named.data_ptr() if bits == 32 else 0, stream)

                def regular():
                    f = c.crc16_rows_dev if bits == 16 else c.crc32_rows_dev
                    f(dp + row * rs, rs, bs, 1, S, nb, o_rows.data_ptr(), 1, stream)

                named()
                label = c.last_kernel()
                regular()
                torch.cuda.synchronize()
                assert torch.equal(o_named, o_rows), "the two routes' raws differ"
                meds = {"named": [], "regular": []}
                for alt in range(args.alternations):
                    r = {"case": "a_dense_crc%d" % bits, "alternation": alt, "kernel": label}
                    for what, fn in (("regular", regular), ("named", named)):
                        med, lo, hi = timed(torch, fn, args.warmup, args.launches)
                        meds[what].append(med)
                        r[what + "_us"], r[what + "_min_us"], r[what + "_max_us"] = round(med, 2), round(lo, 2), round(hi, 2)
                    emit(json.dumps(r))
                spread = max(max(v) - min(v) for v in meds.values())
                diff = statistics.median(meds["named"]) - statistics.median(meds["regular"])
                passed = diff <= 3 * spread
                ok &= passed
                emit(json.dumps({"case": "a_dense_crc%d" % bits, "gate": "named - regular <= 3 x wider range",
                                 "named_minus_regular_us": round(diff, 2), "wider_range_us": round(spread, 2),
                                 "pass": bool(passed)}))

        # ------------------------------------------------------------ (b) mixed
        pats = [(i,) for i in range(n)] + list(itertools.combinations(range(n), 2))
        draw = np.random.default_rng(0xA11B).integers(0, len(pats), size=nb)
        pb = np.ones((nb, n), dtype=np.uint8)
        for b in range(nb):
            pb[b, list(pats[draw[b]])] = 0
        lost = torch.from_numpy(pb == 0).cuda()
        view = d.view(nb, n, rs)
        raw_new = torch.full((nb * n,), -1, dtype=torch.int32, device="cuda")
        raw_old = torch.full((nb * n,), -2, dtype=torch.int32, device="cuda")

        def damage():
            view[:, :, :S][lost] = 0x5C

        def new_route():
            c.reconstruct_mixed_batch_dev_crcs(dp, rs, bs, S, nb, pb.ctypes.data, None, False, raw_new.data_ptr(), 0,
                                               stream, status=False)

        def old_route():
            c.reconstruct_mixed_batch_dev(dp, rs, bs, S, nb, pb.ctypes.data, None, False, stream, status=False)
            c.crc16_rows_dev(dp, rs, bs, n, S, nb, raw_old.data_ptr(), n, stream)

        if args.only in ("", "b"):
            good = d.clone()
            damage()
            old_route()
            torch.cuda.synchronize()
            assert torch.equal(d, good), "the old route did not rebuild the batch"
            damage()
            new_route()
            torch.cuda.synchronize()
            assert torch.equal(d, good), "the new route did not rebuild the batch"
            del good
            keep = lost.reshape(-1)
            assert torch.equal(raw_new[keep], raw_old[keep]) and not raw_new[~keep].any(), "the routes' raws differ"
            lo_old, hi_new = [], []
            for alt in range(args.alternations):
                r = {"case": "b_mixed_105_patterns", "alternation": alt}
                for what, fn in (("old", old_route), ("new", new_route)):
                    med, lo, hi = timed(torch, fn, args.warmup, args.launches, before=damage)
                    r[what + "_us"], r[what + "_min_us"], r[what + "_max_us"] = round(med, 2), round(lo, 2), round(hi, 2)
                    (lo_old if what == "old" else hi_new).append(lo if what == "old" else hi)
                r["new_over_old"] = round(r["new_us"] / r["old_us"], 4)
                emit(json.dumps(r))
            passed = max(hi_new) < min(lo_old)
            ok &= passed
            emit(json.dumps({"case": "b_mixed_105_patterns", "gate": "every new run faster than every old run",
                             "slowest_new_us": round(max(hi_new), 2), "fastest_old_us": round(min(lo_old), 2),
                             "pass": bool(passed)}))

        if args.only == "pmc":
            # the named launch of (b) alone: the rows array as launch_mixed builds it, by-slot output
            slots = 2
            e = np.full((nb, slots), -1, dtype=np.int32)
            for b in range(nb):
                e[b, :len(pats[draw[b]])] = pats[draw[b]]
            d_e = torch.from_numpy(e).cuda()
            o = torch.zeros(nb * slots, dtype=torch.int32, device="cuda")
            for _ in range(3):
                c.crc_named_rows_dev(dp, rs, bs, pp, rs, bs, S, nb, d_e.data_ptr(), slots, o.data_ptr(), 0, stream)
            torch.cuda.synchronize()
            named_bytes = int((e >= 0).sum()) * S
            emit(json.dumps({"case": "pmc", "kernel": c.last_kernel(), "named_rows": int((e >= 0).sum()),
                             "named_row_bytes": named_bytes, "all_row_bytes": nb * n * S}))

        # ------------------------------------------------------------ (c) sparse
        if args.only in ("", "c"):
            e = np.full((nb, 2), -1, dtype=np.int32)
            e[nb // 2] = (3, 11)
            d_e = torch.from_numpy(e).cuda()
            o16 = torch.zeros(nb * 2, dtype=torch.int32, device="cuda")

            def sparse():
                c.crc_named_rows_dev(dp, rs, bs, pp, rs, bs, S, nb, d_e.data_ptr(), 2, o16.data_ptr(), 0, stream)

            sparse()
            torch.cuda.synchronize()
            assert int(o16.count_nonzero()) == 2
            for alt in range(args.alternations):
                med, lo, hi = timed(torch, sparse, args.warmup, args.launches)
                emit(json.dumps({"case": "c_sparse_one_dirty_block", "alternation": alt, "entries": 2 * nb,
                                 "named_us": round(med, 2), "named_min_us": round(lo, 2), "named_max_us": round(hi, 2)}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
