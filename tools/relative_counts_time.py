"""GPU box: what relative counts cost next to the thresholded call whose path they ride.

On the baseline synthetic cohort, in ONE process and on the same bitset, the cases
interleaved round by round (so that clock drift and neighbours hit all of them alike),
HIP-event time around each whole call (conversion of the bitset included, as a caller
sees it), on the default context and on variant 6:

    c   relative_counts, the four KING cut-offs (0.0442, 0.0884, 0.177, 0.354)
    k   compute_king at the lowest of them, 0.0442
    c6 / k6  the same two on variant 6 (four products for every pair)

Reports median and range over the timed rounds and the relation the count call should
keep: it does strictly less than the record call at thresholds[0] (no 24-byte record, no
hom/hom recount), so t(c) <= t(k) within k's own min-max spread over the rounds.  (The
record call's kernels are instruction for instruction those of the commit before relative
counts existed -- DESIGN.md 4.1c --, so k stands for that commit on the same box.)

usage: python tools/relative_counts_time.py SAMPLES SITES [--rounds 10] [--warmup 2]
                                            [--out FILE]   (appends)
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch

import cuking_amd
from cuking_amd.synth import cohort_to_device, plan_cohort

SEED = 20240229
THRESHOLDS = cuking_amd.KING_CUTOFFS
MAX_RESULTS = 10 << 20


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("samples", type=int)
    ap.add_argument("sites", type=int)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    n, m = args.samples, args.sites
    if args.rounds < 10:
        ap.error("at least 10 timed rounds")

    ctx = cuking_amd.KingContext(0)
    default_variant = ctx.get_option("variant")
    kind, pa, pb = cohort_to_device(plan_cohort(n, SEED))
    bits = ctx.synth_bitset(SEED, kind, pa, pb, 0, n, m)
    wps = bits.shape[1]
    sm = cuking_amd.Submatrix(n)
    torch.cuda.synchronize()

    results = torch.zeros((MAX_RESULTS, 6), dtype=torch.int32, device="cuda:0")
    index_flag = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    out = torch.zeros((n, len(THRESHOLDS)), dtype=torch.int32, device="cuda:0")
    last = {}

    def counts(variant):
        def call():
            ctx.set_option("variant", variant)
            out.zero_()
            last[variant] = ctx.relative_counts(sm, wps, bits, thresholds=THRESHOLDS, out=out)
        return call

    def king(variant):
        def call():
            ctx.set_option("variant", variant)
            index_flag.zero_()
            ctx.compute_king(sm, wps, bits, THRESHOLDS[0], MAX_RESULTS, results, index_flag[0:1],
                             index_flag[1:2])
        return call

    cases = [(f"c relative_counts v{default_variant}", counts(default_variant)),
             (f"k compute_king v{default_variant} thr {THRESHOLDS[0]}", king(default_variant)),
             ("c6 relative_counts v6", counts(6)),
             (f"k6 compute_king v6 thr {THRESHOLDS[0]}", king(6))]
    times = {name: [] for name, _ in cases}
    for rnd in range(args.warmup + args.rounds):
        for name, call in cases:
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            call()
            stop.record()
            stop.synchronize()
            if rnd >= args.warmup:
                times[name].append(start.elapsed_time(stop))
    records, overflow = (int(x) & 0xFFFFFFFF for x in index_flag.tolist())
    counted = last[6].num_records(0)          # (the last count call ran on variant 6)
    ctx.set_option("variant", default_variant)

    lines = [f"# relative_counts_time: {n} samples x {m} sites, baseline cohort seed {SEED}, "
             f"{args.warmup} warm-up + {args.rounds} timed rounds, cases interleaved, "
             f"HIP-event ms per whole call; thresholds {THRESHOLDS}; {records} records at "
             f"{THRESHOLDS[0]} (overflow {overflow}), the counts say {counted}",
             f"# device: {torch.cuda.get_device_name(0)}"]
    med, spread = {}, {}
    for name, _ in cases:
        t = times[name]
        key = name.split()[0]
        med[key], spread[key] = statistics.median(t), max(t) - min(t)
        lines.append(f"{name:40s} median {statistics.median(t):10.3f}  min {min(t):10.3f}  "
                     f"max {max(t):10.3f}")
    for c, k in (("c", "k"), ("c6", "k6")):
        ok = med[c] <= med[k] + spread[k]
        lines.append(f"relation t({c}) <= t({k}) + spread({k}): {med[c]:.3f} <= {med[k]:.3f} + "
                     f"{spread[k]:.3f}: {'holds' if ok else 'DOES NOT HOLD'}   "
                     f"(ratio {med[c] / med[k]:.4f})")
    lines.append(json.dumps({"samples": n, "sites": m, "median_ms": med, "records": records,
                             "counted": counted}))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
