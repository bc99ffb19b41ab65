"""GPU box: what site QC costs next to a device copy of the same bitset.

On the baseline synthetic cohort, in ONE process and on the same bitset, the cases interleaved
round by round (so that clock drift and neighbours hit all of them alike), HIP-event time
around each call:

    copy     bits.clone(): reads S x wps x 8 bytes and writes as many -- the yardstick
    counts   site_counts (one read of the bitset, atomics into 16 B per site)
    samples  sample_counts (one read)
    half     compact_sites with a random mask of density 0.5 (one read, half a write)
    rule     compact_sites with the mask of min_call_rate 0.95 / min_maf 0.01

(compact_sites includes the upload of the mask's table and the wait for it.)  Reports the
medians, the range and the ratios to the copy.  With --records also the records pass
(compute_king at 0.0884, conversion included) on the unfiltered and on the rule-filtered
bitset: what the filter buys downstream.

usage: python tools/site_qc_time.py SAMPLES SITES [--rounds 10] [--warmup 2] [--records]
                                    [--out FILE]   (appends)
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np
import torch

import cuking_amd
from cuking_amd.synth import cohort_to_device, plan_cohort

SEED = 20240229
THRESHOLD = 0.0884
MAX_RESULTS = 10 << 20


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("samples", type=int)
    ap.add_argument("sites", type=int)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--records", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    n, m = args.samples, args.sites

    ctx = cuking_amd.KingContext(0)
    kind, pa, pb = cohort_to_device(plan_cohort(n, SEED))
    bits = ctx.synth_bitset(SEED, kind, pa, pb, 0, n, m)
    wps = bits.shape[1]
    torch.cuda.synchronize()

    counts = ctx.site_counts(bits, wps)
    host_counts = counts.cpu().numpy().view(np.uint32)
    rule, rule_kept = cuking_amd.site_mask_host(host_counts, m, 0.95, 0.01, 0)
    half = cuking_amd.site_mask_words(np.random.default_rng(SEED).random(m) < 0.5)
    half_kept = int(cuking_amd.site_mask_bool(half, m).sum())
    out_half = torch.empty((n, cuking_amd.words_per_sample(half_kept)), dtype=torch.int64,
                           device="cuda:0")
    out_rule = torch.empty((n, cuking_amd.words_per_sample(rule_kept)), dtype=torch.int64,
                           device="cuda:0")
    per_sample = torch.empty((n, 4), dtype=torch.int32, device="cuda:0")
    keep = {}

    def copy():
        keep["clone"] = bits.clone()

    cases = {
        "copy": copy,
        "counts": lambda: ctx.site_counts(bits, wps, out=counts),
        "samples": lambda: ctx.sample_counts(bits, wps, m, out=per_sample),
        "half": lambda: ctx.compact_sites(bits, wps, half, m, out=out_half),
        "rule": lambda: ctx.compact_sites(bits, wps, rule, m, out=out_rule),
    }
    sm = cuking_amd.Submatrix(n)
    if args.records:
        results = torch.zeros((MAX_RESULTS, 6), dtype=torch.int32, device="cuda:0")
        index_flag = torch.zeros(2, dtype=torch.int32, device="cuda:0")

        def records(b, w):
            def call():
                index_flag.zero_()
                ctx.invalidate()
                ctx.compute_king(sm, w, b, THRESHOLD, MAX_RESULTS, results, index_flag[0:1],
                                 index_flag[1:2])
            return call
        cases["records, unfiltered"] = records(bits, wps)
        cases["records, rule-filtered"] = records(out_rule, out_rule.shape[1])

    times = {name: [] for name in cases}
    for rnd in range(args.warmup + args.rounds):
        for name, call in cases.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            call()
            stop.record()
            stop.synchronize()
            if rnd >= args.warmup:
                times[name].append(start.elapsed_time(stop))
    torch.cuda.synchronize()

    gb = n * wps * 8 / 1e9
    lines = [f"# tools/site_qc_time.py {n} {m}: baseline cohort seed {SEED}, bitset {gb:.3f} GB "
             f"(wps {wps}), {args.warmup} warm-up + {args.rounds} interleaved rounds, HIP events "
             "around each call",
             f"# device: {torch.cuda.get_device_name(0)}; mask `half` keeps {half_kept} sites, "
             f"`rule` (call rate 0.95, maf 0.01) keeps {rule_kept} of {m}"]
    base = statistics.median(times["copy"])
    for name, t in times.items():
        med = statistics.median(t)
        lines.append(f"{name:24s} median {med:9.3f} ms  min {min(t):9.3f}  max {max(t):9.3f}"
                     f"  = {med / base:5.2f} x copy")
    if args.records:
        lines.append(f"# records found: {int(index_flag[0])} on the filtered bitset (last call)")
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
