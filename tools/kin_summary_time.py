"""GPU box: what the kinship summary costs next to the dense kinship matrix and the
thresholded call it shares its four plane products with.

On the baseline synthetic cohort, in ONE process and on the same bitset, the cases
interleaved round by round (so that clock drift and neighbours hit all of them alike),
HIP-event time around each whole call (conversion of the bitset included, as a caller
sees it):

    a  compute_king, variant 6 (four products for every pair), threshold 0.0884
    s  kin_summary, both outputs, 1536 bins (the context's default variant)
    s6 kin_summary, variant 6 (the same kernel without the quadrant mode)
    m  kin_matrix, upper triangle (default variant); left out when the matrix does not fit
       the GPU beside the bitset (or with --no-matrix)

Reports median and range over the timed rounds and the two relations the summary should
keep: t(s) <= t(m) (it writes almost nothing) and t(s) <= 1.05 t(a) (its only added cost
is one tile's LDS atomics against several hundred k-steps).

With --timers, instead: conversion and pair kernel timed SEPARATELY by the library's own
event pairs (cuking_timing_collect), case by case, the layout invalidated before every call:
matrix and summary on the default context and on variant 6, the summary with the histogram
alone, with the keys alone, and summary and matrix without remainder pieces ("split_wgs" 0).

usage: python tools/kin_summary_time.py SAMPLES SITES [--rounds 10] [--warmup 2]
                                        [--no-matrix] [--timers] [--out FILE]   (appends)
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch

import cuking_amd
from cuking_amd.synth import cohort_to_device, plan_cohort

SEED = 20240229
THRESHOLD = 0.0884
MAX_RESULTS = 10 << 20
BINS = (-1.0, 0.5, 1536)


def timers(ctx, args, sm, wps, bits, kin, hist, best, default_variant) -> str:
    """--timers: per case the library's event time of conversion and pair kernel per call."""
    n, m = args.samples, args.sites
    cbins = cuking_amd._lib.CKinBins(*BINS)
    head = (ctx.handle, C.byref(sm.c), wps, bits.data_ptr())

    def matrix():
        ctx.kin_matrix(sm, wps, bits, out=kin)

    def summary():
        ctx.kin_summary(sm, wps, bits, lo=BINS[0], hi=BINS[1], bins=BINS[2], hist=hist, best=best)

    def hist_only():
        cuking_amd._lib.check(ctx.lib.cuking_compute_kin_summary(
            *head, C.byref(cbins), hist.data_ptr(), None, None))

    def best_only():
        cuking_amd._lib.check(ctx.lib.cuking_compute_kin_summary(
            *head, None, None, best.data_ptr(), None))

    cases = [("summary", default_variant, summary, None), ("summary", 6, summary, None),
             ("summary, histogram only", default_variant, hist_only, None),
             ("summary, keys only", default_variant, best_only, None),
             ("summary, split_wgs 0", default_variant, summary, 0)]
    if kin is not None:
        cases += [("matrix", default_variant, matrix, None), ("matrix", 6, matrix, None),
                  ("matrix, split_wgs 0", default_variant, matrix, 0)]
    lines = [f"# kin_summary_time --timers: {n} samples x {m} sites, baseline cohort seed {SEED}, "
             f"{args.warmup} warm-up + {args.rounds} calls per case, layout invalidated before "
             "every call; ms per call from the library's event pairs (cuking_timing_collect)",
             f"# device: {torch.cuda.get_device_name(0)}"]
    split_wgs = ctx.get_option("split_wgs")
    ctx.timing_enable(True)
    try:
        for name, variant, call, split in cases:
            ctx.set_option("variant", variant)
            if split is not None:
                ctx.set_option("split_wgs", split)
            for rnd in range(args.warmup + args.rounds):
                if rnd == args.warmup:
                    torch.cuda.synchronize()
                    ctx.timing_reset()
                ctx.invalidate()
                call()
            torch.cuda.synchronize()
            t = ctx.timing_collect()
            ctx.set_option("split_wgs", split_wgs)
            lines.append(f"{name + ' v' + str(variant):36s} pair kernel {t.king_ms / args.rounds:9.3f}"
                         f"  conversion {t.prepare_ms / args.rounds:8.3f}")
    finally:
        ctx.timing_enable(False)
        ctx.set_option("split_wgs", split_wgs)
        ctx.set_option("variant", default_variant)
    return "\n".join(lines) + "\n"


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("samples", type=int)
    ap.add_argument("sites", type=int)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-matrix", action="store_true")
    ap.add_argument("--timers", action="store_true")
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
    hist = torch.zeros(BINS[2] + 3, dtype=torch.int64, device="cuda:0")
    best = torch.zeros(n, dtype=torch.int64, device="cuda:0")
    # (the conversion's workspace comes on top: leave it a fifth of what is free)
    free, _ = torch.cuda.mem_get_info(0)
    with_matrix = not args.no_matrix and 4 * n * n < 0.8 * free
    kin = torch.empty((n, n), dtype=torch.float32, device="cuda:0") if with_matrix else None

    def king6():
        ctx.set_option("variant", 6)
        index_flag.zero_()
        ctx.compute_king(sm, wps, bits, THRESHOLD, MAX_RESULTS, results, index_flag[0:1],
                         index_flag[1:2])

    def summary(variant):
        def call():
            ctx.set_option("variant", variant)
            hist.zero_()
            best.zero_()
            ctx.kin_summary(sm, wps, bits, lo=BINS[0], hi=BINS[1], bins=BINS[2], hist=hist,
                            best=best)
        return call

    def matrix():
        ctx.set_option("variant", default_variant)
        ctx.kin_matrix(sm, wps, bits, out=kin)

    if args.timers:
        text = timers(ctx, args, sm, wps, bits, kin, hist, best, default_variant)
        print(text, end="")
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(text)
        ctx.close()
        return 0

    cases = [("a compute_king v6 thr 0.0884", king6),
             (f"s kin_summary v{default_variant}", summary(default_variant)),
             ("s6 kin_summary v6", summary(6))]
    if with_matrix:
        cases.append((f"m kin_matrix upper v{default_variant}", matrix))

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
    records = int(index_flag[0].item())
    ctx.set_option("variant", default_variant)
    counted = int(hist.cpu().numpy().view("uint64").sum())

    lines = [f"# kin_summary_time: {n} samples x {m} sites, baseline cohort seed {SEED}, "
             f"{args.warmup} warm-up + {args.rounds} timed rounds, cases interleaved, "
             f"HIP-event ms per whole call; {records} records at {THRESHOLD}; histogram of "
             f"{BINS[2]} bins holds {counted} of {sm.NumPairs()} pairs"
             + ("" if with_matrix else "; kin_matrix left out (does not fit / --no-matrix)"),
             f"# device: {torch.cuda.get_device_name(0)}"]
    med = {}
    for name, _ in cases:
        t = times[name]
        med[name.split()[0]] = statistics.median(t)
        lines.append(f"{name:36s} median {statistics.median(t):10.3f}  min {min(t):10.3f}  "
                     f"max {max(t):10.3f}")
    ratio = med["s"] / med["a"]
    lines.append(f"relation t(s) <= 1.05 t(a): {med['s']:.3f} <= {1.05 * med['a']:.3f}: "
                 f"{'holds' if ratio <= 1.05 else 'DOES NOT HOLD'}   (ratio {ratio:.4f}; "
                 f"variant 6: {med['s6'] / med['a']:.4f})")
    if with_matrix:
        lines.append(f"relation t(s) <= t(m): {med['s']:.3f} <= {med['m']:.3f}: "
                     f"{'holds' if med['s'] <= med['m'] else 'DOES NOT HOLD'}")
    lines.append(json.dumps({"samples": n, "sites": m, "median_ms": med}))
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
