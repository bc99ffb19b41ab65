"""GPU box: what the dense kinship matrix costs next to the thresholded call it shares its
four plane products with.

On the baseline synthetic cohort, in ONE process, the cases interleaved round by round
(so that clock drift and neighbours hit all of them alike), HIP-event time around each
whole call (conversion of the bitset included, as a caller sees it):

    a  compute_king, variant 6 (four products for every pair), threshold 0.0884
    b  kin_matrix, upper triangle (the context's default variant)
    b6 kin_matrix, upper triangle, variant 6 (the same kernel without the quadrant mode)
    c  kin_matrix, symmetric (b + the mirror kernel)
    d  a memset of the bytes b writes (4 B x N (N - 1) / 2): what this box takes to write them
    e  compute_counts (24 B per pair, five sums), with --counts only

Reports median and range over the timed rounds, and the relation the stores should keep:
t(b) <= 1.05 x (t(a) + t(d)).

usage: python tools/kin_matrix_time.py SAMPLES SITES [--rounds 10] [--warmup 2] [--counts]
                                       [--out FILE]   (appends to FILE)
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


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("samples", type=int)
    ap.add_argument("sites", type=int)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--counts", action="store_true")
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

    kin = torch.empty((n, n), dtype=torch.float32, device="cuda:0")
    results = torch.zeros((MAX_RESULTS, 6), dtype=torch.int32, device="cuda:0")
    index_flag = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    counts = torch.empty((n, n, 6), dtype=torch.int32, device="cuda:0") if args.counts else None
    upper_bytes = 4 * n * (n - 1) // 2
    stream = torch.cuda.current_stream().cuda_stream

    def king6():
        ctx.set_option("variant", 6)
        index_flag.zero_()
        ctx.compute_king(sm, wps, bits, THRESHOLD, MAX_RESULTS, results, index_flag[0:1],
                         index_flag[1:2])

    def kin_upper(variant):
        def call():
            ctx.set_option("variant", variant)
            ctx.kin_matrix(sm, wps, bits, out=kin)
        return call

    def kin_symmetric():
        ctx.set_option("variant", default_variant)
        ctx.kin_matrix(sm, wps, bits, out=kin, symmetric=True)

    def memset():
        cuking_amd._lib.check(ctx.lib.cuking_memset_async(ctx.handle, kin.data_ptr(), 0,
                                                          upper_bytes, stream))

    def all_counts():
        ctx.set_option("variant", default_variant)
        cuking_amd._lib.check(ctx.lib.cuking_compute_counts(
            ctx.handle, C.byref(sm.c), wps, bits.data_ptr(), counts.data_ptr(), stream))

    cases = [("a compute_king v6 thr 0.0884", king6),
             (f"b kin_matrix upper v{default_variant}", kin_upper(default_variant)),
             ("b6 kin_matrix upper v6", kin_upper(6)),
             (f"c kin_matrix symmetric v{default_variant}", kin_symmetric),
             ("d memset of b's bytes", memset)]
    if args.counts:
        cases.append((f"e compute_counts v{default_variant}", all_counts))

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

    lines = [f"# kin_matrix_time: {n} samples x {m} sites, baseline cohort seed {SEED}, "
             f"{args.warmup} warm-up + {args.rounds} timed rounds, cases interleaved, "
             f"HIP-event ms per whole call; {records} records at {THRESHOLD}; "
             f"upper triangle {upper_bytes / 1e9:.3f} GB",
             f"# device: {torch.cuda.get_device_name(0)}"]
    med = {}
    for name, _ in cases:
        t = times[name]
        med[name[:2].strip()] = statistics.median(t)
        lines.append(f"{name:36s} median {statistics.median(t):10.3f}  min {min(t):10.3f}  "
                     f"max {max(t):10.3f}")
    bound = 1.05 * (med["a"] + med["d"])
    lines.append(f"relation t(b) <= 1.05 (t(a) + t(d)): {med['b']:.3f} <= {bound:.3f}: "
                 f"{'holds' if med['b'] <= bound else 'DOES NOT HOLD'}   "
                 f"(variant 6: {med['b6']:.3f})")
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
