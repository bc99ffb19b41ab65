"""GPU box: what the IBD scan of a block costs next to two things that were there before it.

In ONE process, HIP-event time around each call (warm-ups, then the median and the minimum of
seven), on the synthetic bitsets of 10k x 100k and 100k x 100k:

  clone     `bits.clone()`, the yardstick of every profile here;
  listed    `ibd_segments_raw` (strict, no segment list) over the EXPLICIT list of all i < j of
            the 8192 x 8192 diagonal block of the 10k cohort: 33.5 M pairs, 268 MB of list and
            1.34 GB of rows -- what the scan replaces;
  scan      `ibd_scan_raw` over the same block (min_sites = 512, the default buffer), and over
            the 16384 x 16384 diagonal block of the 100k cohort.  The call reads its count back,
            so that wait is inside the time.  `peak_bytes` is what the call allocated at its
            peak (torch's allocator; the context's scratch is the group mask and one counter).

One JSON line per measurement with ns per pair.  The scan is never compared with itself.
`--whole` adds ONE counting call (max_records = 0) over the whole 100k x 100k diagonal block,
timed by the wall clock; run it under a time limit of its own.  The registers and occupancy of
the kernel come from the build (`python -m cuking_amd.build --lib --force --save-temps`), not
from this tool.

usage: python tools/ibd_scan_time.py [--whole] [OUT]
       (OUT is overwritten; default: nothing is written)
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np
import torch

import cuking_amd
from cuking_amd.synth import cohort_to_device, plan_cohort

parser = argparse.ArgumentParser()
parser.add_argument("out", nargs="?", default=os.devnull)
parser.add_argument("--whole", action="store_true")
args = parser.parse_args()
out = open(args.out, "w")


def say(record):
    line = json.dumps(record)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def timed(fn, reps=7, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(min(times))


def cohort(n, m):
    kind, pa, pb = cohort_to_device(plan_cohort(n, SEED))
    bits = ctx.synth_bitset(SEED, kind, pa, pb, 0, n, m)
    torch.cuda.synchronize()
    med, low = timed(lambda: bits.clone())
    say(dict(op="clone", samples=n, sites=m, median_ms=med, min_ms=low,
             bitset_gb=n * wps * 8 / 1e9))
    return bits


def scan(bits, n, side):
    pairs = side * (side - 1) // 2
    found = []
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    med, low = timed(lambda: found.append(ctx.ibd_scan_raw(bits, wps, m,
                                                           block=(0, side, 0, side))[1]))
    peak = torch.cuda.max_memory_allocated() - before
    say(dict(op="ibd_scan", samples=n, block=side, pairs=pairs, min_sites=512,
             records=found[-1], median_ms=med, min_ms=low, ns_per_pair=med * 1e6 / pairs,
             peak_bytes=peak))


ctx = cuking_amd.KingContext(0)
SEED = 7
m = 100_000
wps = cuking_amd.words_per_sample(m)

# ---- the 8192 x 8192 diagonal block of 10k x 100k: the listed call, then the scan
n, side = 10_000, 8192
bits = cohort(n, m)
i, j = torch.triu_indices(side, side, offset=1, device="cuda:0")
d_pairs = torch.stack([i, j], dim=1).to(torch.int32).contiguous()
del i, j
pairs = d_pairs.shape[0]
rows = torch.empty((pairs, 10), dtype=torch.int32, device="cuda:0")
med, low = timed(lambda: ctx.ibd_segments_raw(bits, wps, m, d_pairs, out=rows))
have = int((rows[:, 2] > 0).sum())
say(dict(op="ibd_segments", samples=n, block=side, pairs=pairs, min_sites=512,
         pairs_with_a_segment=have, median_ms=med, min_ms=low, ns_per_pair=med * 1e6 / pairs,
         list_and_rows_bytes=pairs * 48))
del d_pairs, rows
scan(bits, n, side)
del bits
torch.cuda.empty_cache()

# ---- the 16384 x 16384 diagonal block of 100k x 100k
n, side = 100_000, 16384
bits = cohort(n, m)
scan(bits, n, side)

if args.whole:
    torch.cuda.synchronize()
    start = time.perf_counter()
    try:
        ctx.ibd_scan_raw(bits, wps, m, max_records=0)
        count = 0
    except cuking_amd.ResourceExhaustedError as e:
        count = e.num_records
    seconds = time.perf_counter() - start
    pairs = n * (n - 1) // 2
    say(dict(op="ibd_scan_count", samples=n, block=n, pairs=pairs, min_sites=512, records=count,
             seconds=seconds, ns_per_pair=seconds * 1e9 / pairs))
out.close()
