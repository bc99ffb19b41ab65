"""GPU box: what the scan for runs of homozygosity of every sample costs next to a copy of the
bitset it reads.

On the synthetic bitsets of 10k x 100k and 100k x 100k, in ONE process, HIP-event time around each
call (warm-ups, then the median and the minimum of seven): `bits.clone()` as the yardstick -- it
reads the bitset once and writes it once, the scan reads it once --, then `roh_segments_raw` of
all samples (the null list), strictly and with `bridge_sites = 64`, without the segment list
(asynchronous) and with it (min_sites = 512; the call reads its count back, so that wait is inside
the time).  One JSON line per measurement with ns per sample, the bytes the scan reads, the rate
that makes and `vs_clone`, its median over the clone's; the bridged records carry `vs_strict`.
The registers and occupancy of the kernel come from the build (`python -m cuking_amd.build --lib
--force --save-temps`), not from this tool.

usage: python tools/roh_time.py [OUT]
       (OUT is overwritten; default: nothing is written)
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np
import torch

import cuking_amd
from cuking_amd.synth import cohort_to_device, plan_cohort

parser = argparse.ArgumentParser()
parser.add_argument("out", nargs="?", default=os.devnull)
args = parser.parse_args()
out = open(args.out, "w")


def say(record):
    line = json.dumps(record)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def timed(fn, reps=7, warm=2):
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


ctx = cuking_amd.KingContext(0)
SEED, BRIDGE = 7, 64
for n, m in ((10_000, 100_000), (100_000, 100_000)):
    wps = cuking_amd.words_per_sample(m)
    kind, pa, pb = cohort_to_device(plan_cohort(n, SEED))
    bits = ctx.synth_bitset(SEED, kind, pa, pb, 0, n, m)
    torch.cuda.synchronize()
    clone = timed(lambda: bits.clone())
    say(dict(op="clone", samples=n, sites=m, median_ms=clone[0], min_ms=clone[1],
             bitset_gb=n * wps * 8 / 1e9))
    read_bytes = n * 2 * ((m + 63) // 64) * 8   # (the two planes up to num_sites)
    rows = torch.empty((n, 6), dtype=torch.int32, device="cuda:0")
    for with_list in (False, True):
        strict_ms = None
        for bridge in (0, BRIDGE):
            found = []

            def scan():
                found.append(ctx.roh_segments_raw(bits, wps, m, segments=with_list, out=rows,
                                                  bridge_sites=bridge)[2])
            med, low = timed(scan)
            record = dict(op="roh_segments", samples=n, sites=m, segment_list=with_list,
                          min_sites=512, bridge_sites=bridge, segments_found=found[-1],
                          median_ms=med, min_ms=low, ns_per_sample=med * 1e6 / n,
                          read_gb=read_bytes / 1e9, gb_per_s=read_bytes / med / 1e6,
                          vs_clone=med / clone[0])
            if bridge:
                record["vs_strict"] = med / strict_ms
            else:
                strict_ms = med
            say(record)
    del bits, rows
    torch.cuda.empty_cache()
out.close()
