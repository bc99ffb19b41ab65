"""GPU box: what counting the Mendelian errors of a list of trios costs next to a copy of the
bitset it reads.

On the synthetic bitsets of 10k x 100k and 100k x 100k, in ONE process, HIP-event time around each
call (warm-ups, then the median and the minimum of seven): `bits.clone()` as the yardstick, then
10^3, 10^4 and 10^5 random trios (child, father and mother drawn from all samples) through
`mendel_errors_raw` -- rows only: one launch, no mask -- and with the site counts the way
`KingContext.mendel_errors` runs them: chunks of trios through one mask buffer of at most 64 MB,
`mendel_errors_raw` with the mask and `mendel.site_counts_device` per chunk, no wait in between.
The list is on the device beforehand.  One JSON line per measurement with ns per trio, the bytes
the rows call reads (three samples, two planes), the rate that makes and `vs_clone`, its median
over the clone's.  The registers and occupancy of the kernels come from the build (`python -m
cuking_amd.build --lib --force --save-temps`), not from this tool.

usage: python tools/mendel_time.py [OUT]
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
from cuking_amd import mendel
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
SEED = 7
for n, m in ((10_000, 100_000), (100_000, 100_000)):
    wps = cuking_amd.words_per_sample(m)
    plane = wps // 2
    kind, pa, pb = cohort_to_device(plan_cohort(n, SEED))
    bits = ctx.synth_bitset(SEED, kind, pa, pb, 0, n, m)
    torch.cuda.synchronize()
    clone = timed(lambda: bits.clone())
    say(dict(op="clone", samples=n, sites=m, median_ms=clone[0], min_ms=clone[1],
             bitset_gb=n * wps * 8 / 1e9))
    step = mendel._chunk_rows(plane, None)
    for count in (1_000, 10_000, 100_000):
        rng = np.random.default_rng(count)
        trios = torch.from_numpy(rng.integers(0, n, size=(count, 3)).astype(np.int32)).to("cuda:0")
        rows = torch.empty((count, 12), dtype=torch.int32, device="cuda:0")
        mask = torch.empty((min(step, count), plane), dtype=torch.int64, device="cuda:0")
        counts = torch.zeros(64 * plane, dtype=torch.int32, device="cuda:0")
        read_bytes = count * 3 * 2 * ((m + 63) // 64) * 8   # (the planes up to num_sites)

        def rows_only():
            ctx.mendel_errors_raw(bits, wps, m, trios, out=rows)

        def with_sites():
            for lo in range(0, count, step):
                k = min(step, count - lo)
                ctx.mendel_errors_raw(bits, wps, m, trios[lo:lo + k], error_bits=mask[:k],
                                      out=rows[lo:lo + k])
                mendel.site_counts_device(ctx, mask[:k], counts)

        for name, fn in (("rows", rows_only), ("rows_and_site_counts", with_sites)):
            med, low = timed(fn)
            say(dict(op="mendel_errors", form=name, samples=n, sites=m, trios=count,
                     chunks=1 if name == "rows" else -(-count // step),
                     errors=int(mendel.rows_to_host(rows)["errors"].sum()), median_ms=med,
                     min_ms=low, ns_per_trio=med * 1e6 / count, read_gb=read_bytes / 1e9,
                     gb_per_s=read_bytes / med / 1e6, vs_clone=med / clone[0]))
        del trios, rows, mask, counts
    del bits
    torch.cuda.empty_cache()
out.close()
