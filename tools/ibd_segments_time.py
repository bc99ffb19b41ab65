"""GPU box: what the IBD segment scan of a list of pairs costs next to PC-Relate on the same list.

On the synthetic bitset of 100k x 100k, in ONE process, HIP-event time around each call
(warm-ups, then the median and the minimum of seven): `bits.clone()` as the yardstick, then for
10^4, 10^5 and 10^6 random pairs (a plain [P, 2] list) `pcrelate_pairs_raw` with d = 3 columns of
X, `ibd_segments_raw` without the segment list (asynchronous) and with it (min_sites = 512; the
call reads its count back, so that wait is inside the time).  One JSON line per measurement with
ns per pair, the bytes the scan reads per pair (4 planes x P words) and the rate that makes.
Random pairs of unrelated samples have next to no segment: the list costs its counter and the
wait, not its stores.  The registers and occupancy of the kernel come from the build (`python -m
cuking_amd.build --lib --force --save-temps`), not from this tool.

With `--bridge-sites N` the yardsticks are `bits.clone()` and the strict scan of the same process
(PC-Relate is left out): after each strict measurement the same list goes through
`ibd_segments_raw(..., bridge_sites=N)`, the bridging instantiation of the kernel, without and
with the segment list, and the record carries `vs_strict`, its median over the strict one's.

usage: python tools/ibd_segments_time.py [--bridge-sites N] [OUT]
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
parser.add_argument("--bridge-sites", type=int, default=0)
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
n, m, d = 100_000, 100_000, 3
wps = cuking_amd.words_per_sample(m)
kind, pa, pb = cohort_to_device(plan_cohort(n, SEED))
bits = ctx.synth_bitset(SEED, kind, pa, pb, 0, n, m)
torch.cuda.synchronize()
clone = timed(lambda: bits.clone())
say(dict(op="clone", samples=n, sites=m, median_ms=clone[0], min_ms=clone[1],
         bitset_gb=n * wps * 8 / 1e9))
rng = np.random.default_rng(SEED)
x = np.ones((n, d), dtype=np.float32)
x[:, 1:] = rng.standard_normal((n, d - 1))
beta = np.empty((m, d), dtype=np.float32)
beta[:, 0] = 2.0 * rng.uniform(0.05, 0.95, size=m)
beta[:, 1:] = rng.normal(0.0, 0.03, size=(m, d - 1))
d_x, d_beta = torch.from_numpy(x).to("cuda:0"), torch.from_numpy(beta).to("cuda:0")
d_f = torch.from_numpy(rng.uniform(-0.05, 0.05, size=n).astype(np.float32)).to("cuda:0")
bytes_per_pair = 4 * ((m + 63) // 64) * 8
for p in (10_000, 100_000, 1_000_000):
    d_pairs = torch.from_numpy(rng.integers(0, n, size=(p, 2)).astype(np.int32)).to("cuda:0")
    warm = 2 if p < 1_000_000 else 1
    if not args.bridge_sites:
        rows = torch.empty((p, 8), dtype=torch.int32, device="cuda:0")
        med, low = timed(lambda: ctx.pcrelate_pairs_raw(bits, wps, m, d_x, d_beta, 0.01, 0.99,
                                                        d_pairs, d_f, out=rows), warm=warm)
        say(dict(op="pcrelate_pairs", pairs=p, d=d, median_ms=med, min_ms=low,
                 ns_per_pair=med * 1e6 / p))
    rows = torch.empty((p, 10), dtype=torch.int32, device="cuda:0")
    for with_list in (False, True):
        strict_ms = None
        for bridge in (0, args.bridge_sites) if args.bridge_sites else (0,):
            found = []

            def scan():
                found.append(ctx.ibd_segments_raw(bits, wps, m, d_pairs, segments=with_list,
                                                  out=rows, bridge_sites=bridge)[2])
            med, low = timed(scan, warm=warm)
            record = dict(op="ibd_segments", pairs=p, segment_list=with_list, min_sites=512,
                          segments_found=found[-1], median_ms=med, min_ms=low,
                          ns_per_pair=med * 1e6 / p, bytes_per_pair=bytes_per_pair,
                          gb_per_s=bytes_per_pair * p / med / 1e6)
            if args.bridge_sites:
                record["bridge_sites"] = bridge
            if bridge:
                record["vs_strict"] = med / strict_ms
            else:
                strict_ms = med
            say(record)
out.close()
