"""GPU box: what PC-Relate on a list of pairs costs next to the matrix of a block.

On the synthetic `admixed` bitset of 100k x 100k, in ONE process, HIP-event time around each
call (warm-ups, then the median and the minimum of seven): `pcrelate_pairs_raw` on 10^4, 10^5 and
10^6 random pairs (a plain [P, 2] list, f given) with d = 3 and d = 11 columns of X, then
`pcrelate_matrix` on the 8192 x 8192 diagonal block of the same bitset and `bits.clone()` as the
yardstick.  X = [1, standard normal scores], beta = [2 p, small normal]: the kernels are
branchless, their time does not depend on what they hold.  One JSON line per measurement, with ns
per pair for both and, per d, the pair count at which the list stops being cheaper than the
matrix of the block (its time over the list's ns per pair at 10^6).  The registers, LDS and
occupancy of the kernel come from the build (`python -m cuking_amd.build --lib --force
--save-temps`), not from this tool.

usage: python tools/pcrelate_pairs_time.py [OUT]   (OUT is overwritten; default: nothing is written)
"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np
import torch

import cuking_amd
from cuking_amd.synth import cohort_to_device, plan_cohort

out = open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, "w")


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
n, m, block = 100_000, 100_000, (0, 8192, 0, 8192)
wps = cuking_amd.words_per_sample(m)
kind, pa, pb = cohort_to_device(plan_cohort(n, SEED))
bits = ctx.synth_bitset(SEED, kind, pa, pb, 0, n, m, model="admixed")
torch.cuda.synchronize()
clone = timed(lambda: bits.clone())
rng = np.random.default_rng(SEED)
d_f = torch.from_numpy(rng.uniform(-0.05, 0.05, size=n).astype(np.float32)).to("cuda:0")
lists = {p: torch.from_numpy(rng.integers(0, n, size=(p, 2)).astype(np.int32)).to("cuda:0")
         for p in (10_000, 100_000, 1_000_000)}
res = torch.empty((block[1], block[3]), device="cuda:0")
for d in (3, 11):
    x = np.ones((n, d), dtype=np.float32)
    x[:, 1:] = rng.standard_normal((n, d - 1))
    beta = np.empty((m, d), dtype=np.float32)
    beta[:, 0] = 2.0 * rng.uniform(0.05, 0.95, size=m)
    beta[:, 1:] = rng.normal(0.0, 0.03, size=(m, d - 1))
    d_x, d_beta = torch.from_numpy(x).to("cuda:0"), torch.from_numpy(beta).to("cuda:0")
    per_pair = None
    for p, d_pairs in lists.items():
        rows = torch.empty((p, 8), dtype=torch.int32, device="cuda:0")
        med, low = timed(lambda: ctx.pcrelate_pairs_raw(bits, wps, m, d_x, d_beta, 0.01, 0.99,
                                                        d_pairs, d_f, out=rows),
                         warm=2 if p < 1_000_000 else 1)
        per_pair = med * 1e6 / p
        say(dict(op="pcrelate_pairs", samples=n, sites=m, pairs=p, d=d, median_ms=med, min_ms=low,
                 ns_per_pair=per_pair, clone_median_ms=clone[0], bitset_gb=n * wps * 8 / 1e9))
    med, low = timed(lambda: ctx.pcrelate_matrix(bits, wps, m, d_x, d_beta, 0.01, 0.99,
                                                 block=block, out=res))
    entries = block[1] * block[3]
    say(dict(op="pcrelate_matrix", samples=n, sites=m, block=block, d=d, median_ms=med,
             min_ms=low, ns_per_pair=med * 1e6 / entries, clone_median_ms=clone[0],
             list_as_dear_as_this_block_at_pairs=int(med * 1e6 / per_pair)))
out.close()
