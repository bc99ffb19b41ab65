"""GPU box: what a block of the PC-Relate matrix costs next to what the project already has for
the same block.

On synthetic `admixed` bitsets, in ONE process, HIP-event time around each call (two warm-ups,
then the median and the minimum of seven): the 8192 x 8192 diagonal block of 10k x 100k and one
16384 x 16384 off-diagonal block of 100k x 100k, each with d = 3 and d = 11 columns of X, against
`kin_matrix` of the same block (KING-robust: popcounts on the fp4 path) and `bits.clone()` of the
whole bitset.  X = [1, standard normal scores], beta = [2 p, small normal]: the kernel is
branchless, its time does not depend on what they hold.  One JSON line per measurement; tflops =
4 rows cols sites / median (two products of 2 rows cols sites flops), against the 157 TF f32
matrix rate.  The registers, LDS and occupancy of the kernel come from the build
(`python -m cuking_amd.build --lib --force --save-temps`), not from this tool.

usage: python tools/pcrelate_time.py [OUT]   (OUT is overwritten; default: nothing is written)
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
for n, m, block in ((10_000, 100_000, (0, 8192, 0, 8192)),
                    (100_000, 100_000, (0, 16384, 16384, 32768))):
    wps = cuking_amd.words_per_sample(m)
    kind, pa, pb = cohort_to_device(plan_cohort(n, SEED))
    bits = ctx.synth_bitset(SEED, kind, pa, pb, 0, n, m, model="admixed")
    torch.cuda.synchronize()
    rows, cols = block[1] - block[0], block[3] - block[2]
    clone = timed(lambda: bits.clone())
    # kin_matrix takes the block's stored samples: rows first, then columns (contiguous here)
    sm = cuking_amd.Submatrix.from_ranges(*block)
    stored = bits[:max(block[1], block[3])]
    res = torch.empty((rows, cols), device="cuda:0")
    king = timed(lambda: ctx.kin_matrix(sm, wps, stored, out=res))
    say(dict(op="kin_matrix", samples=n, sites=m, block=block, median_ms=king[0], min_ms=king[1],
             clone_median_ms=clone[0], bitset_gb=n * wps * 8 / 1e9))
    rng = np.random.default_rng(SEED)
    for d in (3, 11):
        x = np.ones((n, d), dtype=np.float32)
        x[:, 1:] = rng.standard_normal((n, d - 1))
        beta = np.empty((m, d), dtype=np.float32)
        beta[:, 0] = 2.0 * rng.uniform(0.05, 0.95, size=m)
        beta[:, 1:] = rng.normal(0.0, 0.03, size=(m, d - 1))
        d_x, d_beta = torch.from_numpy(x).to("cuda:0"), torch.from_numpy(beta).to("cuda:0")
        med, low = timed(lambda: ctx.pcrelate_matrix(bits, wps, m, d_x, d_beta, 0.01, 0.99,
                                                     block=block, out=res))
        say(dict(op="pcrelate_matrix", samples=n, sites=m, block=block, d=d, median_ms=med,
                 min_ms=low, tflops=4.0 * rows * cols * m / med / 1e9,
                 share_of_157_tf=4.0 * rows * cols * m / med / 1e9 / 157.0,
                 kin_matrix_median_ms=king[0], clone_median_ms=clone[0]))
    del bits, stored, res
    torch.cuda.empty_cache()
out.close()
