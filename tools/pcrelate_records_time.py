"""GPU box: what the PC-Relate record scan of a diagonal block costs next to the matrix of the
same block.

On the synthetic `admixed` bitset of 10k x 100k, in ONE process, HIP-event time around each call
(two warm-ups, then the median and the minimum of seven): the 8192 x 8192 diagonal block with d = 3
and d = 11 columns of X -- `pcrelate_records_raw` at min_kin = 0.0442 into a buffer of exactly
its count, and at min_kin = -inf as a counting call (max_records = 0: every pair with a defined
kinship is counted, nothing is stored) -- against `pcrelate_matrix` of the same block and
`bits.clone()` of the whole bitset.  The record calls wait for their stream and read the count
back; that is inside their time.  X = [1, standard normal scores], beta = [2 p, small normal] as
in tools/pcrelate_time.py: the kernel body is branchless, its time does not depend on what they
hold, but the NUMBER of records does, and it is printed.  `tile_share` is what the tile counts
alone predict: 2080 of the matrix call's 4096 tiles = 0.51.  One JSON line per measurement.

usage: python tools/pcrelate_records_time.py [OUT]   (OUT is overwritten; default: nothing is
written)
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
n, m, block = 10_000, 100_000, (0, 8192, 0, 8192)
wps = cuking_amd.words_per_sample(m)
kind, pa, pb = cohort_to_device(plan_cohort(n, SEED))
bits = ctx.synth_bitset(SEED, kind, pa, pb, 0, n, m, model="admixed")
torch.cuda.synchronize()
rows = block[1] - block[0]
tiles = (rows + 127) // 128
tile_share = (tiles * (tiles + 1) // 2) / (tiles * tiles)
clone = timed(lambda: bits.clone())
res = torch.empty((rows, rows), device="cuda:0")
rng = np.random.default_rng(SEED)
for d in (3, 11):
    x = np.ones((n, d), dtype=np.float32)
    x[:, 1:] = rng.standard_normal((n, d - 1))
    beta = np.empty((m, d), dtype=np.float32)
    beta[:, 0] = 2.0 * rng.uniform(0.05, 0.95, size=m)
    beta[:, 1:] = rng.normal(0.0, 0.03, size=(m, d - 1))
    d_x, d_beta = torch.from_numpy(x).to("cuda:0"), torch.from_numpy(beta).to("cuda:0")
    args = (bits, wps, m, d_x, d_beta, 0.01, 0.99)
    matrix = timed(lambda: ctx.pcrelate_matrix(*args, block=block, out=res))
    say(dict(op="pcrelate_matrix", samples=n, sites=m, block=block, d=d, median_ms=matrix[0],
             min_ms=matrix[1], clone_median_ms=clone[0]))

    def count_only(min_kin):
        try:
            return ctx.pcrelate_records_raw(*args, min_kin, block=block, max_records=0)[1]
        except cuking_amd.ResourceExhaustedError as e:
            return e.num_records

    for min_kin, counting in ((0.0442, False), (float("-inf"), True)):
        count = count_only(min_kin)
        if counting:
            med, low = timed(lambda: count_only(min_kin))
        else:
            buf = torch.empty((max(count, 1), 6), dtype=torch.int32, device="cuda:0")
            med, low = timed(lambda: ctx.pcrelate_records_raw(*args, min_kin, block=block,
                                                              max_records=count, out=buf))
        say(dict(op="pcrelate_records", samples=n, sites=m, block=block, d=d,
                 min_kin=str(min_kin), counting_call=counting, num_records=count,
                 median_ms=med, min_ms=low, matrix_median_ms=matrix[0],
                 share_of_matrix=med / matrix[0], tile_share=tile_share,
                 estimate_ms=tile_share * matrix[0], clone_median_ms=clone[0]))
out.close()
