"""GPU box: what the genotype matrix products cost next to a device copy of the same bitset.

At 10k x 100k and 100k x 100k, in ONE process, HIP-event time around each call (two warm-ups,
then the median and the minimum of seven): bits.clone() (the yardstick), Z B on the sample-major
bitset with 64 and with 32 right-hand sides (per-column table), Z^T A on a site-major bitset of
the same shape with 64 (per-row table).  The bitset words are random (the kernel's time does not
depend on what the bits hold), table and right-hand sides standard normal.  One JSON line per
measurement; tflops = 2 rows cols rhs / median.

usage: python tools/geno_matmul_time.py [OUT]   (default: profiles/r11_geno_matmul.txt is NOT
                                                 touched; OUT is overwritten)
"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np
import torch

import cuking_amd

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
for n, m in ((10_000, 100_000), (100_000, 100_000)):
    wps = cuking_amd.words_per_sample(m)
    bits = torch.randint(-2**62, 2**62, (n, wps), dtype=torch.int64, device="cuda:0")
    table = torch.randn((m, 4), device="cuda:0")
    clone = timed(lambda: bits.clone())
    for rhs in (64, 32):
        b = torch.randn((m, rhs), device="cuda:0")
        res = torch.empty((n, rhs), device="cuda:0")
        med, low = timed(lambda: ctx.geno_matmul(bits, wps, m, table, b, out=res))
        say(dict(op="Z B per column", rows=n, cols=m, rhs=rhs, median_ms=med, min_ms=low,
                 tflops=2.0 * n * m * rhs / med / 1e9, clone_median_ms=clone[0],
                 bitset_gb=n * wps * 8 / 1e9))
    # the site-major form of a cohort of the same shape: rows = sites, columns = samples
    q2 = 2 * cuking_amd.ld_site_words(n)
    site_bits = torch.randint(-2**62, 2**62, (m, q2), dtype=torch.int64, device="cuda:0")
    a = torch.randn((n, 64), device="cuda:0")
    res = torch.empty((m, 64), device="cuda:0")
    med, low = timed(lambda: ctx.geno_matmul(site_bits, q2, n, table, a, per_row=True, out=res))
    say(dict(op="Z^T A per row", rows=m, cols=n, rhs=64, median_ms=med, min_ms=low,
             tflops=2.0 * n * m * 64 / med / 1e9))
    del bits, site_bits
    torch.cuda.empty_cache()
out.close()
