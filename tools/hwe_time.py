"""GPU box: what the Hardy-Weinberg exact test of every site costs next to the site counts it
reads, a copy of the bitset, and the host twin on the same rows.

On the synthetic bitsets of 10k x 100k and 100k x 100k (baseline model) and on the exome model at
100k x 100k (most sites rare: short walks, lanes of a wavefront far apart), in ONE process,
HIP-event time around each call (warm-ups, then the median and the minimum of seven):
`bits.clone()` and `site_counts` as the yardsticks, then `hwe_sites` on the counts, without and with
mid-p.  The host twin `hwe_sites_host` runs once on the same rows (wall clock, one thread) and its
bytes are compared with the device's.  Walk steps per site and per wavefront (the longest of its 64
sites) are counted with the Python restatement of tests/hwe_cases.py on the first 6400 sites.  One
JSON line per measurement.  The registers and occupancy of the kernel come from the build (`python
-m cuking_amd.build --lib --force --save-temps`), not from this tool.

usage: python tools/hwe_time.py [OUT]
       (OUT is overwritten; default: nothing is written)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

import cuking_amd
import hwe_cases
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
SEED, STEP_SITES = 7, 6400
for model, n, m in (("baseline", 10_000, 100_000), ("baseline", 100_000, 100_000),
                    ("exome", 100_000, 100_000)):
    wps = cuking_amd.words_per_sample(m)
    kind, pa, pb = cohort_to_device(plan_cohort(n, SEED))
    bits = ctx.synth_bitset(SEED, kind, pa, pb, 0, n, m, model=model)
    torch.cuda.synchronize()
    where = dict(model=model, samples=n, sites=m)
    clone = timed(lambda: bits.clone())
    say(dict(op="clone", **where, median_ms=clone[0], min_ms=clone[1],
             bitset_gb=n * wps * 8 / 1e9))
    counts = ctx.site_counts(bits, wps)
    scratch = torch.zeros_like(counts)
    count = timed(lambda: ctx.site_counts(bits, wps, out=scratch))
    say(dict(op="site_counts", **where, median_ms=count[0], min_ms=count[1]))
    host_counts = counts.cpu().numpy().view(np.uint32)
    steps = np.array([sum(hwe_cases.hwe_walk(int(a), int(b), int(c))[1:3])
                      for a, b, c, _ in host_counts[:STEP_SITES]])
    waves = steps.reshape(-1, 64).max(axis=1)
    say(dict(op="steps", **where, counted_sites=STEP_SITES, mean_per_site=float(steps.mean()),
             max_per_site=int(steps.max()), mean_wavefront_max=float(waves.mean()),
             lane_use=float(steps.sum() / (64.0 * waves.sum()))))
    p = torch.empty(m, dtype=torch.float64, device="cuda:0")
    for midp in (False, True):
        med, low = timed(lambda: ctx.hwe_sites(counts, m, midp=midp, out=p))
        t0 = time.perf_counter()
        host_p = cuking_amd.hwe_sites_host(host_counts, m, midp=midp)
        host_ms = (time.perf_counter() - t0) * 1e3
        same = bool((hwe_cases.bits(p.cpu().numpy()) == hwe_cases.bits(host_p)).all())
        say(dict(op="hwe_sites", **where, midp=midp, median_ms=med, min_ms=low,
                 ns_per_site=med * 1e6 / m, vs_clone=med / clone[0],
                 vs_site_counts=med / count[0], host_ms=host_ms, host_over_device=host_ms / med,
                 equals_host_bytes=same, below_1e_6=int((host_p < 1e-6).sum())))
    del bits, counts, scratch, p
    torch.cuda.empty_cache()
out.close()
