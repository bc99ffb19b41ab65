"""GPU box: what the steps of LD pruning cost next to a device copy of the same bitset.

On the baseline synthetic cohort at 10k x 100k and 100k x 100k, window 50, r^2 0.2, in ONE
process, HIP-event time around each whole call (one warm-up, then the minimum and the median of
three): bits.clone() (the yardstick), transpose_sites, ld_edges (it waits for its count) and the
unrelated_set step; then ld_edges and unrelated_set again on a cohort with planted LD -- in the
site-major form every even site copied to its right neighbour, so that every such pair is an
edge (the transpose does not depend on what the bits hold).  Reports the edge count and the share
of sites kept.

usage: python tools/ld_prune_time.py [OUT]   (default: profiles/r09_ld_prune.txt is NOT touched;
                                              OUT is overwritten)
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np
import torch

import cuking_amd
from cuking_amd.synth import cohort_to_device, plan_cohort

out = open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, "w")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def timed(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    best = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        torch.cuda.synchronize()
        best.append(a.elapsed_time(b))
    return r, min(best), sorted(best)[len(best) // 2]


ctx = cuking_amd.KingContext(0)
W, R2 = 50, 0.2
for n, m in ((10_000, 100_000), (100_000, 100_000)):
    seed = 20240229
    kind, pa, pb = cohort_to_device(plan_cohort(n, seed), 0)
    bits = ctx.synth_bitset(seed, kind, pa, pb, 0, n, m)
    torch.cuda.synchronize()
    wps = cuking_amd.words_per_sample(m)
    _, clone_min, clone_med = timed(lambda: bits.clone())
    site_bits, t_min, t_med = timed(lambda: ctx.transpose_sites(bits, wps, m))
    say(f"{n} x {m}: bits.clone() {clone_min:.3f} ms min / {clone_med:.3f} median; "
        f"transpose_sites {t_min:.3f} / {t_med:.3f} ms ({bits.numel() * 8 / 1e9:.2f} GB in, "
        f"{site_bits.numel() * 8 / 1e9:.2f} GB out)")
    counts = ctx.site_counts(bits, wps).cpu().numpy().view(np.uint32)
    prio = torch.from_numpy(cuking_amd.ld_priority_host(counts, m)).to("cuda:0")
    for name in ("baseline", "every even site copied to its right neighbour"):
        if name != "baseline":
            site_bits[1::2] = site_bits[0:m - 1:2].clone()
            prio[1::2] = prio[0:m - 1:2].clone()
        (records, count), e_min, e_med = timed(lambda: ctx.ld_edges(site_bits, m, n, W, R2))
        chosen, u_min, u_med = timed(lambda: ctx.unrelated_set(records, count, m, priority=prio,
                                                               families=False))
        kept = int((chosen.keep == 1).sum())
        say(f"  {name}: ld_edges {e_min:.3f} / {e_med:.3f} ms, {count} edges; unrelated_set "
            f"{u_min:.3f} / {u_med:.3f} ms, {chosen.rounds} rounds; kept {kept} of {m} sites "
            f"({100.0 * kept / m:.2f} %)")
    del bits, site_bits, records
    torch.cuda.empty_cache()
out.close()
