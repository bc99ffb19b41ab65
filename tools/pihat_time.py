"""GPU box: what the PI_HAT scan of a diagonal block costs next to a copy of its bitset, the dense
kinship matrix and the thresholded KING call on the same block.

The last 8192 samples of the 10k x 100k cohort and the last 16384 of the 100k x 100k one (baseline
model; the derived samples sit at the end), each as ONE diagonal block, in ONE process, HIP-event
time around each call (two warm-ups, then the median and the minimum of seven): `bits.clone()`,
`kin_matrix` into a tensor that is there, `compute_king` at the bench's threshold of that cohort
(0.05 / 0.0884) and at threshold 0 with no buffer (the full form on every tile, counting only: the
route the PI_HAT form takes, with the KING epilogue), then `cuking_compute_pihat` at the default
threshold with the model of the block's own samples, bounded and unbounded, and at -1 with no
buffer (every pair decided and counted, nothing stored).  Every timed call includes the
conversion of the bitset into the kernel layout, as the bench's steps do.  One JSON line per
measurement.

The estimate, written before the first run, from the code and the figures the repository already
holds (README: the four-product kernel computes every sum of 10k x 100k in 5.6-5.7 ms; king_abi.hip
use_full_counts: full form 8.8 ms against lean 7.0 ms there, i.e. the hom/hom pass -- 16 MFMAs per
k-step in front of the main loop's 64 -- adds a quarter):
    lean four-product time of the block = 5.65 ms x (pairs of the block / 5.0e7 pairs of 10k)
    + 25 % for the hom/hom pass
    + the epilogue: 64 out-of-line decisions per lane and tile, each three fp64 divides and their
      neighbours, ~300 instructions at ~8 cycles = ~2400 cycles, so ~150k cycles per wavefront and
      tile against 391 k-steps x 80 MFMAs x 32 cycles = 1.0 M cycles of k loop: + 15 %.
8192^2 / 2 = 3.36e7 pairs: 3.8 ms lean, 4.7 ms full, 5.4 ms with the epilogue; 16384^2 / 2 = 1.34e8
pairs: 15.2, 19.0, 21.8 ms.  Printed beside the result, right or wrong.

usage: python tools/pihat_time.py [OUT]
       (OUT is overwritten; default: nothing is written)
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import numpy as np
import torch

import cuking_amd
from cuking_amd.synth import cohort_to_device, plan_cohort

parser = argparse.ArgumentParser()
parser.add_argument("out", nargs="?", default=os.devnull)
args = parser.parse_args()
out = open(args.out, "w")

ESTIMATE_MS = {8192: dict(lean=3.8, full=4.7, pihat=5.4),
               16384: dict(lean=15.2, full=19.0, pihat=21.8)}


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
    return dict(median_ms=float(np.median(times)), min_ms=float(min(times)))


ctx = cuking_amd.KingContext(0)
SEED = 7
MAX_RESULTS = 1 << 20
for n, m, block, king_thr in ((10_000, 100_000, 8192, 0.05), (100_000, 100_000, 16384, 0.0884)):
    wps = cuking_amd.words_per_sample(m)
    kind, pa, pb = cohort_to_device(plan_cohort(n, SEED))
    bits = ctx.synth_bitset(SEED, kind, pa, pb, n - block, n, m)
    torch.cuda.synchronize()
    sm = cuking_amd.Submatrix(block)
    where = dict(cohort=f"{n} x {m}", block=block, pairs=sm.NumPairs(), variant=ctx.variant_name())
    est = ESTIMATE_MS[block]
    say(dict(op="clone", **where, **timed(lambda: bits.clone()),
             bitset_gb=block * wps * 8 / 1e9))
    kin = torch.empty((block, block), dtype=torch.float32, device="cuda:0")
    say(dict(op="kin_matrix", **where, **timed(lambda: ctx.kin_matrix(sm, wps, bits, out=kin)),
             estimate_ms=est["lean"]))
    del kin
    results = torch.zeros((MAX_RESULTS, 6), dtype=torch.int32, device="cuda:0")
    words = torch.zeros(2, dtype=torch.int32, device="cuda:0")

    def king(thr, cap):
        words.zero_()
        ctx.compute_king(sm, wps, bits, thr, cap, results, words[0:1], words[1:2])

    t = timed(lambda: king(king_thr, MAX_RESULTS))
    say(dict(op="compute_king", threshold=king_thr, **where, **t, records=int(words[0])))
    t = timed(lambda: king(0.0, 0))
    say(dict(op="compute_king, full form, counting", threshold=0.0, **where, **t,
             counted=int(words[0]) & 0xFFFFFFFF, estimate_ms=est["full"]))

    model = cuking_amd.pi_hat_model_host(ctx.site_counts(bits, wps).cpu().numpy().view(np.uint32), m)

    def pihat(thr, flags, cap):
        words.zero_()
        cuking_amd._lib.check(ctx.lib.cuking_compute_pihat(
            ctx.handle, C.byref(sm.c), wps, bits.data_ptr(), C.byref(model.c), thr, flags, cap,
            results.data_ptr() if cap else None, words[0:1].data_ptr(), words[1:2].data_ptr(),
            None))

    default = cuking_amd.pihat.DEFAULT_MIN_PI_HAT
    for what, thr, flags, cap in (("bounded", default, 0, MAX_RESULTS),
                                  ("unbounded", default, 1, MAX_RESULTS),
                                  ("every pair, counting", -1.0, 0, 0)):
        t = timed(lambda: pihat(thr, flags, cap))
        say(dict(op=f"compute_pihat, {what}", min_pi_hat=thr, **where, **t,
                 counted=int(words[0]) & 0xFFFFFFFF, overflow=int(words[1]),
                 estimate_ms=est["pihat"], median_over_estimate=t["median_ms"] / est["pihat"]))
    del bits, results, words
    torch.cuda.empty_cache()
out.close()
