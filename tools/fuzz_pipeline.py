#!/usr/bin/env python3
"""Randomised sweep of the input pipeline in bulk: pack_bed, site_counts, sample_counts,
compact_sites, filter_sites, transpose_sites, ld_edges, ld_prune, unrelated_set, prune and a
pair-kernel call on the filtered bits, 4 to 10 of them interleaved over one cohort on a pool of
10 streams, every output compared exactly with numpy and with the host functions.  The cases
are tests/fuzz_cases.py run_pipeline (a fixed-seed sample of them runs in `pytest -m gpu`,
tests/test_gpu_fuzz.py); a failure prints its reproducer.
usage: fuzz_pipeline.py [seed] [cases] [--first-case K] [--size-class small|samples|sites]
       (--first-case: replay one failure; without --size-class: mostly small, some of each)"""
import argparse
import sys
import time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import cuking_amd
import fuzz_cases

ap = argparse.ArgumentParser()
ap.add_argument("seed", type=int, nargs="?", default=1)
ap.add_argument("cases", type=int, nargs="?", default=100)
ap.add_argument("--first-case", type=int, default=0)
ap.add_argument("--size-class", default=None)
args = ap.parse_args()
size_class = None if args.size_class in (None, "mixed") else args.size_class
t0, stats = time.time(), {}
try:
    ran = fuzz_cases.run_pipeline(cuking_amd.KingContext(0), args.seed, args.cases, args.first_case,
                                  log=lambda m: print(m, flush=True), size_class=size_class,
                                  stats=stats)
except fuzz_cases.FuzzMismatch as e:
    print(f"fuzz_pipeline seed {args.seed}: MISMATCH after {time.time() - t0:.0f}s\n{e}", flush=True)
    sys.exit(1)
print(f"fuzz_pipeline seed {args.seed}: {ran} cases OK in {time.time() - t0:.0f}s, {stats}",
      flush=True)
