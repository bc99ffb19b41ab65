#!/usr/bin/env python3
"""Randomised GPU-vs-oracle sweep of the filter path with the site order on, in bulk: record
calls at two thresholds, tile ranges, relative_counts, kin_matrix and a staged pass interleaved
over one bitset -- every block of a split, lengths from one site to 94 k-steps, forms, gather
forms, filter options, reuse, side streams.  The cases are tests/site_order_cases.py, the runner
tests/fuzz_cases.py run_site_order (a fixed-seed sample of them runs in `pytest -m gpu`,
tests/test_gpu_fuzz.py).
usage: fuzz_site_order.py [seed] [cases] [first_case]   (first_case: replay one failure)"""
import sys
import time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import cuking_amd
import fuzz_cases

seed = int(sys.argv[1]) if len(sys.argv) > 1 else 1
cases = int(sys.argv[2]) if len(sys.argv) > 2 else 100
first = int(sys.argv[3]) if len(sys.argv) > 3 else 0
t0, stats = time.time(), {}
ran = fuzz_cases.run_site_order(cuking_amd.KingContext(0), seed, cases, first,
                                log=lambda m: print(m, flush=True), stats=stats)
print(f"fuzz_site_order seed {seed}: {ran} cases OK in {time.time() - t0:.0f}s, {stats}",
      flush=True)
