#!/usr/bin/env python3
"""Randomised GPU-vs-oracle sweep of the reducing calls in bulk: kin_matrix, kin_summary,
relative_counts and the record call interleaved over one bitset -- shapes up to launches of
>= 64 tiles and more tiles than CUs, blocks of a split, launch and filter options, bins,
thresholds, tile ranges, strided outputs, side streams.  The cases are tests/fuzz_cases.py
run_reducing (a fixed-seed sample of them runs in `pytest -m gpu`, tests/test_gpu_fuzz.py).
usage: fuzz_reducing.py [seed] [cases] [first_case] [size_class]
       (first_case: replay one failure; size_class: small | tiles | giveup, default mixed)"""
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
size_class = sys.argv[4] if len(sys.argv) > 4 and sys.argv[4] != "mixed" else None
t0, stats = time.time(), {}
ran = fuzz_cases.run_reducing(cuking_amd.KingContext(0), seed, cases, first,
                              log=lambda m: print(m, flush=True), size_class=size_class,
                              stats=stats)
print(f"fuzz_reducing seed {seed}: {ran} cases OK in {time.time() - t0:.0f}s, "
      f"{stats['compared']} of {stats['pairs']} pairs compared bit for bit, "
      f"give-up dense quadrants {stats['giveup_dense_quadrants']}", flush=True)
