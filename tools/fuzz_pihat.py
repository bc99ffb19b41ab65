#!/usr/bin/env python3
"""Randomised sweep of the PI_HAT scan among the other pair calls in bulk: pi_hat_records at two
thresholds and both settings of `bounded`, the tile-range entry point, counting, a short buffer,
compute_counts, the KING records and kin_matrix or relative_counts interleaved over one bitset --
shapes, blocks, models (of the block, the cohort, founders, made by hand), variants and launch
shapes drawn -- against the CPU oracle and the numpy restatement of the pair math, on bytes, and
the host twin.  The cases are tests/pihat_fuzz_cases.py, the runner tests/fuzz_cases.py run_pihat
(a fixed-seed sample of them runs in `pytest -m gpu`, tests/test_gpu_fuzz.py).
usage: fuzz_pihat.py [seed] [cases] [first_case] [size_class]
       (first_case: replay one failure; size_class: small (default), edges or tiles)"""
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
size_class = sys.argv[4] if len(sys.argv) > 4 else "small"
t0, stats = time.time(), {}
ran = fuzz_cases.run_pihat(cuking_amd.KingContext(0), seed, cases, first,
                           log=lambda m: print(m, flush=True), size_class=size_class,
                           stats=stats)
print(f"fuzz_pihat seed {seed} ({size_class}): {ran} cases OK in {time.time() - t0:.0f}s, "
      f"{stats}", flush=True)
