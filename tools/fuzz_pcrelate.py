#!/usr/bin/env python3
"""Randomised sweep of the three PC-Relate calls in bulk: pcrelate_matrix, a sub-block of it,
pcrelate_records and pcrelate_pairs interleaved over one bitset and one model -- every d, blocks
off the tile edges, pitches, bounds, launch caps, side streams, pair lists -- against the float64
references, each other's bytes and the host twins.  The cases are tests/pcrelate_fuzz_cases.py,
the runner tests/fuzz_cases.py run_pcrelate (a fixed-seed sample of them runs in `pytest -m gpu`,
tests/test_gpu_fuzz.py).
usage: fuzz_pcrelate.py [seed] [cases] [first_case] [size_class]
       (first_case: replay one failure; size_class: small (default), tiles or exact)"""
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
ran = fuzz_cases.run_pcrelate(cuking_amd.KingContext(0), seed, cases, first,
                              log=lambda m: print(m, flush=True), size_class=size_class,
                              stats=stats)
print(f"fuzz_pcrelate seed {seed} ({size_class}): {ran} cases OK in {time.time() - t0:.0f}s, "
      f"{stats}", flush=True)
