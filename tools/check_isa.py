#!/usr/bin/env python3
"""Lists the matrix-core kernels' LDS-DMA loops in the assembly the last library
build left in cuking_amd/build_tmp/ (or in the listing given: king_mfma-*.s or
king_filter-*.s) and what the compiler put into them: instruction counts, scratch
accesses, vector-memory waits (the same check every build runs: cuking_amd/build.py,
check_mfma_loops and check_filter_loop)."""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from cuking_amd.build import PKG, check_filter_loop, check_mfma_loops

paths = [Path(p) for p in sys.argv[1:]] or [
    PKG / "build_tmp" / f"king_{k}-hip-amdgcn-amd-amdhsa-gfx950.s" for k in ("mfma", "filter")]
problems = []
for path in paths:
    check = check_filter_loop if path.name.startswith("king_filter") else check_mfma_loops
    problems += check(path, verbose=True)
for p in problems:
    print("BAD:", p)
sys.exit(1 if problems else 0)
