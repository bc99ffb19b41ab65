"""bench.py as the driver starts it: a plain run times the headline alone (the side
measurements take --full), and --dump-outputs writes the records of the last timed
step, which must be the oracle's records of the same seeded cohort."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


def run_bench(*args, timeout=60):
    return subprocess.run([sys.executable, "bench.py", *map(str, args)], capture_output=True,
                          text=True, timeout=timeout, cwd=str(ROOT))


@pytest.mark.parametrize("args,message", [
    (["--steps", "0"], "--steps must be at least 1"),
    (["--warmup", "-1"], "--warmup at least 0"),
    (["--extra-configs", "c1"], "--extra-configs measures beside the headline: it needs --full"),
])
def test_bench_refuses_arguments_it_cannot_honour(args, message):
    p = run_bench(*args)
    assert p.returncode == 2 and message in p.stderr, p.stderr
    assert p.stdout.strip() == ""


@pytest.mark.gpu
def test_plain_bench_dumps_the_records_of_its_last_step(tmp_path, oracle):
    from cuking_amd.synth import plan_cohort
    n, m, thr, seed, steps = 2000, 20000, 0.05, 11, 3
    p = run_bench("--gpus", 1, "--steps", steps, "--warmup", 1, "--samples", n, "--sites", m,
                  "--kin-threshold", thr, "--seed", seed, "--dump-outputs", tmp_path / "out",
                  timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["steps"] == steps and out["ms_per_step"] > 0 and out["value"] > 0
    for key in ("metric", "unit", "higher_is_better", "dtype"):
        assert key in out
    # the side measurements are --full's
    for key in ("value_layout_reused", "value_including_h2d", "other_configs"):
        assert key not in out
    assert out["cpu_baseline"] is None and out["roofline"]["sustained_clock_mhz"] is None

    cohort = plan_cohort(n, seed)
    bits = oracle.synth_bitset(seed, cohort.kind, cohort.pa, cohort.pb, 0, n, m)
    exp, ovf, _ = oracle.compute(oracle.submatrix(n), bits, thr)
    assert not ovf and len(exp) == out["config"]["results_per_step"]
    d = tmp_path / "out"
    assert np.load(d / "num_results.npy").tolist() == [len(exp)]
    for name in exp.dtype.names:
        got = np.load(d / f"{name}.npy")
        assert got.dtype == (np.float32 if name == "kin" else np.float64)
        assert np.array_equal(got, exp[name].astype(got.dtype)), name
    assert np.load(d / "kin.npy").view(np.uint32).tolist() == exp["kin"].view(np.uint32).tolist()
