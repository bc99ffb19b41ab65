"""Cohort models of the synthetic generator on the GPU: the device generator against the
numpy twin (tests/synth_models_twin.py) bit for bit, and the records of every kernel on the
new cohorts against oracle.pyoracle byte for byte.  No tolerance anywhere."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import cuking_amd
from cuking_amd import _lib
from cuking_amd import build as cbuild
from cuking_amd.synth import cohort_to_device, plan_cohort

import synth_models_twin as twin
from test_synth_models import NEW_MODELS, fixture_records, load_fixture

pytestmark = pytest.mark.gpu

ALL_MODELS = twin.MODELS
# (kernel, variant, filter_sort): the default kernel with the sorted layout on and off,
# the four-product kernel, a VALU shape and the stream kernel
KERNELS = [("tiled", 7, 1), ("tiled", 7, 0), ("tiled", 6, 1), ("tiled", 2, 1), ("stream", 0, 1)]


@pytest.fixture(scope="module")
def mctx():
    """A context of this module's own: the tests below change its kernel and options."""
    c = cuking_amd.KingContext(0)
    yield c
    c.close()


def select(ctx, kernel, variant, filter_sort=1):
    ctx.set_kernel(kernel)
    ctx.set_option("filter_sort", filter_sort)
    if kernel == "tiled":
        ctx.set_option("variant", variant)


def device_bits(ctx, model, seed, cohort, begin, end, num_sites):
    import torch
    kind, pa, pb = cohort_to_device(cohort, 0)
    dev = ctx.synth_bitset(seed, kind, pa, pb, begin, end, num_sites, model=model)
    torch.cuda.synchronize()
    return dev


def host(dev):
    return dev.cpu().numpy().view(np.uint64)


# ------------------------------------------------------- 6. device == twin ----
@pytest.mark.parametrize("model", ALL_MODELS)
def test_device_equals_twin(mctx, model):
    cohort = plan_cohort(400, 77)
    for m in (1, 63, 64, 1000, 2049):
        dev = device_bits(mctx, model, 77, cohort, 0, 400, m)
        assert dev.shape == (400, cuking_amd.words_per_sample(m))
        exp = twin.synth_bitset(model, 77, cohort.kind, cohort.pa, cohort.pb, 0, 400, m)
        assert np.array_equal(host(dev), exp), m
    # a row sub-range: what the shards of a split run generate
    dev = device_bits(mctx, model, 77, cohort, 380, 400, 500)
    exp = twin.synth_bitset(model, 77, cohort.kind, cohort.pa, cohort.pb, 380, 400, 500)
    assert np.array_equal(host(dev), exp)
    # ... and by number
    by_number = device_bits(mctx, twin.MODELS.index(model), 77, cohort, 380, 400, 500)
    assert np.array_equal(host(by_number), exp)


@pytest.mark.parametrize("model", ALL_MODELS)
def test_device_equals_twin_larger(mctx, model):
    n, m = 3000, 20000                      # (the twin takes ~3 s at this size)
    cohort = plan_cohort(n, 9)
    dev = device_bits(mctx, model, 9, cohort, 0, n, m)
    exp = twin.synth_bitset(model, 9, cohort.kind, cohort.pa, cohort.pb, 0, n, m)
    assert np.array_equal(host(dev), exp)


# ------------------------------------- 7. model 0 == the entry point of old ----
def test_baseline_model_is_cuking_synth_bitset(mctx, oracle):
    import torch
    n, m, seed = 2000, 10000, 4242
    cohort = plan_cohort(n, seed)
    kind, pa, pb = cohort_to_device(cohort, 0)
    wps = cuking_amd.words_per_sample(m)
    old = torch.zeros((n, wps), dtype=torch.int64, device="cuda:0")
    stream = int(torch.cuda.current_stream().cuda_stream)
    _lib.check(mctx.lib.cuking_synth_bitset(mctx.handle, seed, kind.data_ptr(), pa.data_ptr(),
                                            pb.data_ptr(), 0, n, m, wps, old.data_ptr(), stream))
    new = mctx.synth_bitset(seed, kind, pa, pb, 0, n, m, model="baseline")
    default = mctx.synth_bitset(seed, kind, pa, pb, 0, n, m)
    torch.cuda.synchronize()
    exp = oracle.synth_bitset(seed, cohort.kind, cohort.pa, cohort.pb, 0, n, m)
    assert host(old).tobytes() == host(new).tobytes() == host(default).tobytes() == exp.tobytes()


def test_device_entry_point_argument_checks(mctx):
    import torch
    cohort = plan_cohort(100, 1)
    kind, pa, pb = cohort_to_device(cohort, 0)
    wps = cuking_amd.words_per_sample(100)
    out = torch.zeros((100, wps), dtype=torch.int64, device="cuda:0")
    lib, h = mctx.lib, mctx.handle
    call = lambda model, b, e, w, dst: lib.cuking_synth_bitset_model(  # noqa: E731
        h, model, 1, kind.data_ptr(), pa.data_ptr(), pb.data_ptr(), b, e, 100, w, dst, None)
    assert call(3, 0, 100, wps, out.data_ptr()) == _lib.ERR_INVALID_ARGUMENT
    assert b"unknown synthetic cohort model" in lib.cuking_last_error()
    assert call(-1, 0, 100, wps, out.data_ptr()) == _lib.ERR_INVALID_ARGUMENT
    assert call(2, 5, 4, wps, out.data_ptr()) == _lib.ERR_INVALID_ARGUMENT      # reversed
    assert call(2, 0, 100, wps + 2, out.data_ptr()) == _lib.ERR_INVALID_ARGUMENT
    assert call(2, 0, 100, wps, None) == _lib.ERR_INVALID_ARGUMENT
    assert call(2, 7, 7, wps, None) == _lib.OK                                  # empty range
    with pytest.raises(ValueError):
        mctx.synth_bitset(1, kind, pa, pb, 0, 100, 100, model="nope")


# ------------------------------------------------------------ 8. fixtures ----
@pytest.mark.parametrize("kernel,variant", [("tiled", 7), ("tiled", 6), ("stream", 0)])
@pytest.mark.parametrize("model", NEW_MODELS)
def test_device_reproduces_the_fixture(mctx, model, kernel, variant):
    import torch
    select(mctx, kernel, variant)
    g, bits = load_fixture(model)
    n, m = g["num_samples"], g["num_sites"]
    as_t = lambda a: torch.tensor(a, dtype=torch.int32, device="cuda:0")  # noqa: E731
    dev = mctx.synth_bitset(g["seed"], as_t(g["kind"]), as_t(g["pa"]), as_t(g["pb"]), 0, n, m,
                            model=model)
    torch.cuda.synchronize()
    assert np.array_equal(host(dev), bits)
    got = mctx.run(cuking_amd.Submatrix(n), bits.shape[1], dev, g["kin_threshold"])
    assert got.tobytes() == fixture_records(g["records"]).tobytes()


# ------------------------------------- 9. records of every kernel == oracle ----
RECORDS_N, RECORDS_M, RECORDS_SEED = 1500, 20000, 31


@pytest.fixture(scope="module")
def record_cohorts(oracle):
    """Per new model: the cohort, the twin's bitset, and the oracle's records at both
    thresholds.  20,000 sites = 79 k-steps of 256: the filter's check points are active
    (filter_check_min_steps = 64)."""
    out = {}
    cohort = plan_cohort(RECORDS_N, RECORDS_SEED)
    for model in NEW_MODELS:
        bits = twin.synth_bitset(model, RECORDS_SEED, cohort.kind, cohort.pa, cohort.pb, 0,
                                 RECORDS_N, RECORDS_M)
        tail = twin.in_tail(model, RECORDS_SEED, np.arange(RECORDS_N))
        # so that "empty equals empty" cannot pass: every planted duplicate and
        # parent-child pair outside the admixed tail must be a record (the oracle meets
        # this on the twin's bitset: 108 / 110 records against a bar of 93 / 91)
        bar = sum(1 for i, j, rel in cohort.planted
                  if rel in ("dup", "po") and not tail[i] and not tail[j])
        exp = {}
        for thr in (0.05, 0.0884):
            res, ovf, _ = oracle.compute(oracle.submatrix(RECORDS_N), bits, thr, threads=8)
            assert ovf == 0 and len(res) >= bar > 80, (model, thr, len(res), bar)
            exp[thr] = res
        out[model] = (cohort, bits, tail, exp)
    return out


@pytest.mark.parametrize("kernel,variant,filter_sort", KERNELS)
@pytest.mark.parametrize("model", NEW_MODELS)
def test_records_equal_the_oracle(mctx, record_cohorts, model, kernel, variant, filter_sort):
    cohort, bits, tail, exp = record_cohorts[model]
    if model == "admixed":
        assert 5 <= tail.sum() <= 40        # low-call-rate samples for the sorted layout to move
    dev = device_bits(mctx, model, RECORDS_SEED, cohort, 0, RECORDS_N, RECORDS_M)
    assert np.array_equal(host(dev), bits)
    select(mctx, kernel, variant, filter_sort)
    try:
        for thr, want in exp.items():
            got = mctx.run(cuking_amd.Submatrix(RECORDS_N), bits.shape[1], dev, thr)
            assert got.tobytes() == want.tobytes(), (model, kernel, variant, filter_sort, thr)
    finally:
        select(mctx, "tiled", 7, 1)


# ------------------------------------------------------------ 10. both hosts ----
HOST_N, HOST_M, HOST_SEED, HOST_THR = 600, 3000, 5, 0.06


def expected_host_records(oracle, model, k, shard):
    cohort = plan_cohort(HOST_N, HOST_SEED)
    bits = twin.synth_bitset(model, HOST_SEED, cohort.kind, cohort.pa, cohort.pb, 0, HOST_N,
                             HOST_M)
    osm = oracle.submatrix(HOST_N, k, shard)
    idx = list(range(osm.i_begin, osm.i_end))
    if osm.i_begin != osm.j_begin:
        idx += list(range(osm.j_begin, osm.j_end))
    exp, ovf, _ = oracle.compute(osm, np.ascontiguousarray(bits[idx]), HOST_THR)
    assert ovf == 0 and len(exp) > 0
    return exp


def check_table(path, exp):
    import pyarrow.parquet as pq
    t = pq.read_table(path)
    assert t.num_rows == len(exp)
    assert t.column("i").to_pylist() == [f"S{x:07d}" for x in exp["sample_i"]]
    assert t.column("j").to_pylist() == [f"S{x:07d}" for x in exp["sample_j"]]
    assert np.array_equal(t.column("kin").to_numpy().view(np.uint32), exp["kin"].view(np.uint32))
    for name in ("ibs0", "ibs1", "ibs2"):
        assert np.array_equal(t.column(name).to_numpy().astype(np.uint32), exp[name])


@pytest.fixture(scope="module")
def cli():
    cbuild.build_library()
    cbuild.build_cli()

    def run(*args):
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")    # (as tests/test_multi_gpu.py)
        p = subprocess.run([str(cbuild.CLI_PATH), *map(str, args)], capture_output=True,
                           text=True, timeout=600, env=env)
        assert p.returncode == 0, f"cuking failed ({p.returncode}):\n{p.stdout}\n{p.stderr}"
        return p
    return run


@pytest.mark.parametrize("extra,k,shard", [([], 1, 0),
                                           (["--split_factor=2", "--shard_index=1"], 2, 1)])
def test_cli_synthetic_model(tmp_path, oracle, cli, extra, k, shard):
    out = tmp_path / "out"
    p = cli("--output_uri", out, f"--synthetic={HOST_N},{HOST_M},{HOST_SEED}",
            "--synthetic_model=admixed", f"--kin_threshold={HOST_THR}", *extra)
    exp = expected_host_records(oracle, "admixed", k, shard)
    check_table(out / f"part-{shard:05d}.snappy.parquet", exp)
    summary = json.loads(p.stdout.strip().splitlines()[-1])
    assert summary["pack"] == "synthetic" and summary["synthetic_model"] == "admixed"
    assert summary["results"] == len(exp)


def test_cli_summary_names_the_default_model(tmp_path, cli):
    p = cli("--output_uri", tmp_path / "out", "--synthetic=300,1000,5")
    assert json.loads(p.stdout.strip().splitlines()[-1])["synthetic_model"] == "baseline"


@pytest.mark.parametrize("k,shard", [(1, 0), (2, 1)])
def test_python_host_synthetic_model(tmp_path, oracle, k, shard):
    out = tmp_path / "out"
    p = subprocess.run([sys.executable, "-m", "cuking_amd.run", "--output-uri", str(out),
                        "--synthetic", f"{HOST_N},{HOST_M},{HOST_SEED}",
                        "--synthetic-model", "admixed", f"--kin-threshold={HOST_THR}",
                        f"--split-factor={k}", f"--shard-index={shard}"],
                       capture_output=True, text=True, timeout=600, cwd=str(ROOT))
    assert p.returncode == 0, p.stderr
    check_table(out / f"part-{shard:05d}.snappy.parquet",
                expected_host_records(oracle, "admixed", k, shard))


@pytest.mark.skipif(cuking_amd.device_count() < 2, reason="needs at least two GPUs")
def test_cli_synthetic_model_two_gpus(tmp_path, oracle, cli):
    import pyarrow.parquet as pq
    args = [f"--synthetic={HOST_N},{HOST_M},{HOST_SEED}", "--synthetic_model=admixed",
            f"--kin_threshold={HOST_THR}"]
    cli("--output_uri", tmp_path / "one", *args)
    cli("--output_uri", tmp_path / "two", "--num_gpus=2", *args)
    one = pq.read_table(tmp_path / "one" / "part-00000.snappy.parquet")
    two = pq.read_table(tmp_path / "two" / "part-00000.snappy.parquet")
    assert one.equals(two) and one.num_rows > 0
    check_table(tmp_path / "two" / "part-00000.snappy.parquet",
                expected_host_records(oracle, "admixed", 1, 0))
