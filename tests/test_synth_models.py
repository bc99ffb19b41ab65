"""Cohort models of the synthetic generator (csrc/synth.hip), CPU side: the numpy twin
(tests/synth_models_twin.py) against the older C twin and the committed fixtures, the
properties the specification promises, the ABI and the flags of both hosts.

The fixtures tests/golden/synth_<model>_96x700.json were written by `regenerate_fixtures()`
below (python tests/test_synth_models.py): the plan of tests/golden/make_golden.py (96
samples, a few relatives planted by hand), the bitset of the numpy twin, the records of
oracle.pyoracle on it."""
import json
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT     # (puts the repository root on sys.path)

import cuking_amd
from cuking_amd import _lib
from cuking_amd import build as cbuild
from cuking_amd.synth import plan_cohort

import synth_models_twin as twin

NEW_MODELS = ("exome", "admixed")
SEEDS = (20240229, 7, 12345)
U32 = float(1 << 32)

FIXTURE_N, FIXTURE_M, FIXTURE_SEED, FIXTURE_THR = 96, 700, 424242, 0.1


# ------------------------------------------------------------------ fixtures ----
def fixture_path(model):
    return GOLDEN / f"synth_{model}_{FIXTURE_N}x{FIXTURE_M}.json"


def fixture_plan():
    """The plan of tests/golden/make_golden.py: 96 samples are too few for plan_cohort to
    plant relatives, so a few are planted by hand."""
    cohort = plan_cohort(FIXTURE_N, FIXTURE_SEED)
    kind, pa, pb = cohort.kind.copy(), cohort.pa.copy(), cohort.pb.copy()
    kind[90], pa[90], pb[90] = 1, 3, 3          # duplicate of 3
    kind[91], pa[91], pb[91] = 2, 10, 11        # child of 10 x 11
    kind[92], pa[92], pb[92] = 2, 10, 11        # full sibling
    kind[93], pa[93], pb[93] = 2, 10, 12        # half sibling
    return kind, pa, pb


def record_rows(res):
    return [[int(r["sample_i"]), int(r["sample_j"]), int(r["kin"].view(np.uint32)),
             int(r["ibs0"]), int(r["ibs1"]), int(r["ibs2"])] for r in res]


def regenerate_fixtures():
    from oracle import pyoracle
    kind, pa, pb = fixture_plan()
    for model in NEW_MODELS:
        bits = twin.synth_bitset(model, FIXTURE_SEED, kind, pa, pb, 0, FIXTURE_N, FIXTURE_M)
        res, ovf, _ = pyoracle.compute(pyoracle.submatrix(FIXTURE_N), bits, FIXTURE_THR)
        assert ovf == 0
        out = {"comment": f"cohort model '{model}': plan of make_golden.py, bitset of "
                          "tests/synth_models_twin.py, records of oracle.pyoracle",
               "model": model, "num_samples": FIXTURE_N, "num_sites": FIXTURE_M,
               "seed": FIXTURE_SEED, "kin_threshold": FIXTURE_THR,
               "kind": kind.tolist(), "pa": pa.tolist(), "pb": pb.tolist(),
               "bitset_words_per_sample": int(bits.shape[1]),
               "bitset_hex": [row.tobytes().hex() for row in bits],
               "record_fields": ["sample_i", "sample_j", "kin_bits", "ibs0", "ibs1", "ibs2"],
               "records": record_rows(res)}
        path = fixture_path(model)
        path.write_text(json.dumps(out, indent=None, separators=(",", ":")))
        print(path, len(out["records"]), "records", path.stat().st_size, "bytes")


def load_fixture(model):
    g = json.loads(fixture_path(model).read_text())
    bits = np.frombuffer(bytes.fromhex("".join(g["bitset_hex"])), dtype=np.uint64).reshape(
        g["num_samples"], g["bitset_words_per_sample"]).copy()
    return g, bits


def fixture_records(rows):
    from oracle.pyoracle import RESULT_DTYPE
    out = np.zeros(len(rows), dtype=RESULT_DTYPE)
    for k, (i, j, kin_bits, a, b, c) in enumerate(rows):
        out[k] = (i, j, np.uint32(kin_bits).view(np.float32), a, b, c)
    return out


# --------------------------------------------------------- 1. twin == C twin ----
@pytest.mark.parametrize("num_sites", [1, 63, 64, 1000, 2049])
def test_twin_baseline_equals_the_c_twin(oracle, num_sites):
    cohort = plan_cohort(400, 77)
    got = twin.synth_bitset("baseline", 77, cohort.kind, cohort.pa, cohort.pb, 0, 400, num_sites)
    exp = oracle.synth_bitset(77, cohort.kind, cohort.pa, cohort.pb, 0, 400, num_sites)
    assert got.dtype == exp.dtype and got.shape == exp.shape
    assert np.array_equal(got, exp)


def test_twin_baseline_equals_the_c_twin_on_a_row_range_and_a_tiny_cohort(oracle):
    cohort = plan_cohort(400, 77)
    assert (cohort.kind[380:400] != 0).any()       # the range holds planted relatives
    got = twin.synth_bitset(0, 77, cohort.kind, cohort.pa, cohort.pb, 380, 400, 500)
    assert np.array_equal(got, oracle.synth_bitset(77, cohort.kind, cohort.pa, cohort.pb,
                                                   380, 400, 500))
    tiny = plan_cohort(50, 3)                      # too small for planted relatives
    assert not tiny.planted and not tiny.kind.any()
    got = twin.synth_bitset(0, 3, tiny.kind, tiny.pa, tiny.pb, 0, 50, 333)
    assert np.array_equal(got, oracle.synth_bitset(3, tiny.kind, tiny.pa, tiny.pb, 0, 50, 333))


def test_twin_rows_can_be_generated_separately():
    cohort = plan_cohort(400, 5)
    for model in NEW_MODELS:
        whole = twin.synth_bitset(model, 5, cohort.kind, cohort.pa, cohort.pb, 0, 400, 300)
        part = twin.synth_bitset(model, 5, cohort.kind, cohort.pa, cohort.pb, 370, 400, 300)
        assert np.array_equal(whole[370:], part)


# --------------------------------------------------------------- 2. fixtures ----
@pytest.mark.parametrize("model", NEW_MODELS)
def test_twin_reproduces_the_fixture(oracle, model):
    g, bits = load_fixture(model)
    assert g["model"] == model
    kind, pa, pb = fixture_plan()
    assert g["kind"] == kind.tolist() and g["pa"] == pa.tolist() and g["pb"] == pb.tolist()
    again = twin.synth_bitset(model, g["seed"], g["kind"], g["pa"], g["pb"], 0,
                              g["num_samples"], g["num_sites"])
    assert np.array_equal(again, bits)
    res, ovf, _ = oracle.compute(oracle.submatrix(g["num_samples"]), bits, g["kin_threshold"])
    assert ovf == 0 and res.tobytes() == fixture_records(g["records"]).tobytes()
    pairs = {(r[0], r[1]) for r in g["records"]}
    assert {(3, 90), (10, 91), (11, 91), (91, 92)} <= pairs   # duplicate, parents, full sibs


# ------------------------------------------------------------- 3. properties ----
@pytest.mark.parametrize("seed", SEEDS)
def test_exome_spectrum(seed):
    """log-uniform AF on [2^-13, 1/2): octave k = 1..12 uniform, AF = (1 + u) * 2^-(k+1)."""
    a, b = twin.site_thresholds("exome", seed, 100000)
    assert np.array_equal(a, b)                      # one ancestry
    p = a / U32
    # the construction: the smallest value is 2^31 >> 12 = 2^19, the largest below 2^31
    assert a.min() >= 1 << 19 and a.max() < 1 << 31
    # P(AF >= 0.05) for an exact log-uniform law on 12 octaves below 1/2 is
    # log2(0.5 / 0.05) / 12 = log2(10) / 12 = 27.7 %; octave-uniform + linear inside differs
    # only inside the octave [1/32, 1/16) that 0.05 cuts: 3 octaves + (1/16 - 0.05) / (1/32)
    # = 3.4 octaves of 12 = 28.3 %.  Binomial sd at 100,000 sites: 0.14 points; the bound
    # is +-2 points around log2(10)/12.
    common = p >= 0.05
    share = common.mean()
    print(f"seed {seed}: sites with AF >= 0.05: {share:.4f}")
    assert abs(share - np.log2(10) / 12) < 0.02
    # Their share of sum 2p(1-p): for density 1/p on [a, 1/2] the integral of 2p(1-p)/p is
    # 2p - p^2, so (0.75 - (0.1 - 0.0025)) / (0.75 - ~0) = 0.87; asserted >= 0.8.
    het = 2 * p * (1 - p)
    het_share = het[common].sum() / het.sum()
    print(f"seed {seed}: their share of the heterozygosity: {het_share:.4f}, mean het {het.mean():.4f}")
    assert het_share >= 0.8


@pytest.mark.parametrize("seed", SEEDS)
def test_admixed_tables(seed):
    n, m = 10000, 100000
    cohort = plan_cohort(n, seed)
    founders = np.arange(cohort.num_founders)
    # ancestry: a fair coin per founder; sd of the share over ~9,650 founders is 0.5 points,
    # the bound (45 % .. 55 %) is ten of them
    share_b = twin.ancestry("admixed", seed, founders).mean()
    print(f"seed {seed}: founders in ancestry B: {share_b:.4f}")
    assert 0.45 < share_b < 0.55
    # thresholds differ where the site diverged (P = 1/4) and the two independent draws
    # differ (all but ~never): 25 % of 100,000 sites, sd 0.14 points; bound 23 % .. 27 %
    a, b = twin.site_thresholds("admixed", seed, m)
    assert np.array_equal(a, twin.site_thresholds("exome", seed, m)[0])
    differ = (a != b).mean()
    print(f"seed {seed}: sites whose thresholds differ between A and B: {differ:.4f}")
    assert 0.23 < differ < 0.27
    assert b.min() >= 1 << 19 and b.max() < 1 << 31
    # call rates: outside the tail uniform on [0.5 %, 3.5 %): mean 2 %, sd of the mean over
    # ~9,900 samples 0.0087 points; bound +-0.1 point
    samples = np.arange(n)
    thr = twin.missing_thresholds("admixed", seed, samples) / U32
    tail = twin.in_tail("admixed", seed, samples)
    body_mean = thr[~tail].mean()
    print(f"seed {seed}: mean missing threshold outside the tail {body_mean:.5f}, "
          f"tail {tail.mean():.4f} of the samples, {thr[tail].min():.4f} .. {thr[tail].max():.4f}")
    assert abs(body_mean - 0.02) < 0.001
    assert thr[~tail].min() >= 0.005 - 1e-9 and thr[~tail].max() < 0.035
    # the tail: 1 % of 10,000 samples, sd 0.1 point; bound 0.5 % .. 1.5 %
    assert 0.005 < tail.mean() < 0.015
    assert thr[tail].min() >= 0.10 - 1e-9 and thr[tail].max() <= 0.30
    # the other models: one ancestry, 1 % for everybody
    for model in ("baseline", "exome"):
        assert not twin.ancestry(model, seed, samples).any()
        assert (twin.missing_thresholds(model, seed, samples) == (1 << 32) // 100).all()


def kinship_matrix(g):
    """float64 KING-robust kinship of every pair (the formula of cuking.cu:289-294, as in
    conftest.kin_exact_two_roundings, without the float32 roundings); g uint8, 3 = missing."""
    het = (g == 1).astype(np.float64)
    hom0 = (g == 0).astype(np.float64)
    hom2 = (g == 2).astype(np.float64)
    defined = (g != 3).astype(np.float64)
    both_het = het @ het.T
    opposing = hom0 @ hom2.T + hom2 @ hom0.T
    het_i = het @ defined.T           # het sites of i among the sites j is defined at
    het_j = het_i.T
    num = 2 * both_het - 4 * opposing - het_i - het_j
    den = 4 * np.minimum(het_i, het_j)
    return 0.5 + num / den


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("model", NEW_MODELS)
def test_genotype_matrix_properties(model, seed):
    """600 founders x 20,000 sites: measured missing shares, and in `admixed` the
    separation of cross-ancestry pairs."""
    n, m = 600, 20000
    zeros = np.zeros(n, dtype=np.uint32)
    g = twin.genotypes(model, seed, zeros, zeros, zeros, 0, n, m)
    # a sample's missing calls are m Bernoulli draws at its threshold
    p = twin.missing_thresholds(model, seed, np.arange(n)) / U32
    z = np.abs((g == 3).mean(axis=1) - p) / np.sqrt(p * (1 - p) / m)
    print(f"{model} seed {seed}: largest deviation of a sample's missing share: "
          f"{z.max():.2f} standard errors")
    assert z.max() < 5
    anc = twin.ancestry(model, seed, np.arange(n))
    if model != "admixed":
        assert not anc.any()
        return
    kin = kinship_matrix(g)
    i, j = np.triu_indices(n, 1)
    same = anc[i] == anc[j]
    k_same, k_cross = kin[i, j][same], kin[i, j][~same]
    gap = (k_same.mean() - k_cross.mean()) / k_same.std()
    print(f"admixed seed {seed}: mean kinship same-ancestry {k_same.mean():.4f} "
          f"(sd {k_same.std():.4f}), cross-ancestry {k_cross.mean():.4f}: gap {gap:.1f} sd")
    assert k_cross.mean() < k_same.mean() - 3 * k_same.std()


# --------------------------------------------------------------------- 4. ABI ----
def test_abi_model_table():
    lib = _lib.load()
    for name in ("cuking_synth_bitset_model", "cuking_synth_num_models", "cuking_synth_model_name"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.cuking_synth_num_models() == 3
    names = [lib.cuking_synth_model_name(k).decode() for k in range(3)]
    assert names == ["baseline", "exome", "admixed"] == list(twin.MODELS)
    assert lib.cuking_synth_model_name(-1) == b"" and lib.cuking_synth_model_name(3) == b""
    assert cuking_amd.synth_models() == names
    for k, name in enumerate(names):
        assert cuking_amd.synth_model_number(name) == cuking_amd.synth_model_number(k) == k
    for bad in ("nope", "Exome", 3, -1):
        with pytest.raises(ValueError):
            cuking_amd.synth_model_number(bad)
    assert lib.cuking_abi_version() == 2


def test_abi_unknown_model_and_no_cpu_fallback():
    lib = _lib.load()
    words = cuking_amd.words_per_sample(100)
    for bad in (3, -1, 1 << 20):
        st = lib.cuking_synth_bitset_model(None, bad, 1, None, None, None, 0, 4, 100, words,
                                           None, None)
        assert st == _lib.ERR_INVALID_ARGUMENT
        assert b"unknown synthetic cohort model" in lib.cuking_last_error()
    # a known model still needs a context, and a context needs a gfx950 device: nothing
    # is computed on the CPU
    st = lib.cuking_synth_bitset_model(None, 2, 1, None, None, None, 0, 4, 100, words, None, None)
    assert st == _lib.ERR_INVALID_ARGUMENT and b"null context" in lib.cuking_last_error()
    if cuking_amd.device_count() == 0:
        with pytest.raises(cuking_amd.CukingError) as e:
            cuking_amd.KingContext(0).synth_bitset(1, None, None, None, 0, 4, 100, model="exome")
        assert e.value.status == _lib.ERR_DEVICE


# ------------------------------------------------------------------- 5. flags ----
@pytest.fixture(scope="module")
def cli():
    cbuild.build_library()
    cbuild.build_cli()
    assert cbuild.CLI_PATH.exists()

    def run(*args):
        return subprocess.run([str(cbuild.CLI_PATH), *map(str, args)], capture_output=True,
                              text=True, timeout=600)
    return run


def run_python_host(*args):
    return subprocess.run([sys.executable, "-m", "cuking_amd.run", *map(str, args)],
                          capture_output=True, text=True, timeout=300, cwd=str(ROOT))


def test_cli_model_flag_errors(cli, tmp_path):
    for spelling in ("--synthetic_model", "--synthetic-model"):
        p = cli("--synthetic=10,20", "--output_uri", tmp_path, f"{spelling}=nope")
        assert p.returncode == 1, p.stderr
        assert "Illegal value 'nope' specified for flag 'synthetic_model'" in p.stderr
        p = cli("--input_uri", tmp_path, "--output_uri", tmp_path, f"{spelling}=exome")
        assert p.returncode == 1
        assert "Error: INVALID_ARGUMENT: --synthetic_model needs --synthetic" in p.stderr
    p = cli("--synthetic=10,20", "--output_uri", tmp_path, "--synthetic_model")
    assert p.returncode == 1 and "Missing value for --synthetic_model" in p.stderr
    # a known name passes the flags: the schedule printer stops before any GPU work
    for spelling in ("--synthetic_model=admixed", "--synthetic-model=exome"):
        p = cli("--synthetic=1000,200", "--output_uri", tmp_path, spelling, "--num_gpus=2",
                "--print_schedule")
        assert p.returncode == 0, p.stderr
    p = cli("--help")
    assert p.returncode == 0 and "--synthetic_model=NAME" in p.stdout
    for name in twin.MODELS:
        assert name in p.stdout


def test_python_host_model_flag_errors(tmp_path):
    for spelling in ("--synthetic-model", "--synthetic_model"):
        p = run_python_host("--synthetic", "10,20", "--output-uri", tmp_path, spelling, "nope")
        assert p.returncode == 1, p.stderr
        assert ("Error: INVALID_ARGUMENT: Illegal value 'nope' specified for flag "
                "'synthetic_model'") in p.stderr
        p = run_python_host("--input-uri", tmp_path, "--output-uri", tmp_path, spelling, "exome")
        assert p.returncode == 1
        assert "Error: INVALID_ARGUMENT: --synthetic_model needs --synthetic" in p.stderr
    p = run_python_host("--help")
    assert p.returncode == 0 and "--synthetic-model" in p.stdout
    for name in twin.MODELS:
        assert name in p.stdout


if __name__ == "__main__":
    regenerate_fixtures()
