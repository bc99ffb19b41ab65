"""Seeded random sweeps of the HIP path against the CPU oracle, inside the gate
(`pytest -m gpu`): the cases of tools/fuzz_gpu.py, tools/fuzz_split.py and
tools/stress_split.py (tests/fuzz_cases.py) with fixed seeds.  Round 2's two
silent-wrong-answer compiler incidents were both found by these generators and
by nothing in the deterministic suite.  A failure prints its reproducer (seed,
case index, parameters)."""
import os
import time

import pytest

import fuzz_cases

pytestmark = pytest.mark.gpu

# (seed, cases): about 30 s per general sweep and 10 s per split sweep on one MI355X
# box with 16 host threads (the CPU oracle is most of it)
GENERAL = [(101, 500), (102, 500), (103, 500)]
SPLIT = [(201, 100), (202, 100), (203, 100)]
# run_reducing (kin_matrix, kin_summary, relative_counts and the record call interleaved), in
# one session on one MI355X box in which the three general sweeps took 22, 30 and 23 s: the
# mixed sweeps 20 s (seed 301: one case of the class "giveup" among them), 13 s and 10 s, the
# sweep of launches of >= 64 tiles 13 s, the three cases with more tiles than CUs 10 s (the
# oracle and the numpy expectations are most of it: 21 million pairs per case of that class)
REDUCING = [(301, 120), (302, 120), (303, 120)]
REDUCING_TILES = [(311, 30)]
REDUCING_GIVEUP = [(321, 3)]
# (what tests/test_reducing_cases.py checks on the CPU: the share of pairs compared bit for bit)
REDUCING_SWEEPS = [(s, c, None) for s, c in REDUCING] + \
    [(s, c, "tiles") for s, c in REDUCING_TILES] + [(s, c, "giveup") for s, c in REDUCING_GIVEUP]
# run_pipeline (bed, site QC, LD and unrelated-set calls interleaved on a pool of 10 streams), in
# one session on one MI355X box in which the three mixed run_reducing sweeps took 20, 12 and
# 10 s: the three sweeps of the class "small" 2 s each, the one around the sample boundaries
# 1 s, the one around the site boundaries 3 s (numpy and the oracle are most of it)
PIPELINE = [(401, 200), (402, 200), (403, 200)]
PIPELINE_SAMPLES = [(411, 40)]
PIPELINE_SITES = [(421, 40)]
# (what tests/test_pipeline_cases.py holds to its conditions on the CPU)
PIPELINE_SWEEPS = [(s, c, "small") for s, c in PIPELINE] + \
    [(s, c, "samples") for s, c in PIPELINE_SAMPLES] + [(s, c, "sites") for s, c in PIPELINE_SITES]
# run_site_order (the filter path with "filter_site_order" on: record calls at two thresholds,
# tile ranges, relative_counts, kin_matrix and a staged pass interleaved), in
# one session on one MI355X box with 16 host threads: 7, 7 and 6 s (the oracle's all_pairs call
# and the numpy expectations are most of it), against the 22 to 30 s of a general sweep
SITE_ORDER = [(501, 100), (502, 100), (503, 100)]
# (what tests/test_site_order_cases.py holds to its conditions on the CPU)
# run_pcrelate (pcrelate_matrix, a sub-block, pcrelate_records at four thresholds and
# pcrelate_pairs twice, interleaved over one bitset and one model, the host twins on every case),
# in one session on one MI355X box in which the three run_site_order sweeps took 7, 7 and 6 s:
# the three sweeps of the class "small" 3, 2 and 2 s, the one on the tile and step edges 1 s,
# the exact one 1 s (the float64 references and the host twins are most of it)
PCRELATE = [(601, 60), (602, 60), (603, 60)]
PCRELATE_TILES = [(611, 40)]
PCRELATE_EXACT = [(621, 40)]
# (what tests/test_pcrelate_fuzz_cases.py holds to its conditions on the CPU)
PCRELATE_SWEEPS = [(s, c, "small") for s, c in PCRELATE] + \
    [(s, c, "tiles") for s, c in PCRELATE_TILES] + [(s, c, "exact") for s, c in PCRELATE_EXACT]
PCRELATE_TWIN_EVERY = 1
# run_pihat (the PI_HAT scan at two thresholds, over tile ranges, counting and into a short
# buffer, compute_counts, the KING records and kin_matrix or relative_counts, interleaved over
# one bitset), in one session on one MI355X box in which the three mixed run_reducing sweeps took
# 19, 11 and 9 s and the one of launches of >= 64 tiles 11 s: the three sweeps of the class
# "small" 5, 3 and 5 s, the one on the tile and step edges 2 s, the one of launches of >= 64
# tiles 14 s (17.8 million pairs; the oracle's all_pairs and the numpy references are most of it.
# Nine cases are the fewest that draw every model once; the host twin runs on every third of them
# and on every case of the other classes, and is not what dominates: 14 s with it on every case too)
PIHAT = [(701, 40), (702, 40), (704, 40)]
PIHAT_EDGES = [(711, 30)]
PIHAT_TILES = [(727, 9)]
# (what tests/test_pihat_fuzz_cases.py holds to its conditions on the CPU)
PIHAT_SWEEPS = [(s, c, "small") for s, c in PIHAT] + \
    [(s, c, "edges") for s, c in PIHAT_EDGES] + [(s, c, "tiles") for s, c in PIHAT_TILES]
PIHAT_TWIN_EVERY = {"small": 1, "edges": 1, "tiles": 3}
SCALE =float(os.environ.get("CUKING_FUZZ_SCALE", "1"))


def _log(msg):
    print(msg, flush=True)


@pytest.mark.parametrize("seed,cases", GENERAL)
def test_random_shapes_shards_variants_forms(ctx, seed, cases):
    t0 = time.time()
    ran = fuzz_cases.run_general(ctx, seed, max(1, int(cases * SCALE)), log=_log)
    print(f"run_general seed {seed}: {ran} cases OK in {time.time() - t0:.0f}s")
    assert ran == max(1, int(cases * SCALE))


@pytest.mark.parametrize("seed,cases", SPLIT)
def test_random_remainder_splits_ranges_and_staged_streams(ctx, seed, cases):
    t0 = time.time()
    ran = fuzz_cases.run_split(ctx, seed, max(1, int(cases * SCALE)), log=_log)
    print(f"run_split seed {seed}: {ran} cases OK in {time.time() - t0:.0f}s")
    assert ran == max(1, int(cases * SCALE))


def _reducing_sweep(ctx, seed, cases, size_class):
    """One run_reducing sweep: every case drawn was run, and at least 95 % of its pairs had a
    kinship that is not NaN (the only entries assert_same does not compare bit for bit)."""
    t0 = time.time()
    cases, stats = max(1, int(cases * SCALE)), {}
    ran = fuzz_cases.run_reducing(ctx, seed, cases, log=_log, size_class=size_class, stats=stats)
    print(f"run_reducing seed {seed} ({size_class}): {ran} cases OK in {time.time() - t0:.0f}s, "
          f"{stats['compared']} of {stats['pairs']} pairs compared bit for bit")
    assert ran == cases
    assert stats["pairs"] > 0 and stats["compared"] >= 0.95 * stats["pairs"], stats
    return stats


@pytest.mark.parametrize("seed,cases", REDUCING)
def test_random_reducing_calls_interleaved(ctx, seed, cases):
    _reducing_sweep(ctx, seed, cases, None)


@pytest.mark.parametrize("seed,cases", REDUCING_TILES)
def test_random_reducing_calls_launches_of_64_tiles(ctx, seed, cases):
    _reducing_sweep(ctx, seed, cases, "tiles")


@pytest.mark.parametrize("seed,cases", REDUCING_GIVEUP)
def test_random_reducing_calls_more_tiles_than_cus(ctx, seed, cases):
    """... and the filter variant's give-up path was really taken by a relative_counts call:
    later tiles handed their quadrants to the four-product kernel's counting form."""
    stats = _reducing_sweep(ctx, seed, cases, "giveup")
    assert stats["giveup_dense_quadrants"] > 0, stats


def _pipeline_sweep(ctx, seed, cases, size_class):
    """One run_pipeline sweep: every case drawn was run, every kind of call at least once, and
    a stream came back after the context had given its scratch entry to another."""
    import pipeline_cases
    t0 = time.time()
    cases, stats = max(1, int(cases * SCALE)), {}
    ran = fuzz_cases.run_pipeline(ctx, seed, cases, log=_log, size_class=size_class, stats=stats)
    print(f"run_pipeline seed {seed} ({size_class}): {ran} cases OK in {time.time() - t0:.0f}s, "
          f"{stats}")
    assert ran == cases
    assert all(stats[kind] > 0 for kind in pipeline_cases.KINDS), stats
    assert stats["evictions"] > 0, stats


@pytest.mark.parametrize("seed,cases", PIPELINE)
def test_random_pipeline_calls_interleaved(ctx, seed, cases):
    _pipeline_sweep(ctx, seed, cases, "small")


@pytest.mark.parametrize("seed,cases", PIPELINE_SAMPLES)
def test_random_pipeline_calls_sample_boundaries(ctx, seed, cases):
    _pipeline_sweep(ctx, seed, cases, "samples")


@pytest.mark.parametrize("seed,cases", PIPELINE_SITES)
def test_random_pipeline_calls_site_boundaries(ctx, seed, cases):
    _pipeline_sweep(ctx, seed, cases, "sites")


@pytest.mark.parametrize("seed,cases", SITE_ORDER)
def test_random_site_order_calls_interleaved(ctx, seed, cases):
    """One run_site_order sweep: every case drawn was run; every whole-block call the rule of
    prepare() expects an ordered layout behind left one (a mismatch raises at once: the sums
    say that there were such calls); tiles left at a check; every gather form ordered a
    layout."""
    import site_order_cases
    t0 = time.time()
    cases, stats = max(1, int(cases * SCALE)), {}
    ran = fuzz_cases.run_site_order(ctx, seed, cases, log=_log, stats=stats)
    print(f"run_site_order seed {seed}: {ran} cases OK in {time.time() - t0:.0f}s, {stats}")
    assert ran == cases
    assert stats["ordered"] == stats["expected_ordered"] > 0, stats
    assert stats["early_exits"] > 0, stats
    assert stats["gathers"] == sorted(site_order_cases.GATHERS), stats


def _pcrelate_sweep(ctx, seed, cases, size_class):
    """One run_pcrelate sweep: every case drawn was run; every D bucket of every kernel was
    launched; a launch cap really split calls."""
    import pcrelate_fuzz_cases as pf
    t0 = time.time()
    cases, stats = max(1, int(cases * SCALE)), {}
    ran = fuzz_cases.run_pcrelate(ctx, seed, cases, log=_log, size_class=size_class, stats=stats,
                                  twin_every=PCRELATE_TWIN_EVERY)
    print(f"run_pcrelate seed {seed} ({size_class}): {ran} cases OK in {time.time() - t0:.0f}s, "
          f"{stats}")
    assert ran == cases
    buckets = [4] if size_class == "exact" else [4, 8, 16, 32]
    assert all(stats["d_seen"][kind] == buckets for kind in pf.KINDS), stats
    assert stats["split_launches"] > 0, stats
    return stats


@pytest.mark.parametrize("seed,cases", PCRELATE)
def test_random_pcrelate_calls_interleaved(ctx, seed, cases):
    """... and at least 90 % of the matrix entries were not NaN: held to a tolerance."""
    stats = _pcrelate_sweep(ctx, seed, cases, "small")
    assert stats["entries"] > 0 and stats["compared"] >= 0.9 * stats["entries"], stats


@pytest.mark.parametrize("seed,cases", PCRELATE_TILES)
def test_random_pcrelate_calls_tile_and_step_edges(ctx, seed, cases):
    stats = _pcrelate_sweep(ctx, seed, cases, "tiles")
    assert stats["entries"] > 0 and stats["compared"] >= 0.9 * stats["entries"], stats


@pytest.mark.parametrize("seed,cases", PCRELATE_EXACT)
def test_random_pcrelate_calls_exact_on_bytes(ctx, seed, cases):
    _pcrelate_sweep(ctx, seed, cases, "exact")


def _pihat_sweep(ctx, seed, cases, size_class):
    """One run_pihat sweep: every case drawn was run; on what ran, pairs took every bounding step
    and the NaN exit, every model spec and every variant was drawn, and pairs sat exactly ON a
    threshold of 0.0, of 0.5 and of 1.0."""
    import pihat_cases
    import pihat_fuzz_cases as pf
    t0 = time.time()
    cases, stats = max(1, int(cases * SCALE)), {}
    ran = fuzz_cases.run_pihat(ctx, seed, cases, log=_log, size_class=size_class, stats=stats,
                               twin_every=PIHAT_TWIN_EVERY[size_class])
    print(f"run_pihat seed {seed} ({size_class}): {ran} cases OK in {time.time() - t0:.0f}s, "
          f"{stats}")
    assert ran == cases
    assert set(stats["branches"]) == set(pihat_cases.BRANCHES), stats
    assert set(stats["models"]) == set(pf.SPECS), stats
    assert set(stats["variants"]) == set(pf.VARIANTS), stats
    assert all(stats["ties"].get(t, 0) > 0 for t in pf.TIE_THRESHOLDS), stats
    assert 0 < stats["records"] < stats["pairs"], stats
    return stats


@pytest.mark.parametrize("seed,cases", PIHAT)
def test_random_pihat_among_the_pair_calls(ctx, seed, cases):
    """... and PI_HAT launches had remainder pieces: the SPLIT instantiations ran."""
    stats = _pihat_sweep(ctx, seed, cases, "small")
    assert stats["split_launches"] > 0, stats


@pytest.mark.parametrize("seed,cases", PIHAT_EDGES)
def test_random_pihat_tile_and_step_edges(ctx, seed, cases):
    _pihat_sweep(ctx, seed, cases, "edges")


@pytest.mark.parametrize("seed,cases", PIHAT_TILES)
def test_random_pihat_launches_of_64_tiles(ctx, seed, cases):
    _pihat_sweep(ctx, seed, cases, "tiles")


def test_one_staged_configuration_repeated(ctx):
    """100 repetitions of each (matrix-core variant, form, split, streams)
    combination: the intermittent failure of round 2 showed up a few times in
    hundreds of repetitions of exactly this configuration."""
    t0 = time.time()
    rows = fuzz_cases.run_stress(ctx, max(1, int(100 * SCALE)), log=_log)
    print(f"run_stress: {len(rows)} combinations in {time.time() - t0:.0f}s")
    assert rows and all(bad == 0 for _, bad, _, _ in rows), rows
