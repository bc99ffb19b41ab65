"""The input pipeline's fuzzer judged on the CPU (tests/pipeline_cases.py): ld_edges_fast by
the Python double loop of ld_cases.py and by the library's host function, the bed decode and the
other expectations by their `*_host` twins, the generator's determinism, and that the sweeps
tests/test_gpu_fuzz.py commits are not vacuous."""
import numpy as np
import pytest

import cuking_amd
from cuking_amd import api
from ld_cases import ld_edges_numpy, same_records
from site_qc_cases import pack

import pipeline_cases as pc


def ld_draws(seed, cases, size_class, want, fits=lambda n, m: True):
    """(geno, call, expectation) of the first `want` ld_edges / ld_prune draws."""
    out = []
    for tag, geno in pc.pipeline_cases(seed, cases, 0, size_class):
        if not fits(*geno.shape):
            continue
        for call, e in zip(tag["calls"], pc.expect_calls(tag, geno)):
            if call["kind"] in ("ld_edges", "ld_prune"):
                out.append((geno, call, e))
        if len(out) >= want:
            break
    return out


def test_ld_edges_fast_is_the_double_loop():
    """Byte for byte on generated draws of n <= 70, m <= 200, among them groups, window 2, a
    window beyond m, r^2 0 and r^2 1 -- and on each of those by hand."""
    draws = ld_draws(900, 400, "small", 30, lambda n, m: n <= 70 and m <= 200)
    assert len(draws) >= 30
    seen = set()
    for geno, call, e in draws:
        group = pc.group_of(call["group"], geno.shape[1])
        assert same_records(e["edges"], ld_edges_numpy(geno, call["window"], call["r2"], group))
        seen |= {("group", group is not None), ("w2", call["window"] == 2),
                 ("wide", call["window"] > geno.shape[1]), ("r0", call["r2"] == 0.0),
                 ("r1", call["r2"] == 1.0), ("edges", len(e["edges"]) > 0)}
    assert {(k, True) for k in ("group", "w2", "wide", "r0", "r1", "edges")} <= seen, seen
    geno = pc._cohort(np.random.default_rng(3), 37, 150)[1]
    group = pc.group_of([40, 64, 100], 150)
    for window, r2, g in ((2, 0.2, None), (155, 0.0, group), (7, 1.0, None), (66, 0.001, group)):
        fast = pc.ld_edges_fast(geno, window, r2, g)
        assert same_records(fast, ld_edges_numpy(geno, window, r2, g)), (window, r2)
        assert (r2 == 1.0) == (len(fast) == 0)


@pytest.mark.parametrize("size_class", ("samples", "sites"))
def test_ld_edges_fast_is_the_host_function(size_class):
    draws = ld_draws(901, 60, size_class, 15)
    assert len(draws) >= 15
    for geno, call, e in draws:
        n, m = geno.shape
        site_bits = pc.site_bits_numpy(geno)
        want, count = cuking_amd.ld_edges_host(site_bits, m, n, call["window"], call["r2"],
                                               group=e["group"])
        assert count == len(e["edges"]) and same_records(e["edges"], want), (n, m, call)


def check_against_host(tag, geno):
    """Every expectation of a case that has a `*_host` twin equals it; returns the kinds seen."""
    n, m = geno.shape
    bits = pack(geno)
    wps = bits.shape[1]
    seen = set()
    for call, e in zip(tag["calls"], pc.expect_calls(tag, geno)):
        kind = call["kind"]
        seen.add(kind)
        if kind == "pack_bed":
            sm = cuking_amd.Submatrix(n, call["split"], call["shard"])
            got = np.full((sm.NumSamples(), wps), np.uint64(0xA5A5A5A5A5A5A5A5), dtype=np.uint64)
            for begin, end in e["chunks"]:
                cuking_amd.pack_bed_host(sm, got, e["rows"][begin:end], e["rows"].shape[1], begin,
                                         end, m)
            assert np.array_equal(got, e["bits"]), call
        elif kind == "compact_sites":
            want, _, kept = cuking_amd.compact_sites_host(bits, wps, cuking_amd.site_mask_words(
                e["keep"]), m)
            assert kept == e["keep"].sum() and np.array_equal(want, e["bits"]), call
        elif kind == "filter_sites":
            words, kept = cuking_amd.site_mask_host(
                pc.site_counts_numpy(geno, wps // 2), m, call["min_call_rate"], call["min_maf"],
                call["min_mac"], e["also"])
            assert np.array_equal(cuking_amd.site_mask_bool(words, m), e["keep"]), call
            assert e["fails"] == (kept == 0)
        elif kind == "transpose_sites":
            assert np.array_equal(cuking_amd.transpose_sites_host(bits, wps, m), e["site_bits"])
        elif kind == "ld_prune":
            assert np.array_equal(api.ld_priority_host(pc.site_counts_numpy(geno, wps // 2), m)
                                  .view(np.uint32), pc.priority_numpy(geno).view(np.uint32))
            keep, _ = api.unrelated_set_host(e["edges"], m, priority=e["used"], families=False)
            assert np.array_equal(keep == 1, e["keep"]), call
        elif kind in ("unrelated_set", "prune"):
            keep, family = api.unrelated_set_host(e["records"], e["count"], e["thr"],
                                                  priority=e["priority"])
            assert np.array_equal(keep, e["keep"]) and np.array_equal(family, e["family"]), call
    return seen


@pytest.mark.parametrize("size_class,cases", (("small", 40), ("samples", 6), ("sites", 6)))
def test_expectations_equal_their_host_twins(oracle, size_class, cases):
    seen = set()
    for tag, geno in pc.pipeline_cases(902, cases, 0, size_class):
        seen |= check_against_host(tag, geno)
    assert {"pack_bed", "compact_sites", "filter_sites", "transpose_sites", "ld_prune",
            "unrelated_set"} <= seen


def test_bed_decode_is_the_table():
    rows = np.array([[0b11100100, 0b01]], dtype=np.uint8)        # codes 0, 1, 2, 3, 1
    assert pc.bed_decode(rows, 5).T.tolist() == [[2, -1, 1, 0, -1]]
    geno = pc._cohort(np.random.default_rng(5), 13, 40)[1]
    assert np.array_equal(pc.bed_decode(cuking_amd.plink.encode_rows(geno), 13), geno)
    call = dict(seed=7, source="encode")
    rows = pc.bed_rows_of(call, geno)
    assert (rows[:, -1] >> 2).any() and np.array_equal(pc.bed_decode(rows, 13), geno)


def test_generator_is_deterministic():
    tags = pc.pipeline_tags(77, 12)
    assert [t["case"] for t in tags] == list(range(12))
    assert tags == pc.pipeline_tags(77, 12)
    assert tags[9:] == pc.pipeline_tags(77, 12, first_case=9)
    assert tags != pc.pipeline_tags(78, 12)
    genos = [g for _, g in pc.pipeline_cases(77, 12)]
    for (_, geno), first in zip(pc.pipeline_cases(77, 12, first_case=9), genos[9:]):
        assert np.array_equal(geno, first)
    bounds = dict(small=(1, 140, 1, 720), samples=(247, 2025, 1, 200), sites=(1, 70, 247, 4169))
    for size_class, (n0, n1, m0, m1) in bounds.items():
        for tag in pc.pipeline_tags(5, 8, size_class=size_class):
            assert tag["size_class"] == size_class
            assert n0 <= tag["n"] <= n1 and m0 <= tag["m"] <= m1
            assert 4 <= len(tag["calls"]) <= 10
            for call in tag["calls"]:
                assert call["kind"] in pc.KINDS and 0 <= call["stream"] < pc.NUM_STREAMS
                assert call["max_launch_blocks"] in (0, 3, 7)
                assert call["kind"] != "pair" or tag["n"] <= pc.PAIR_MAX_SAMPLES
                if call["kind"] in ("ld_edges", "ld_prune"):
                    assert call["window"] >= 2
                    assert tag["n"] * tag["m"] * (call["window"] - 1) <= pc.LD_WORK
                if call["kind"] == "pack_bed":
                    assert all(c % 64 == 0 and 0 < c < tag["m"] for c in call["cuts"])
                    assert call["offset"] % 2 == 1
    with pytest.raises(ValueError):
        pc.pipeline_tags(5, 1, size_class="huge")


def crosses(values, at):
    return any(v < at for v in values) and any(v >= at for v in values)


def committed_sweeps():
    import test_gpu_fuzz as sweeps
    return sweeps.PIPELINE_SWEEPS


@pytest.mark.parametrize("seed,cases,size_class", committed_sweeps())
def test_committed_sweeps_are_not_vacuous(oracle, seed, cases, size_class):
    f = pc.sweep_facts(seed, cases, size_class)
    print({k: v for k, v in f.items() if not isinstance(v, set)})
    assert f["cases"] == cases and all(f["calls"].values()), f["calls"]
    assert 2 * f["ld_partial"] >= f["ld"] > 0, "edges, but not the whole band"
    assert f["retries"] >= 1, "the default buffer overflows: one retry"
    assert f["exhausted"] >= 1, "a buffer too small"
    assert 2 * f["filter_both"] >= f["filters"] > 0, "filter_sites keeps and drops"
    assert f["filter_equal"] >= 1 and f["filter_nothing"] >= 1
    assert f["compact_gap"] >= 1, "an empty mask word between kept ones"
    assert pc.wps_changes(f["compact_kept"]), "both sides of a words_per_sample change"
    assert f["prune_ties"] >= 1 and f["prune_nan"] >= 1
    assert f["rounds2"] >= 1, "an unrelated_set of two rounds"
    assert f["streams"] == set(range(pc.NUM_STREAMS)) and f["tours"] >= 1
    assert f["n_mod8"] >= 1 and f["n_mod4"] >= 1
    if size_class == "samples":
        assert all(crosses(f["n_values"], at) for at in (256, 512, 2016)), sorted(f["n_values"])
    if size_class == "sites":
        assert crosses(f["m_values"], 4096), sorted(f["m_values"])
