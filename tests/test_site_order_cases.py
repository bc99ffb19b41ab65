"""The site-order sweep judged on the CPU (tests/site_order_cases.py): the conditions its
committed seeds rest on, from the generator and the oracle alone -- a sweep that met none of
them would pass without having tested the order -- the generator's determinism, the records
it derives from ONE all_pairs call against pyoracle.compute, and that the four older
generators still name the cases they named."""
import hashlib

import numpy as np
import pytest

import fuzz_cases
import site_order_cases as so


def sweep_conditions(seed, cases):
    """What one committed sweep is counted by."""
    c = dict(cases=0, expect_order=0, off_diagonal=0, four_steps=0, filter_threshold=0,
             with_record=0, under_256_sites=0, two_or_three_stored=0, kinds=set(), gathers=set(),
             orders=set(), outside=0)
    for tag, geno in so.site_order_cases(seed, cases):
        osm, bits, all_pairs = so.site_order_oracle(tag, geno)
        i0, _, j0, _ = osm.as_tuple()
        c["cases"] += 1
        c["expect_order"] += so.expects_order(tag)
        c["off_diagonal"] += i0 != j0
        c["four_steps"] += -(-tag["m"] // so.K_STEP_SITES) >= 4
        if 0.0 < tag["thr"] < 0.5:
            c["filter_threshold"] += 1
            c["with_record"] += len(so.records_of(all_pairs, tag["thr"])) > 0
        else:
            c["outside"] += 1
        c["under_256_sites"] += tag["m"] < 256
        c["two_or_three_stored"] += so.stored_samples(tag) in (2, 3)
        c["kinds"] |= set(tag["calls"])
        c["orders"].add(tag["filter_site_order"])
        if so.expects_order(tag):
            c["gathers"].add(tag["filter_site_gather"])
        assert bits.shape[0] == so.stored_samples(tag) >= 2
    return c


def test_committed_sweeps_meet_their_conditions():
    import test_gpu_fuzz as sweeps
    for seed, cases in sweeps.SITE_ORDER:
        c = sweep_conditions(seed, cases)
        print(f"run_site_order seed {seed}: {c}")
        assert c["cases"] == cases
        assert 2 * c["expect_order"] >= cases, (seed, c)
        assert 5 * c["off_diagonal"] >= cases, (seed, c)
        assert 3 * c["four_steps"] >= cases, (seed, c)
        assert 5 * c["with_record"] >= 4 * c["filter_threshold"] > 0, (seed, c)
        assert c["under_256_sites"] >= 4 and c["two_or_three_stored"] >= 4, (seed, c)
        assert c["kinds"] == set(so.KINDS), (seed, c)
        # (every gather value in a case whose layout must be ordered: the form really runs)
        assert c["gathers"] == set(so.GATHERS), (seed, c)
        assert c["orders"] == {-1, 1, 2} and c["outside"] >= 1, (seed, c)


def test_generator_is_deterministic():
    """The same seed gives the same cases, and `first_case` skips without changing later
    ones; every case is one the sweep can run."""
    tags = so.site_order_tags(77, 14)
    assert [t["case"] for t in tags] == list(range(14))
    assert tags == so.site_order_tags(77, 14)
    assert tags[9:] == so.site_order_tags(77, 14, first_case=9)
    assert tags != so.site_order_tags(78, 14)
    genos = [g for _, g in so.site_order_cases(77, 14)]
    for (tag, geno), first in zip(so.site_order_cases(77, 14, first_case=9), genos[9:]):
        assert np.array_equal(geno, first)
    for tag in so.site_order_tags(5, 60):
        assert 2 <= tag["n"] < 700 or 1400 <= tag["n"] < 2300
        assert 1 <= tag["m"] < 24000 and (tag["n"] < 1400 or tag["m"] < 6000)
        shards = tag["split_factor"] * (tag["split_factor"] + 1) // 2
        assert 1 <= tag["split_factor"] <= 3 and 0 <= tag["shard"] < shards
        assert tag["n"] >= 2 * tag["split_factor"]
        assert tag["thr"] in so.MENU + so.OUTSIDE and tag["thr2"] in so.MENU
        thr = tag["thresholds"]
        assert thr[0] == tag["thr"] and 1 <= len(thr) <= 4
        assert all(a < b for a, b in zip(thr, thr[1:]))
        assert 3 <= len(tag["calls"]) <= 6 and len(set(tag["calls"])) == len(tag["calls"])
        assert set(tag["calls"]) <= set(so.KINDS) and set(tag["calls"]) & set(so.WHOLE)
        assert "staged" not in tag["calls"] or tag["split_factor"] == 1
        assert tag["filter_site_order"] in (-1, 1, 2)
        assert tag["filter_site_gather"] in so.GATHERS and tag["counts_mode"] in (-1, 0, 1)
        assert len(tag["streams"]) == tag["world"]


def test_the_rule_of_the_expected_flag():
    base = dict(n=600, m=3000, split_factor=1, shard=0, counts_mode=0, filter_site_order=1,
                thr=0.0884, thr2=0.177)
    assert so.expected_flag(base, "run", 0.0884) == 1
    assert so.expected_flag(dict(base, filter_site_order=2), "relative_counts", 0.354) == 1
    assert so.expected_flag(dict(base, filter_site_order=-1), "run", 0.0884) is None
    for thr in so.OUTSIDE:            # the filter does not run: stored order, whatever else
        assert so.expected_flag(dict(base, filter_site_order=-1), "run", thr) == 0
        assert so.expected_flag(base, "relative_counts", thr) == 0
    assert so.expected_flag(dict(base, counts_mode=1), "run", 0.0884) == 0
    assert so.expected_flag(dict(base, counts_mode=-1), "run2", 0.177) is None
    assert so.expected_flag(dict(base, counts_mode=1), "relative_counts", 0.0884) == 1
    assert so.expected_flag(dict(base, m=64 * 4096), "run", 0.0884) == 1
    assert so.expected_flag(dict(base, m=64 * 4096 + 1), "run", 0.0884) == 0
    assert so.expected_flag(dict(base, n=2), "run", 0.0884) == 1


def test_records_from_all_pairs_are_the_oracles_records(oracle):
    """records_of against pyoracle.compute, byte for byte, at both thresholds of generated
    cases -- off-diagonal blocks, a threshold outside (0, 1/2) and an empty result among them."""
    seen = set()
    for tag, geno in so.site_order_cases(31, 40):
        if tag["n"] >= 1400:
            continue
        osm, bits, all_pairs = so.site_order_oracle(tag, geno)
        for thr in (tag["thr"], tag["thr2"]):
            want, ovf, _ = oracle.compute(osm, bits, thr)
            got = so.records_of(all_pairs, thr)
            assert ovf == 0 and got.dtype == want.dtype
            assert got.tobytes() == want.tobytes(), (tag["case"], thr)
            seen |= {("empty", len(want) == 0), ("outside", not 0 < thr < 0.5),
                     ("off-diagonal", osm.i_begin != osm.j_begin)}
    assert {(k, True) for k in ("empty", "outside", "off-diagonal")} <= seen, seen


def digest(tags) -> str:
    return hashlib.sha256(repr(tags).encode()).hexdigest()[:16]


def test_the_older_generators_name_the_cases_they_named():
    """The sweep has a generator of its own: no draw was added to the others (digests of the
    tags of a committed seed, taken before the sweep was added)."""
    import pipeline_cases as pc
    assert digest(fuzz_cases.reducing_tags(301, 12)) == REDUCING_301
    assert digest([tag for tag, _ in pc.pipeline_cases(401, 12, 0, "small")]) == PIPELINE_401


REDUCING_301 = "43f0ccbd1560cfba"
PIPELINE_401 = "aca3f80a9a8a1379"
