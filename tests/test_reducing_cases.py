"""The expectations of the reducing calls (tests/reducing_cases.py) and the case generator of
their fuzzer (fuzz_cases.reducing_cases) checked on the CPU, before any kernel is judged by
them: against plain Python loops over the pairs, against the rules of include/cuking_amd.h
applied pair by pair with np.float32 scalars, against the record oracle (pyoracle.compute)
and against the naive oracle.

Cohorts: at most 40 samples and about 300 sites, 7 % missing calls, an all-missing sample
(NaN with everybody), a sample without hets (-inf) and a duplicate pair (0.5); the whole
cohort, a diagonal and an off-diagonal block of a split."""
import functools

import numpy as np
import pytest

import fuzz_cases
import reducing_cases as rc
from conftest import random_genotypes

f32 = np.float32
COHORTS = [(40, 300), (23, 311), (7, 64)]
BLOCKS = [(1, 0), (2, 1), (2, 2), (3, 4)]      # whole, off-diagonal, diagonal, off-diagonal
# one with a negative threshold, one with a threshold equal to a kinship that occurs
THRESHOLD_SETS = [(-0.5, 0.0442, 0.177), (0.0884, 0.354, 0.5)]


def make_genotypes(n, m):
    rng = np.random.default_rng(1000 * n + m)
    geno = random_genotypes(rng, n, m, missing=0.07)
    geno[1] = -1            # nothing defined: NaN with everybody
    geno[2] = 0             # no het site: -inf
    geno[n - 1] = geno[0]   # a duplicate pair: 0.5
    return geno


@functools.lru_cache(maxsize=None)
def block(n, m, split_factor, shard_index):
    """(genotypes, oracle block, its bitset, its ranges, the all_pairs result)."""
    from oracle import pyoracle
    geno = make_genotypes(n, m)
    osm = pyoracle.submatrix(n, split_factor, shard_index)
    bits = pyoracle.bitset_from_genotypes(geno, osm)
    return geno, osm, bits, osm.as_tuple(), pyoracle.all_pairs(osm, bits)


def every_block():
    return [(n, m, k, s) for n, m in COHORTS for k, s in BLOCKS]


def stored_offset(sm, sample, column):
    i_begin, i_end, j_begin, _ = sm
    if i_begin == j_begin or not column:
        return sample - (j_begin if column else i_begin)
    return sample - j_begin + (i_end - i_begin)


def test_cohorts_hold_the_special_values():
    _, _, _, sm, (oi, oj, _, kin) = block(40, 300, 1, 0)
    assert sm == (0, 40, 0, 40) and kin.size == 40 * 39 // 2
    assert np.isnan(kin[(oi == 1) | (oj == 1)]).all()
    assert np.isneginf(kin[((oi == 2) | (oj == 2)) & (oi != 1)]).all()
    assert kin[(oi == 0) & (oj == 39)][0] == f32(0.5)
    _, _, _, sm, (oi, oj, _, kin) = block(40, 300, 2, 1)
    assert sm == (0, 20, 20, 40) and kin.size == 400 and np.isnan(kin).any()


@pytest.mark.parametrize("n,m,k,shard", every_block())
def test_nearest_is_the_double_loop(n, m, k, shard):
    """Larger kinship, then lower partner; NaN never wins."""
    _, _, _, sm, pairs = block(n, m, k, shard)
    exp = rc.expect_all(sm, pairs, rc_bins(), THRESHOLD_SETS[0])
    oi, oj, kin = exp.pairs
    count = exp.keys.size
    best = [None] * count
    for i, j, x in zip(oi.tolist(), oj.tolist(), kin.tolist()):
        if x != x:
            continue
        for slot, partner in ((stored_offset(sm, i, False), j), (stored_offset(sm, j, True), i)):
            if best[slot] is None or x > best[slot][0] or \
                    (x == best[slot][0] and partner < best[slot][1]):
                best[slot] = (x, partner)
    got_kin, got_partner, got_keys = rc.nearest_of(sm, oi, oj, kin)
    for s in range(count):
        if best[s] is None:
            assert got_partner[s] == -1 and np.isnan(got_kin[s]) and got_keys[s] == 0
        else:
            assert got_partner[s] == best[s][1] and got_kin[s] == f32(best[s][0]), s
            assert got_keys[s] == rc.key_of(np.array([best[s][0]], dtype=f32),
                                            np.array([best[s][1]]))[0]
    # ... and expect_all's shorter way to the keys gives the same three arrays
    assert np.array_equal(exp.keys, got_keys) and np.array_equal(exp.best_partner, got_partner)
    assert np.array_equal(exp.best_kin.view(np.uint32), got_kin.view(np.uint32))
    if (n, k) == (40, 1):
        assert got_partner[1] == -1                         # the all-missing sample
        assert np.isneginf(got_kin[2]) and got_partner[2] == 0
        assert got_kin[0] == f32(0.5) and got_partner[0] == 39 and got_partner[39] == 0


def rc_bins():
    return fuzz_cases.BIN_MENU[0]


def slot_of(kin, lo, hi, num_bins):
    """include/cuking_amd.h, "Kinship summary": the slot of one float32 kinship."""
    lo, hi = f32(lo), f32(hi)
    scale = f32(f32(num_bins) / f32(hi - lo))
    if kin != kin:
        return num_bins + 2
    if kin < lo:
        return 0
    with np.errstate(over="ignore"):
        t = f32(f32(kin - lo) * scale)
    if not t < f32(num_bins):
        return num_bins + 1
    return 1 + int(t)


@pytest.mark.parametrize("bins", fuzz_cases.BIN_MENU)
def test_histogram_is_the_slot_rule_pair_by_pair(bins):
    for n, m, k, shard in every_block():
        _, _, _, sm, pairs = block(n, m, k, shard)
        kin = np.asarray(pairs[3], dtype=f32)
        want = np.zeros(bins[2] + 3, dtype=np.uint64)
        for x in kin:
            want[slot_of(x, *bins)] += np.uint64(1)
        got = rc.histogram_of(kin, *bins)
        assert got.dtype == np.uint64 and np.array_equal(got, want), (n, m, k, shard)
        assert int(got.sum()) == kin.size == (sm[1] - sm[0]) * (sm[3] - sm[2]) - \
            (0 if sm[0] != sm[2] else (sm[1] - sm[0]) * (sm[1] - sm[0] + 1) // 2)
    edge = np.array([bins[0], bins[1], np.nextafter(f32(bins[1]), f32(-1)), np.inf, -np.inf, np.nan],
                    dtype=f32)
    assert rc.slots_of(edge, *bins).tolist() == [slot_of(x, *bins) for x in edge]


@pytest.mark.parametrize("thresholds", THRESHOLD_SETS)
def test_suffix_sums_are_twice_the_records(thresholds):
    """Every record of the thresholded oracle names two samples: the strict `>` included (0.5
    is the duplicate's kinship, and no record at threshold 0.5 carries it)."""
    from oracle import pyoracle
    for n, m, k, shard in every_block():
        _, osm, bits, sm, (oi, oj, _, kin) = block(n, m, k, shard)
        counts = rc.counts_of(sm, oi.astype(np.int64), oj.astype(np.int64), kin, thresholds)
        assert counts.dtype == np.uint32
        suffix = counts[:, ::-1].astype(np.uint64).cumsum(axis=1)[:, ::-1]
        for t, thr in enumerate(thresholds):
            records, ovf, _ = pyoracle.compute(osm, bits, thr)
            assert ovf == 0 and int(suffix[:, t].sum()) == 2 * len(records), (n, m, k, shard, t)
            named = np.zeros(counts.shape[0], dtype=np.uint64)
            for r in records:
                named[stored_offset(sm, int(r["sample_i"]), False)] += np.uint64(1)
                named[stored_offset(sm, int(r["sample_j"]), True)] += np.uint64(1)
            assert np.array_equal(suffix[:, t], named)
    _, _, _, _, (_, _, _, kin) = block(40, 300, 1, 0)
    assert (kin == f32(0.5)).any() and rc.bands_of(np.array([0.5], dtype=f32), THRESHOLD_SETS[1])[0] == 1


@pytest.mark.parametrize("n,m,k,shard", every_block())
def test_matrix_is_the_naive_oracle(naive, n, m, k, shard):
    geno, _, _, sm, pairs = block(n, m, k, shard)
    exp = rc.expect_all(sm, pairs, rc_bins(), THRESHOLD_SETS[0])
    ni, nj, counts = naive.all_pairs_matmul(geno, (sm[0], sm[1]), (sm[2], sm[3]))
    want = np.full((sm[1] - sm[0], sm[3] - sm[2]), rc.SENTINEL, dtype=f32)
    want[ni.astype(np.int64) - sm[0], nj.astype(np.int64) - sm[2]] = \
        naive.kin_f32(counts[:, 0], counts[:, 1], counts[:, 2], counts[:, 3])
    assert exp.matrix.dtype == f32 and exp.matrix.shape == want.shape
    # (bit for bit, NaN patterns included: both are 0/0 of the same FPU)
    assert np.array_equal(exp.matrix.view(np.uint32), want.view(np.uint32))
    assert int((exp.matrix != rc.SENTINEL).sum()) == exp.pairs[2].size
    rc.assert_same(exp.matrix, want)
    if exp.pairs[2].size and not np.isnan(want).all():
        wrong = want.copy()
        where = tuple(np.argwhere(~np.isnan(want) & (want != rc.SENTINEL))[0])
        wrong[where] = np.nextafter(wrong[where], f32(1))
        with pytest.raises(AssertionError):
            rc.assert_same(wrong, want)
    # the histogram and the bands are those of the same pairs
    assert np.array_equal(exp.hist, rc.histogram_of(exp.pairs[2], *rc_bins()))
    assert np.array_equal(exp.bands, rc.counts_of(sm, *exp.pairs, THRESHOLD_SETS[0]))


def test_generator_is_deterministic():
    """The same seed gives the same cases, and `first_case` skips without changing later
    ones; every case is one the library serves."""
    tags = fuzz_cases.reducing_tags(77, 14)
    assert [t["case"] for t in tags] == list(range(14))
    assert tags == fuzz_cases.reducing_tags(77, 14)
    assert tags[9:] == fuzz_cases.reducing_tags(77, 14, first_case=9)
    assert tags != fuzz_cases.reducing_tags(78, 14)
    genos = [g for _, g in fuzz_cases.reducing_cases(77, 14)]
    for (tag, geno), first in zip(fuzz_cases.reducing_cases(77, 14, first_case=9), genos[9:]):
        assert np.array_equal(geno, first)
    for size_class, lo, hi in (("small", 2, 700), ("tiles", 1400, 2300), ("giveup", 5900, 6600)):
        for tag in fuzz_cases.reducing_tags(5, 6, size_class=size_class):
            assert tag["size_class"] == size_class and lo <= tag["n"] < hi
            assert tag["variant"] in fuzz_cases.REDUCING_VARIANTS
            assert tag["matrix_variant"] == "stream" or 0 <= tag["matrix_variant"] < 8
            thr = tag["thresholds"]
            assert 1 <= len(thr) <= 8 and all(a < b for a, b in zip(thr, thr[1:]))
            assert sorted(tag["order"]) == sorted(fuzz_cases.CALLS)
            assert tag["bins"] in fuzz_cases.BIN_MENU and 2 <= tag["tile_ranges"] <= 5
            shards = tag["split_factor"] * (tag["split_factor"] + 1) // 2
            assert 1 <= tag["split_factor"] <= 3 and 0 <= tag["shard"] < shards
            if size_class == "giveup":
                assert (tag["split_factor"], thr[0]) == (1, 0.0884) and 100 <= tag["m"] < 200
    with pytest.raises(ValueError):
        fuzz_cases.reducing_tags(5, 1, size_class="huge")


def test_committed_sweeps_compare_95_percent_bit_for_bit():
    """assert_same lets any NaN pass where the oracle is NaN: of the pairs of each sweep
    tests/test_gpu_fuzz.py runs, at least 95 % must have a kinship that is not NaN -- counted
    here from the generator and the oracle alone."""
    import test_gpu_fuzz as sweeps
    for seed, cases, size_class in sweeps.REDUCING_SWEEPS:
        pairs, compared = fuzz_cases.reducing_compared_share(seed, cases, size_class)
        print(f"run_reducing seed {seed} ({size_class}): {compared} of {pairs} pairs")
        assert pairs > 0 and compared >= 0.95 * pairs, (seed, cases, size_class)
