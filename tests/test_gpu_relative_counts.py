"""Relative counts (cuking_compute_relative_counts, KingContext.relative_counts) against the
CPU oracle's kinship of every pair (oracle.all_pairs) and the band rule of
include/cuking_amd.h in numpy float32; every comparison is exact integer equality.  And,
with no oracle, against the records of compute_king at each threshold.

Cohorts: 7 % missing calls; from 5 samples on an all-missing sample (NaN with everybody), a
sample without hets (-inf) and a duplicate pair (0.5); from 65 samples on a family built in
numpy from founders' haplotypes: two parents, two children (parent-child, siblings), a
grandchild and a great-grandchild.  Shapes: the smallest that cross a 128-sample tile (130),
a 256-sample tile (257) and a k-step of 256 sites (257, 1000, 3000 sites)."""
import ctypes as C
import functools

import numpy as np
import pytest

import cuking_amd
from cuking_amd import _lib
from reducing_cases import bands_of, counts_of

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1), (5, 32), (65, 257), (130, 1000), (257, 3000)]
KING = (0.0442, 0.0884, 0.177, 0.354)
THRESHOLD_SETS = [KING, (0.05,), (-0.5, 0.0, 0.25),
                  (-0.5, -0.1, 0.0, 0.0442, 0.0884, 0.177, 0.354, 0.45)]
CONTEXTS = [None, 6, 5]            # the context as it comes, then variants 6 and 5
f32, u32 = np.float32, np.uint32
# what the path-forcing cases change, and the shipped values they are put back to
DEFAULTS = dict(filter_quadrant_cap=384, filter_check0=1, filter_check1=1, filter_check_emit=64,
                filter_check_min_steps=64, filter_sort=1, split_wgs=256, reuse_prepared=0)


@pytest.fixture
def restored(ctx):
    """The shared context, put back the way it came."""
    variant = ctx.get_option("variant")
    yield ctx
    ctx.set_kernel("tiled")
    ctx.set_option("variant", variant)
    for key, value in DEFAULTS.items():
        ctx.set_option(key, value)
    ctx.invalidate()


def make_genotypes(n, m, seed, low_call=()):
    rng = np.random.default_rng(seed)
    af = rng.uniform(0.05, 0.5, size=m)
    hap = (rng.random((n, 2, m)) < af).astype(np.int8)       # founders: two haplotypes each
    sites = np.arange(m)

    def child(a, b):          # one haplotype of each parent per site, drawn freely
        return np.stack([hap[a, rng.integers(0, 2, m), sites], hap[b, rng.integers(0, 2, m), sites]])
    if n >= 65:
        hap[12], hap[13] = child(10, 11), child(10, 11)      # parent-child x 4, one sibling pair
        hap[15] = child(12, 14)                              # grandchild of 10 and 11
        hap[17] = child(15, 16)                              # great-grandchild of 10 and 11
    geno = hap.sum(axis=1).astype(np.int8)
    geno[rng.random((n, m)) < 0.07] = -1
    for s in low_call:
        geno[s, rng.random(m) < 0.30] = -1
    if n >= 5:
        geno[1] = -1            # nothing defined: NaN with everybody
        geno[2] = 0             # no het site: -inf
        geno[n - 1] = geno[3]   # a duplicate pair: 0.5
    return geno


# ---- the expectation, from the kinship of every pair ---------------------------------------
@functools.lru_cache(maxsize=None)
def cohort(n, m, split_factor=1, shard_index=0, low_call=()):
    """(bits of the block's samples, its ranges, (oi, oj, kin) of every pair).  Once per shape."""
    from oracle import pyoracle
    geno = make_genotypes(n, m, 1000 * n + m, low_call)
    osm = pyoracle.submatrix(n, split_factor, shard_index)
    sm = (osm.i_begin, osm.i_end, osm.j_begin, osm.j_end)
    idx = list(range(sm[0], sm[1]))
    if sm[0] != sm[2]:
        idx += list(range(sm[2], sm[3]))
    bits = pyoracle.bitset_from_genotypes(np.ascontiguousarray(geno[idx]))
    oi, oj, _, ok = pyoracle.all_pairs(osm, bits)
    pairs = (np.asarray(oi, dtype=np.int64), np.asarray(oj, dtype=np.int64),
             np.asarray(ok, dtype=f32))
    for a in pairs + (bits,):
        a.setflags(write=False)
    return bits, sm, pairs


@functools.lru_cache(maxsize=None)
def expectation(n, m, thresholds, split_factor=1, shard_index=0, low_call=()):
    _, sm, (oi, oj, kin) = cohort(n, m, split_factor, shard_index, low_call)
    out = counts_of(sm, oi, oj, kin, thresholds)
    out.setflags(write=False)
    return out


def check_counts(counts, exp, what=""):
    got = counts.bands()
    assert got.dtype == u32 and got.shape == exp.shape, what
    assert np.array_equal(got, exp), \
        f"{what}: counts differ at (sample, band) {np.argwhere(got != exp)[:8].tolist()}"
    suffix = exp[:, ::-1].astype(np.uint64).cumsum(axis=1)[:, ::-1]
    assert np.array_equal(counts.at_least(), suffix), what


def upload(ctx, bits):
    return ctx.upload_bitset(np.array(bits))


def run_whole(ctx, n, m, thresholds, low_call=(), **kw):
    bits, _, _ = cohort(n, m, low_call=low_call)
    return ctx.relative_counts(cuking_amd.Submatrix(n), bits.shape[1], upload(ctx, bits),
                               thresholds=thresholds, **kw)


# ---- tests -----------------------------------------------------------------------------------
def test_expectation_has_every_band():
    """ON THE EXPECTATION: at the two largest shapes every band of the KING cut-offs holds a
    pair, the duplicates sit in the last one, and NaN / -inf never get a band."""
    for n, m in SHAPES[-2:]:
        _, _, (oi, oj, kin) = cohort(n, m)
        exp = expectation(n, m, KING)
        assert (exp.sum(axis=0) > 0).all(), (n, m, exp.sum(axis=0))
        dup = (oi == 3) & (oj == n - 1)
        assert dup.sum() == 1 and kin[dup][0] == f32(0.5) and bands_of(kin[dup], KING)[0] == 3
        assert np.isnan(kin[(oi == 1) | (oj == 1)]).all() and exp[1].sum() == 0
        assert np.isneginf(kin[((oi == 2) | (oj == 2)) & (oi != 1)]).all() and exp[2].sum() == 0
    # (the third threshold set lets most pairs count)
    n, m = SHAPES[-1]
    assert expectation(n, m, THRESHOLD_SETS[2]).sum() > cuking_amd.Submatrix(n).NumPairs()


@pytest.mark.parametrize("thresholds", THRESHOLD_SETS, ids=lambda t: f"T{len(t)}")
@pytest.mark.parametrize("variant", CONTEXTS)
def test_bands_match_oracle(restored, variant, thresholds):
    if variant is not None:
        restored.set_option("variant", variant)
    for n, m in SHAPES:
        counts = run_whole(restored, n, m, thresholds)
        assert tuple(counts.counts.shape) == (n, len(thresholds))
        assert np.array_equal(counts.thresholds, np.asarray(thresholds, dtype=f32))
        check_counts(counts, expectation(n, m, thresholds), f"{n} x {m}")


def totals(ctx):
    return {k: ctx.get_option(k) for k in ("filter_candidates", "filter_dense_quadrants",
                                            "filter_early_exits")}


LOW_CALL = (7, 40, 129, 200)      # a few 30 %-missing samples: the sorted layout's case
# (name, options, thresholds, low-call samples, the counters that must move, must not move)
PATHS = [
    # every quadrant below the cap: the candidate list and the counting refine kernel
    ("refine", dict(filter_quadrant_cap=16384, filter_check0=0, filter_check1=0), (0.177, 0.354),
     (), ("filter_candidates",), ("filter_early_exits",)),
    # cap 0: every quadrant with a candidate goes to the four-product kernel's list launch
    ("dense quadrants", dict(filter_quadrant_cap=0, filter_check0=0, filter_check1=0), KING, (),
     ("filter_dense_quadrants",), ()),
    # a lowest threshold inside the level of the bound for unrelated pairs: every tile gives
    # up at once and the gated fallback computes the block
    ("gated fallback", dict(), (0.001, 0.0884), (), ("filter_dense_quadrants",),
     ("filter_candidates",)),
    # the forecast forced on a short bitset: tiles that look dense leave inside the k loop
    ("forecast", dict(filter_check_min_steps=4, filter_check0=2), (0.05,), (), (), ()),
    # the rigorous check forced, tiles hand over nothing there
    ("rigorous check", dict(filter_check_min_steps=4, filter_check1=3, filter_check_emit=0),
     (0.354,), (), (), ()),
    ("rigorous check, hand-over", dict(filter_check_min_steps=4, filter_check1=3), KING, (), (), ()),
    ("unsorted layout", dict(filter_sort=0), KING, LOW_CALL, (), ()),
    # (without the forecast's switch: these heavily missing cohorts would give up at once)
    ("sorted layout", dict(filter_sort=1, filter_check0=0), KING, LOW_CALL,
     ("filter_candidates",), ()),
    ("sorted layout, dense", dict(filter_sort=1, filter_check0=0, filter_quadrant_cap=0), KING,
     LOW_CALL, ("filter_dense_quadrants",), ()),
    ("remainder pieces", dict(split_wgs=6, filter_check0=0), KING, (), (), ()),
]


@pytest.mark.parametrize("name,options,thresholds,low_call,moved,still", PATHS,
                         ids=[p[0] for p in PATHS])
def test_forced_paths(restored, name, options, thresholds, low_call, moved, still):
    """The refine path, the dense-quadrant path and the gated fallback of the default context,
    each forced with the test hooks; the diagnostic counters say the path was taken."""
    assert restored.get_option("variant") == 7
    n, m = SHAPES[-1]
    for key, value in options.items():
        restored.set_option(key, value)
    before = totals(restored)
    counts = run_whole(restored, n, m, thresholds, low_call)
    check_counts(counts, expectation(n, m, thresholds, low_call=low_call), name)
    after = totals(restored)
    print(name, {k: after[k] - before[k] for k in after})
    for key in moved:
        assert after[key] > before[key], (name, key, before, after)
    for key in still:
        assert after[key] == before[key], (name, key, before, after)


def test_early_exits_and_remainder_pieces_of_the_other_kernels(restored):
    """Tiles without a close relative leave at the rigorous check (600 samples: three tiles hold
    unrelated pairs only, whose bound lies far below 0.354 after 50/64 of the sites); the four-
    and five-product kernels cut a remainder into pieces."""
    n, m, thresholds = 600, 3000, (0.354, 0.45)
    exp = expectation(n, m, thresholds)
    restored.set_option("filter_check_min_steps", 4)
    restored.set_option("filter_check0", 0)
    restored.set_option("filter_check1", 3)
    before = totals(restored)
    check_counts(run_whole(restored, n, m, thresholds), exp, "early exits")
    after = totals(restored)
    print("early exits", {k: after[k] - before[k] for k in after})
    assert after["filter_early_exits"] > before["filter_early_exits"]
    restored.set_option("split_wgs", 6)
    for variant in (7, 6, 5):
        restored.set_option("variant", variant)
        check_counts(run_whole(restored, n, m, thresholds), exp, f"split_wgs 6, variant {variant}")


@pytest.mark.parametrize("variant", CONTEXTS)
def test_counts_equal_the_records(restored, variant):
    """No oracle: for each threshold the suffix-summed counts are the number of records of
    compute_king at that threshold that name the sample; num_records is their number; and
    count_records sizes a record call exactly."""
    import torch
    if variant is not None:
        restored.set_option("variant", variant)
    n, m = SHAPES[-1]
    bits, _, _ = cohort(n, m)
    sm, wps, d_bits = cuking_amd.Submatrix(n), bits.shape[1], upload(restored, bits)
    counts = restored.relative_counts(sm, wps, d_bits)
    assert np.array_equal(counts.thresholds, np.asarray(KING, dtype=f32))
    at_least = counts.at_least()
    for t, thr in enumerate(counts.thresholds):
        recs = restored.run(sm, wps, d_bits, float(thr))
        named = np.bincount(recs["sample_i"], minlength=n) + np.bincount(recs["sample_j"], minlength=n)
        assert np.array_equal(at_least[:, t], named.astype(np.uint64)), t
        assert counts.num_records(t) == len(recs) > 0
    need = restored.count_records(sm, wps, d_bits, KING[0])
    assert need == counts.num_records(0)
    results = torch.zeros((need, 6), dtype=torch.int32, device="cuda:0")
    index_flag = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    restored.compute_king(sm, wps, d_bits, KING[0], need, results, index_flag[0:1], index_flag[1:2])
    torch.cuda.synchronize()
    assert index_flag.tolist() == [need, 0]        # neither an overflow nor a slot unused


@pytest.mark.parametrize("shard", [0, 1, 2])
def test_blocks_of_a_split(ctx, shard):
    n, m = 300, 1000
    bits, sm, (oi, oj, kin) = cohort(n, m, 2, shard)
    block = cuking_amd.Submatrix(n, split_factor=2, shard_index=shard)
    assert block.as_tuple() == sm and kin.size == block.NumPairs()
    counts = ctx.relative_counts(block, bits.shape[1], upload(ctx, bits))
    assert counts.counts.shape[0] == block.NumSamples() == (300 if shard == 1 else 150)
    check_counts(counts, expectation(n, m, KING, 2, shard), f"shard {shard}")
    recs = ctx.run(block, bits.shape[1], upload(ctx, bits), KING[0])
    assert counts.num_records(0) == len(recs) == int((bands_of(kin, KING) >= 0).sum())


@pytest.mark.parametrize("variant", [None, 6])
def test_accumulates_tile_ranges_and_out(restored, variant):
    """Two disjoint halves of the tiles into one zeroed output equal the whole call; one half
    alone is partial; a pre-filled output gains exactly the counts; `out` is what comes back."""
    import torch
    if variant is not None:
        restored.set_option("variant", variant)
    n, m = 600, 2000
    bits, _, _ = cohort(n, m)
    exp = expectation(n, m, KING)
    sm, wps, d_bits = cuking_amd.Submatrix(n), bits.shape[1], upload(restored, bits)
    tiles = restored.num_tiles(sm)
    assert tiles >= 2
    half = tiles // 2
    counts = restored.relative_counts(sm, wps, d_bits, tile_range=(0, half))
    first = counts.bands()
    assert (first <= exp).all() and 0 < int(first.sum()) < int(exp.sum())
    again = restored.relative_counts(sm, wps, d_bits, tile_range=(half, tiles), out=counts.counts)
    assert again.counts is counts.counts
    check_counts(counts, exp, "two halves")
    out = torch.full((n, len(KING)), 1000, dtype=torch.int32, device="cuda:0")
    filled = restored.relative_counts(sm, wps, d_bits, out=out)
    assert filled.counts is out
    assert np.array_equal(filled.bands(), exp + u32(1000))
    for bad in (torch.zeros((n, 3), dtype=torch.int32, device="cuda:0"),
                torch.zeros((n, 4), dtype=torch.int64, device="cuda:0"),
                torch.zeros((n, 8), dtype=torch.int32, device="cuda:0")[:, ::2]):
        with pytest.raises(ValueError):
            restored.relative_counts(sm, wps, d_bits, out=bad)
    st = restored.lib.cuking_compute_relative_counts_tiles(
        restored.handle, C.byref(sm.c), wps, d_bits.data_ptr(), 0, tiles + 1,
        (C.c_float * 1)(0.1), 1, out.data_ptr(), None)
    assert st == _lib.ERR_INVALID_ARGUMENT and b"tile range" in restored.lib.cuking_last_error()


def test_prepared_layout_is_shared_with_the_record_call(restored):
    """reuse_prepared = 1: a count call and a record call on the same bitset convert once (they
    are the same kind of call); a dense matrix in between makes the next count call convert
    again."""
    from oracle import pyoracle
    n, m = SHAPES[-1]
    bits, _, _ = cohort(n, m, low_call=LOW_CALL)
    exp = expectation(n, m, KING, low_call=LOW_CALL)
    records, ovf, _ = pyoracle.compute(pyoracle.submatrix(n), np.array(bits), KING[1])
    assert ovf == 0 and len(records) > 0
    sm, wps, d_bits = cuking_amd.Submatrix(n), bits.shape[1], upload(restored, bits)
    restored.set_option("reuse_prepared", 1)
    restored.invalidate()
    skipped = lambda: restored.get_option("conversions_skipped")     # noqa: E731
    at = skipped()
    check_counts(restored.relative_counts(sm, wps, d_bits), exp, "first call")
    assert skipped() == at
    assert restored.run(sm, wps, d_bits, KING[1]).tobytes() == records.tobytes()
    assert skipped() == at + 1
    check_counts(restored.relative_counts(sm, wps, d_bits), exp, "after the records")
    assert skipped() == at + 2
    restored.kin_matrix(sm, wps, d_bits)
    assert skipped() == at + 2
    check_counts(restored.relative_counts(sm, wps, d_bits), exp, "after a dense matrix")
    assert skipped() == at + 2                   # converted again
    assert restored.run(sm, wps, d_bits, KING[1]).tobytes() == records.tobytes()
    assert skipped() == at + 3


def test_refused_widths_and_contexts(restored):
    """From 2^24 sites on the call is refused; so are the VALU variants and the stream
    kernel -- nothing is written."""
    import torch
    wide = cuking_amd.words_per_sample((1 << 24) + 64)
    d_wide = torch.zeros((6, wide), dtype=torch.int64, device="cuda:0")
    with pytest.raises(cuking_amd.CukingError) as e:
        restored.relative_counts(cuking_amd.Submatrix(6), wide, d_wide)
    assert e.value.status == _lib.ERR_INVALID_ARGUMENT and "2^24" in e.value.message
    del d_wide
    n, m = 65, 257
    bits, _, _ = cohort(n, m)
    sm = cuking_amd.Submatrix(n)
    out = torch.full((n, 4), 77, dtype=torch.int32, device="cuda:0")
    for kernel, variant in (("stream", None), ("tiled", 0), ("tiled", 2)):
        restored.set_kernel(kernel)
        if variant is not None:
            restored.set_option("variant", variant)
        for tile_range in (None, (0, 1)):
            with pytest.raises(cuking_amd.CukingError) as e:
                restored.relative_counts(sm, bits.shape[1], upload(restored, bits), out=out,
                                         tile_range=tile_range)
            assert e.value.status == _lib.ERR_INVALID_ARGUMENT
            assert "variant 5, 6 or 7" in e.value.message
        restored.set_kernel("tiled")
        restored.set_option("variant", 7)
    torch.cuda.synchronize()
    assert (out == 77).all()
