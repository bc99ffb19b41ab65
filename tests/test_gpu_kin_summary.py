"""Kinship summary (cuking_compute_kin_summary, KingContext.kin_summary) against the CPU
oracle's kinship of every pair (oracle.all_pairs), the slot rule of include/cuking_amd.h
restated in numpy float32 operations, and a numpy arg-max with the tie rule (larger kinship,
then lower partner).  Every comparison is exact: integer equality of counts and keys,
bit-equal floats.

Cohorts as in test_gpu_kin_matrix.py: 7 % missing calls; from 5 samples on an all-missing
sample (NaN with everybody), a sample without hets (-inf) and a duplicate pair (0.5).
Shapes: the smallest that cross a 128-sample tile (130), a 256-sample tile (257) and a
k-step of 256 sites (257, 1000, 3000 sites)."""
import ctypes as C
import functools

import numpy as np
import pytest

import cuking_amd
from cuking_amd import _lib
from conftest import random_genotypes
from reducing_cases import histogram_of, nearest_of, slots_of

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1), (5, 32), (65, 257), (130, 1000), (257, 3000)]
BIN_SETS = [(-1.0, 0.5, 1536), (-0.25, 0.25, 7)]
CONTEXTS = [None, 6, 5]            # the context as it comes, then variants 6 and 5
SENTINEL = 0x5A5A5A5A5A5A5A5A
f32, u32, u64 = np.float32, np.uint32, np.uint64


@pytest.fixture
def restored(ctx):
    """The shared context, put back the way it came."""
    variant = ctx.get_option("variant")
    yield ctx
    ctx.set_kernel("tiled")
    ctx.set_option("variant", variant)


def make_genotypes(n, m, seed, low_call=()):
    rng = np.random.default_rng(seed)
    geno = random_genotypes(rng, n, m, missing=0.07)
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
def expectation(n, m, lo, hi, num_bins, split_factor=1, shard_index=0, low_call=()):
    _, sm, (oi, oj, kin) = cohort(n, m, split_factor, shard_index, low_call)
    hist = histogram_of(kin, lo, hi, num_bins)
    best_kin, best_partner, keys = nearest_of(sm, oi, oj, kin)
    for a in (hist, best_kin, best_partner, keys):
        a.setflags(write=False)
    return hist, keys, best_kin, best_partner


def same_floats(a, b):
    nan = np.isnan(b)
    return a.dtype == b.dtype == f32 and np.isnan(a[nan]).all() and \
        np.array_equal(a.view(u32)[~nan], b.view(u32)[~nan])


def check_summary(summary, exp, pairs, what=""):
    hist, keys, best_kin, best_partner = exp
    got = summary.counts()
    assert got.dtype == u64 and np.array_equal(got, hist), \
        f"{what}: histogram differs at slots {np.flatnonzero(got != hist)[:8]}"
    assert int(got.sum()) == pairs, what
    got_keys = summary.keys()
    assert np.array_equal(got_keys, keys), \
        f"{what}: keys differ at samples {np.flatnonzero(got_keys != keys)[:8]}"
    kin, partner = summary.nearest()
    assert partner.dtype == np.int64 and np.array_equal(partner, best_partner), what
    assert same_floats(kin, best_kin), what


def run_whole(ctx, n, m, bins, **kw):
    bits, _, _ = cohort(n, m)
    return ctx.kin_summary(cuking_amd.Submatrix(n), bits.shape[1],
                           ctx.upload_bitset(np.array(bits)), lo=bins[0], hi=bins[1],
                           bins=bins[2], **kw)


# ---- tests -----------------------------------------------------------------------------------
@pytest.mark.parametrize("bins", BIN_SETS)
@pytest.mark.parametrize("variant", CONTEXTS)
def test_histogram_and_nearest(restored, variant, bins):
    if variant is not None:
        restored.set_option("variant", variant)
    for n, m in SHAPES:
        exp = expectation(n, m, *bins)
        _, _, (oi, oj, kin) = cohort(n, m)
        summary = run_whole(restored, n, m, bins)
        assert summary.hist.numel() == bins[2] + 3 and summary.best.numel() == n
        assert (summary.lo, summary.hi, summary.bins) == bins
        check_summary(summary, exp, cuking_amd.Submatrix(n).NumPairs(), f"{n} x {m}")
        if n < 5:
            continue
        hist, keys, best_kin, best_partner = exp
        # NaN, -inf and an exact 0.5 really occur
        assert hist[bins[2] + 2] > 0 and hist[0] > 0 and (kin == f32(0.5)).any()
        assert keys[1] == 0 and best_partner[1] == -1          # the all-missing sample
        # the sample without hets: -inf at its lowest partner that gives -inf and not NaN
        of_2 = (oi == 2) | (oj == 2)
        partners = np.where(oi == 2, oj, oi)[of_2 & np.isneginf(kin)]
        assert not (kin[of_2] > f32("-inf")).any() and partners.size > 0
        got_kin, got_partner = summary.nearest()
        assert np.isneginf(got_kin[2]) and got_partner[2] == partners.min()
        assert got_kin[3] == f32(0.5) and got_partner[3] == n - 1 and got_partner[n - 1] == 3


def test_off_diagonal_block(ctx):
    bins = BIN_SETS[0]
    bits, sm, (oi, oj, kin) = cohort(300, 1000, 2, 1)
    block = cuking_amd.Submatrix(300, split_factor=2, shard_index=1)
    assert block.as_tuple() == sm == (0, 150, 150, 300) and kin.size == 150 * 150
    summary = ctx.kin_summary(block, bits.shape[1], ctx.upload_bitset(np.array(bits)),
                              lo=bins[0], hi=bins[1], bins=bins[2])
    assert summary.best.numel() == 300
    exp = expectation(300, 1000, *bins, 2, 1)
    check_summary(summary, exp, 150 * 150)
    _, partner = summary.nearest()
    # rows first, then columns; partners are global indices of the other side
    assert ((partner[:150] >= 150) | (partner[:150] == -1)).all()
    assert (partner[150:] < 150).all() and (partner[150:] >= -1).all()


@pytest.mark.parametrize("variant", [None, 6])
def test_accumulates_and_tile_ranges(restored, variant):
    """Three disjoint tile ranges into one zeroed pair of outputs equal the whole call; one
    range alone is partial; a second whole call doubles the counts and leaves the keys."""
    if variant is not None:
        restored.set_option("variant", variant)
    n, m, bins = 600, 2000, BIN_SETS[0]
    bits, _, _ = cohort(n, m)
    exp = expectation(n, m, *bins)
    sm = cuking_amd.Submatrix(n)
    d_bits = restored.upload_bitset(np.array(bits))
    tiles = restored.num_tiles(sm)
    parts = np.zeros(6, dtype=np.uint64)
    restored.lib.cuking_schedule_tile_partition(tiles, 3, parts.ctypes.data)
    ranges = [(int(parts[2 * r]), int(parts[2 * r + 1])) for r in range(3)]
    assert tiles >= 3 and ranges[0][0] == 0 and ranges[2][1] == tiles
    kw = dict(lo=bins[0], hi=bins[1], bins=bins[2])
    summary = restored.kin_summary(sm, bits.shape[1], d_bits, tile_range=ranges[0], **kw)
    first = summary.counts()
    assert 0 < int(first.sum()) < sm.NumPairs() and (first <= exp[0]).all()
    assert (summary.keys() <= exp[1]).all()
    for r in ranges[1:]:
        again = restored.kin_summary(sm, bits.shape[1], d_bits, tile_range=r,
                                     hist=summary.hist, best=summary.best, **kw)
        assert again.hist is summary.hist and again.best is summary.best
    check_summary(summary, exp, sm.NumPairs(), "three ranges")
    restored.kin_summary(sm, bits.shape[1], d_bits, hist=summary.hist, best=summary.best, **kw)
    assert np.array_equal(summary.counts(), 2 * exp[0])
    assert np.array_equal(summary.keys(), exp[1])


def test_launch_shapes(restored):
    """Several launches, remainder pieces, the dynamic tail: the same summary each time (the
    histogram's sum catches an epilogue that runs twice or not at all for a split tile)."""
    n, m, bins = 600, 2000, BIN_SETS[0]
    exp = expectation(n, m, *bins)
    pairs = cuking_amd.Submatrix(n).NumPairs()

    def check(what):
        check_summary(run_whole(restored, n, m, bins), exp, pairs, what)
    try:
        restored.set_option("max_launch_blocks", 3)
        check("max_launch_blocks 3")
        restored.set_option("variant", 5)
        check("max_launch_blocks 3, variant 5")
        restored.set_option("max_launch_blocks", 0)
        restored.set_option("split_wgs", 6)
        for variant in (6, 5):
            restored.set_option("variant", variant)
            check(f"split_wgs 6, variant {variant}")
        restored.set_option("variant", 7)
        check("split_wgs 6, variant 7")
        restored.set_option("split_wgs", 256)
        restored.set_option("dyn_tail_tiles", 1)
        for variant in (7, 6):
            restored.set_option("variant", variant)
            check(f"dyn_tail_tiles 1, variant {variant}")
        restored.set_option("xcd_swizzle", 0)
        check("xcd_swizzle 0")
    finally:
        restored.set_option("max_launch_blocks", 0)
        restored.set_option("split_wgs", 256)
        restored.set_option("dyn_tail_tiles", 16384)
        restored.set_option("xcd_swizzle", 2)


def test_single_outputs(ctx):
    """d_hist alone and d_best alone each give their half; the words around the output passed
    and the buffer of the output not passed keep their sentinel."""
    import torch
    n, m, bins = 130, 1000, BIN_SETS[1]
    bits, _, _ = cohort(n, m)
    hist, keys, _, _ = expectation(n, m, *bins)
    sm = cuking_amd.Submatrix(n)
    d_bits = ctx.upload_bitset(np.array(bits))
    cbins = _lib.CKinBins(*bins)
    pad, slots = 16, bins[2] + 3
    sentinel = np.array(SENTINEL, dtype=u64).view(np.int64).item()

    def buffer(length):
        t = torch.full((length + 2 * pad,), sentinel, dtype=torch.int64, device="cuda:0")
        t[pad:pad + length] = 0
        return t

    def host(t):
        torch.cuda.synchronize()
        return t.cpu().numpy().view(u64)

    def padding_intact(t, length):
        h = host(t)
        return (h[:pad] == SENTINEL).all() and (h[pad + length:] == SENTINEL).all()

    d_hist, d_best = buffer(slots), buffer(n)
    other_best = torch.full((n,), sentinel, dtype=torch.int64, device="cuda:0")
    other_hist = torch.full((slots,), sentinel, dtype=torch.int64, device="cuda:0")
    args = (ctx.handle, C.byref(sm.c), bits.shape[1], d_bits.data_ptr())
    _lib.check(ctx.lib.cuking_compute_kin_summary(
        *args, C.byref(cbins), d_hist.data_ptr() + 8 * pad, None, None))
    assert np.array_equal(host(d_hist)[pad:pad + slots], hist) and padding_intact(d_hist, slots)
    assert (host(other_best) == SENTINEL).all() and (host(d_best)[pad:pad + n] == 0).all()
    _lib.check(ctx.lib.cuking_compute_kin_summary(
        *args, None, None, d_best.data_ptr() + 8 * pad, None))
    assert np.array_equal(host(d_best)[pad:pad + n], keys) and padding_intact(d_best, n)
    assert np.array_equal(host(d_hist)[pad:pad + slots], hist) and padding_intact(d_hist, slots)
    assert (host(other_hist) == SENTINEL).all()
    # ... and the tiles form, both halves at once over the whole range
    d_hist, d_best = buffer(slots), buffer(n)
    _lib.check(ctx.lib.cuking_compute_kin_summary_tiles(
        *args, 0, ctx.num_tiles(sm), C.byref(cbins), d_hist.data_ptr() + 8 * pad,
        d_best.data_ptr() + 8 * pad, None))
    assert np.array_equal(host(d_hist)[pad:pad + slots], hist) and padding_intact(d_hist, slots)
    assert np.array_equal(host(d_best)[pad:pad + n], keys) and padding_intact(d_best, n)
    st = ctx.lib.cuking_compute_kin_summary_tiles(
        *args, 0, ctx.num_tiles(sm) + 1, C.byref(cbins), d_hist.data_ptr() + 8 * pad, None, None)
    assert st == _lib.ERR_INVALID_ARGUMENT and b"tile range" in ctx.lib.cuking_last_error()


def test_agrees_with_kin_matrix(ctx):
    """No CPU oracle: 78+ tiles merge through global atomics, and the summary equals what the
    host derives from the dense matrix of the same bitset."""
    import torch
    from oracle import pyoracle
    n, m, bins = 1500, 5000, (0.0, 0.5001, 4096)
    bits = pyoracle.bitset_from_genotypes(np.ascontiguousarray(make_genotypes(n, m, 15005000)))
    sm = cuking_amd.Submatrix(n)
    d_bits = ctx.upload_bitset(bits)
    assert ctx.num_tiles(sm) * (ctx.tile_samples() // 128) ** 2 >= 78
    matrix = ctx.kin_matrix(sm, bits.shape[1], d_bits)
    summary = ctx.kin_summary(sm, bits.shape[1], d_bits, lo=bins[0], hi=bins[1], bins=bins[2])
    torch.cuda.synchronize()
    oi, oj = np.triu_indices(n, 1)
    kin = matrix.cpu().numpy()[oi, oj]
    best_kin, best_partner, keys = nearest_of((0, n, 0, n), oi, oj, kin)
    check_summary(summary, (histogram_of(kin, *bins), keys, best_kin, best_partner),
                  sm.NumPairs())
    assert summary.count_at_least(0) == int(summary.counts()[1:bins[2] + 2].sum())
    # hi lies above 0.5: OVER stays empty, and the duplicates sit in one of the last bins
    assert summary.count_at_least(bins[2]) == int(summary.counts()[bins[2] + 1]) == 0
    slots = slots_of(kin, *bins)
    dup = int(slots_of(np.array([0.5], dtype=f32), *bins)[0])
    assert 1 <= dup <= bins[2] and (kin == f32(0.5)).any()
    assert summary.count_at_least(dup - 1) == int(((slots >= dup) & (slots <= bins[2] + 1)).sum()) > 0


def test_wide_route(ctx):
    """From 2^22 sites on the default context hands the block to the five-product kernel: the
    same summary; from 2^24 sites on the call is refused."""
    from oracle import pyoracle
    n, bins = 6, BIN_SETS[0]
    sites = (1 << 22) + 64
    wps = cuking_amd.words_per_sample(sites)
    rng = np.random.default_rng(sites)
    bits = rng.integers(0, 1 << 63, size=(n, wps), dtype=np.uint64) << np.uint64(1) | \
        rng.integers(0, 2, size=(n, wps), dtype=np.uint64)
    bits[:, wps // 2 - 1] = ~np.uint64(0)      # the het plane's last word ...
    bits[:, wps - 1] = ~np.uint64(0)           # ... and the hom_var plane's: missing
    bits[1] = ~np.uint64(0)
    oi, oj, _, ok = pyoracle.all_pairs(pyoracle.submatrix(n), bits)
    oi, oj, kin = np.asarray(oi, np.int64), np.asarray(oj, np.int64), np.asarray(ok, f32)
    best_kin, best_partner, keys = nearest_of((0, n, 0, n), oi, oj, kin)
    sm = cuking_amd.Submatrix(n)
    summary = ctx.kin_summary(sm, wps, ctx.upload_bitset(bits), lo=bins[0], hi=bins[1],
                              bins=bins[2])
    check_summary(summary, (histogram_of(kin, *bins), keys, best_kin, best_partner),
                  sm.NumPairs())
    import torch
    wide = cuking_amd.words_per_sample((1 << 24) + 64)
    d_wide = torch.zeros((n, wide), dtype=torch.int64, device="cuda:0")
    with pytest.raises(cuking_amd.CukingError) as e:
        ctx.kin_summary(sm, wide, d_wide)
    assert e.value.status == _lib.ERR_INVALID_ARGUMENT and "2^24" in e.value.message


@pytest.mark.parametrize("kernel,variant", [("stream", None), ("tiled", 0), ("tiled", 2)])
def test_refused_contexts(restored, kernel, variant):
    import torch
    n, m = 65, 257
    bits, _, _ = cohort(n, m)
    restored.set_kernel(kernel)
    if variant is not None:
        restored.set_option("variant", variant)
    sentinel = np.array(SENTINEL, dtype=u64).view(np.int64).item()
    hist = torch.full((1536 + 3,), sentinel, dtype=torch.int64, device="cuda:0")
    best = torch.full((n,), sentinel, dtype=torch.int64, device="cuda:0")
    for tile_range in (None, (0, 1)):
        with pytest.raises(cuking_amd.CukingError) as e:
            restored.kin_summary(cuking_amd.Submatrix(n), bits.shape[1],
                                 restored.upload_bitset(np.array(bits)), hist=hist, best=best,
                                 tile_range=tile_range)
        assert e.value.status == _lib.ERR_INVALID_ARGUMENT
        assert "variant 5, 6 or 7" in e.value.message
    torch.cuda.synchronize()
    assert (hist == sentinel).all() and (best == sentinel).all()


def test_sorted_layout(restored):
    """A cohort whose low-call-rate samples the default context sorts to the end of its
    layout: the summary still sits at the stored samples' positions, and thresholded runs on
    the same context before and after still give the oracle's records (with and without the
    reuse of a prepared layout)."""
    from oracle import pyoracle
    n, m, thr, bins = 600, 2000, 0.0884, BIN_SETS[0]
    low = tuple(range(7, 600, 50))
    assert len(low) == 12
    bits, _, _ = cohort(n, m, low_call=low)
    exp = expectation(n, m, *bins, low_call=low)
    assert restored.get_option("variant") == 7 and restored.get_option("filter_sort") == 1
    records, ovf, _ = pyoracle.compute(pyoracle.submatrix(n), np.array(bits), thr)
    assert ovf == 0 and len(records) > 0
    sm = cuking_amd.Submatrix(n)
    d_bits = restored.upload_bitset(np.array(bits))
    try:
        for reuse in (0, 1):
            restored.set_option("reuse_prepared", reuse)
            restored.invalidate()
            assert restored.run(sm, bits.shape[1], d_bits, thr).tobytes() == records.tobytes()
            summary = restored.kin_summary(sm, bits.shape[1], d_bits, lo=bins[0], hi=bins[1],
                                           bins=bins[2])
            check_summary(summary, exp, sm.NumPairs(), f"reuse_prepared {reuse}")
            assert restored.run(sm, bits.shape[1], d_bits, thr).tobytes() == records.tobytes()
    finally:
        restored.set_option("reuse_prepared", 0)
        restored.invalidate()
