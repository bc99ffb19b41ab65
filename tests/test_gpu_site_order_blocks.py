"""The site order of the filter path ("filter_site_order", king_abi.hip prepare()) held to the
oracle wherever prepare() takes another turn: every block of a split (off-diagonal blocks
store rows + columns, their statistics are a launch of their own on the ordered copy, the
plane layout pads between rows and columns), the counting forms of relative_counts, the second
conversion of the codes behind an ordered T2, the sample sort and remainder pieces on an
ordered layout, reuse across thresholds, layouts taken over by kin_matrix and by a staged
pass, a conversion on another stream, bitsets beyond G = 4 and beyond the gather, and curves
whose weights are all zero.

Expectations are the oracle's (pyoracle.compute for records, pyoracle.all_pairs through
reducing_cases.expect_all for counts and the matrix), and order 1 is compared with order 0
byte for byte besides.  A call that is expected to run on an ordered layout must say so
("site_order_on"): falling back to stored order is a failure here, not a pass."""
import itertools

import numpy as np
import pytest

import cuking_amd
import reducing_cases as rc
from cuking_amd.dist import tile_partition
from conftest import random_genotypes
from test_gpu_site_gather import COUNTERS
from test_gpu_site_order import plant, prepare_ctx

pytestmark = pytest.mark.gpu

THR = 0.0884
# the shipped value of everything a test here sets
RESTORE = (("filter_site_order", -1), ("filter_site_order_min_tiles", 24576),
           ("filter_site_gather", -1), ("filter_check_min_steps", 64),
           ("filter_rotate_min_steps", 128), ("filter_rotate_min_tiles", 2048),
           ("filter_sort", 1), ("filter_lazy_codes", 1), ("filter_quadrant_cap", 384),
           ("filter_cand_cap", 1 << 25), ("split_wgs", 256), ("counts_mode", -1),
           ("reuse_prepared", 0))
BINS = (-1.0, 0.5, 1536)               # (expect_all wants bins; no test here reads the histogram)
SPLITS = [(600, 2, s) for s in range(3)] + [(700, 3, s) for s in range(6)]
CAPS = ((384, 1 << 20), (0, 0), (2, 5))           # as shipped / everything dense / tiny
THRESHOLD_SETS = ((0.0442, 0.0884, 0.177, 0.354), (0.0884,))


def set_up(ctx):
    prepare_ctx(ctx)
    ctx.set_option("filter_site_order_min_tiles", 0)


def restore(ctx):
    for k, v in RESTORE:
        ctx.set_option(k, v)
    ctx.invalidate()


def cohort(rng, n, m, split=1, missing=0.01, af_lo=0.05, af_hi=0.5):
    """Spread allele frequencies, 1 % missing, the three planted relatives, and a
    parent-child-like pair inside every block of the split that holds none of the three."""
    geno = random_genotypes(rng, n, m, missing=missing, af_lo=af_lo, af_hi=af_hi)
    if n < 8:                      # (no room for the three: a sibling-like pair)
        geno[n - 1, ::2] = geno[0, ::2]
        return geno
    plant(geno)
    taken = {n - 1, 3, n // 2, 5, n - 7, 260 % n}
    half = m // 2
    for shard in range(split * (split + 1) // 2 if split > 1 else 0):
        i0, i1, j0, j1 = cuking_amd.Submatrix(n, split, shard).as_tuple()
        src, dst = i0 + 37, (i0 if i0 == j0 else j0) + 41 + 3 * (i0 // max(i1 - i0, 1))
        assert i0 <= src < i1 and j0 <= dst < j1 and not {src, dst} & taken, (shard, src, dst)
        taken.add(dst)
        geno[dst, :half] = geno[src, :half]
    return geno


class Block:
    """One block of a cohort: its bitset (rows, then columns), the oracle's view of it."""

    def __init__(self, oracle, geno, split=1, shard=0):
        n, self.sites = geno.shape
        self.sm = cuking_amd.Submatrix(n, split, shard)
        self.osm = oracle.submatrix(n, split, shard)
        assert self.osm.as_tuple() == self.sm.as_tuple()
        self.bits = oracle.bitset_from_genotypes(geno, self.osm)
        self.wps = self.bits.shape[1]
        self.oracle = oracle
        self._records, self._all = {}, None

    def records(self, thr=THR):
        if thr not in self._records:
            self._records[thr] = self.oracle.compute(self.osm, self.bits, thr, threads=16)[0]
        return self._records[thr]

    def expect(self, thresholds):
        if self._all is None:
            self._all = self.oracle.all_pairs(self.osm, self.bits)
        return rc.expect_all(self.sm.as_tuple(), self._all, BINS, thresholds)


@pytest.fixture(scope="module")
def material(oracle):
    """Cohorts, blocks and the oracle's records, computed once."""
    rng = np.random.default_rng(2301)
    out = {}
    for n, split in ((600, 2), (700, 3)):
        geno = cohort(rng, n, 3000, split)
        for shard in range(split * (split + 1) // 2):
            b = out[(n, split, shard)] = Block(oracle, geno, split, shard)
            assert len(b.records()) >= 1, (n, split, shard)
        if n == 600:
            out["600"], out["600 off"] = Block(oracle, geno), out[(600, 2, 1)]
    geno = cohort(rng, 1100, 20480, 2)
    out["1100"], out["1100 off"] = Block(oracle, geno), Block(oracle, geno, 2, 1)
    # every site weighs the same, 3 % missing: nothing to sort, the automatic rule says no
    # (test_gpu_site_order.py test_device_curve_share_and_automatic_rule_match_numpy)
    flat = np.random.default_rng(1812)
    out["1100 flat"] = Block(oracle, cohort(flat, 1100, 20480, missing=0.03, af_lo=0.5, af_hi=0.5))
    for name in ("1100", "1100 off", "1100 flat"):
        assert len(out[name].records()) >= 2, name
    return out


def run(ctx, b, d_bits, thr=THR, **kw):
    return ctx.run(b.sm, b.wps, d_bits, thr, max_results=1 << 20, **kw)


# ---- (a) every block of a split -------------------------------------------------------------
@pytest.mark.parametrize("n,split,shard", SPLITS)
def test_every_block_of_a_split(ctx, material, n, split, shard):
    """600 samples in two parts and 700 in three, x 3,000 sites (12 k-steps, the last word
    padded): no part is a multiple of 64 samples, so an off-diagonal block's plane
    layout pads between rows and columns where the stored bitset does not.  Orders 0 / 1 / 2
    by gathers -1 / 0 / 2 / 4."""
    b = material[(n, split, shard)]
    exp = b.records()
    d_bits = ctx.upload_bitset(b.bits)
    set_up(ctx)
    try:
        got = {}
        for order in (0, 1, 2):
            ctx.set_option("filter_site_order", order)
            moved = {}
            for gather in (-1, 0, 2, 4):
                ctx.set_option("filter_site_gather", gather)
                before = [ctx.get_option(c) for c in COUNTERS]
                got[order, gather] = run(ctx, b, d_bits)
                moved[gather] = [ctx.get_option(c) - x for c, x in zip(COUNTERS, before)]
                assert ctx.get_option("site_order_on") == int(order != 0), (order, gather)
                assert got[order, gather].tobytes() == exp.tobytes(), (order, gather)
            assert moved[-1] == moved[0] == moved[2] == moved[4], (order, moved)
        for gather in (-1, 0, 2, 4):
            assert got[1, gather].tobytes() == got[0, gather].tobytes(), gather
    finally:
        restore(ctx)


# ---- (b) forms and options ------------------------------------------------------------------
def options_grid(ctx, b, modes):
    """Order 1 over counts_mode x filter_sort x lazy codes x caps x split_wgs: records equal
    the oracle everywhere; tiles leave at the check wherever the lean form runs whole tiles
    with the shipped caps; the full form keeps stored order."""
    exp = b.records()
    d_bits = ctx.upload_bitset(b.bits)
    set_up(ctx)
    try:
        ctx.set_option("filter_site_order", 1)
        for mode, sort, lazy, (qcap, ccap), wgs in itertools.product(
                modes, (0, 1, 2), (0, 1), CAPS, (0, 256)):
            point = dict(counts_mode=mode, filter_sort=sort, filter_lazy_codes=lazy,
                         filter_quadrant_cap=qcap, filter_cand_cap=ccap, split_wgs=wgs)
            for k, v in point.items():
                ctx.set_option(k, v)
            exits = ctx.get_option("filter_early_exits")
            got = run(ctx, b, d_bits)
            exits = ctx.get_option("filter_early_exits") - exits
            assert got.tobytes() == exp.tobytes(), point
            # (-1: the automatic rule picks the lean form at 20,480 sites and this threshold)
            assert ctx.get_option("site_order_on") == int(mode != 1), point
            if mode == 0 and wgs == 0 and (qcap, ccap) == CAPS[0]:
                assert exits > 0, point
    finally:
        restore(ctx)


@pytest.mark.parametrize("mode", [0, -1, 1])
def test_forms_and_options_on_the_diagonal_block(ctx, material, mode):
    """1,100 x 20,480, 80 k-steps: tiles leave at the check.  Lazy codes off, or caps that
    send quadrants to the four-product kernel, convert the codes a second time from the
    stored bitset behind the ordered T2."""
    options_grid(ctx, material["1100"], (mode,))


def test_forms_and_options_on_an_off_diagonal_block(ctx, material):
    """The same grid, lean form, on the 550 x 550 block Submatrix(1100, 2, 1)."""
    options_grid(ctx, material["1100 off"], (0,))


# ---- (c) relative_counts with the order on ---------------------------------------------------
@pytest.mark.parametrize("thresholds", THRESHOLD_SETS)
@pytest.mark.parametrize("name", ["600", "600 off"])
def test_relative_counts_on_an_ordered_layout(ctx, material, name, thresholds):
    """The counting forms convert with the order on (kin_threshold = thresholds[0])."""
    import torch
    b = material[name]
    exp = b.expect(thresholds)
    above = len(b.records(thresholds[0]))
    stored = b.sm.NumSamples()
    assert exp.bands.shape == (stored, len(thresholds)) and above >= 1
    d_bits = ctx.upload_bitset(b.bits)
    set_up(ctx)
    try:
        ctx.set_option("filter_site_order", 1)
        out = torch.zeros((stored, len(thresholds)), dtype=torch.int32, device=d_bits.device)
        for times in (1, 2):           # the call accumulates: a second one doubles the counts
            counts = ctx.relative_counts(b.sm, b.wps, d_bits, thresholds=thresholds, out=out)
            assert np.array_equal(counts.bands(), np.uint32(times) * exp.bands), times
            assert ctx.get_option("site_order_on") == 1
            assert counts.num_records(0) == times * above
        tiles = ctx.num_tiles(b.sm)
        assert tiles >= 3
        out = torch.zeros_like(out)
        for r in tile_partition(tiles, 3):
            counts = ctx.relative_counts(b.sm, b.wps, d_bits, thresholds=thresholds, out=out,
                                         tile_range=r)
            assert ctx.get_option("site_order_on") == 1, r
        assert np.array_equal(counts.bands(), exp.bands)
        assert counts.num_records(0) == above
    finally:
        restore(ctx)


# ---- (d) reuse and take-overs ---------------------------------------------------------------
def test_reuse_converts_again_at_another_threshold(ctx, material):
    """reuse_prepared = 1: an ordered layout's share comes from its curve at the threshold of
    the call that converted it, so a call at another threshold converts afresh; a repeat
    reuses."""
    b = material["1100"]
    d_bits = ctx.upload_bitset(b.bits)
    set_up(ctx)
    try:
        ctx.set_option("filter_site_order", 1)
        ctx.set_option("reuse_prepared", 1)
        ctx.invalidate()
        for thr, moves in ((0.0884, 0), (0.177, 0), (0.0884, 0), (0.0884, 1)):
            skipped = ctx.get_option("conversions_skipped")
            got = run(ctx, b, d_bits, thr)
            assert got.tobytes() == b.records(thr).tobytes(), (thr, moves)
            assert ctx.get_option("conversions_skipped") - skipped == moves, (thr, moves)
            assert ctx.get_option("site_order_on") == 1
        assert len(b.records(0.177)) >= 1
    finally:
        restore(ctx)


def test_an_automatic_no_is_trusted_at_its_own_threshold_only(ctx, material):
    """The flat cohort: the automatic rule says no at 0.0884 and remembers it for the block's
    next conversions (reuse_prepared = 0: each call converts).  A call at 0.177 builds a curve
    of its own -- one wait of the host -- and does not inherit the "no".  With reuse_prepared
    = 1 a stored-order layout serves any threshold: it is reused, nothing is built."""
    b = material["1100 flat"]
    d_bits = ctx.upload_bitset(b.bits)
    set_up(ctx)
    try:
        ctx.set_option("filter_site_order", -1)
        assert run(ctx, b, d_bits, 0.0884).tobytes() == b.records(0.0884).tobytes()
        assert ctx.get_option("site_order_on") == 0          # the rule said no
        syncs = ctx.get_option("host_syncs")
        assert run(ctx, b, d_bits, 0.0884).tobytes() == b.records(0.0884).tobytes()
        assert ctx.get_option("host_syncs") - syncs == 0     # remembered
        assert run(ctx, b, d_bits, 0.177).tobytes() == b.records(0.177).tobytes()
        assert ctx.get_option("host_syncs") - syncs == 1     # a curve of its own
        assert len(b.records(0.177)) >= 1
        ctx.set_option("reuse_prepared", 1)
        ctx.invalidate()
        for thr, moves in ((0.0884, 0), (0.177, 1)):
            skipped = ctx.get_option("conversions_skipped")
            assert run(ctx, b, d_bits, thr).tobytes() == b.records(thr).tobytes(), thr
            assert ctx.get_option("conversions_skipped") - skipped == moves, thr
            assert ctx.get_option("site_order_on") == 0
    finally:
        restore(ctx)


@pytest.mark.parametrize("name", ["1100", "1100 off"])
def test_kin_matrix_takes_an_ordered_layout_over_and_gives_it_back(ctx, material, name):
    import torch
    b = material[name]
    exp = b.expect((THR,))
    d_bits = ctx.upload_bitset(b.bits)
    set_up(ctx)
    try:
        ctx.set_option("filter_site_order", 1)
        ctx.set_option("reuse_prepared", 1)
        ctx.invalidate()
        assert run(ctx, b, d_bits).tobytes() == b.records().tobytes()
        assert ctx.get_option("site_order_on") == 1
        out = torch.full(exp.matrix.shape, float(rc.SENTINEL), dtype=torch.float32,
                         device=d_bits.device)
        ctx.kin_matrix(b.sm, b.wps, d_bits, out=out)
        torch.cuda.synchronize()
        rc.assert_same(out.cpu().numpy(), exp.matrix, "kin_matrix behind an ordered layout")
        assert ctx.get_option("site_order_on") == 0
        assert run(ctx, b, d_bits).tobytes() == b.records().tobytes()
        assert ctx.get_option("site_order_on") == 1
    finally:
        restore(ctx)


def test_a_staged_pass_takes_an_ordered_layout_over_and_gives_it_back(ctx, material):
    """The ranges of cuking_prepare_samples keep stored order: world 3, 4 chunks."""
    import fuzz_cases
    b = material["1100"]
    exp = b.records()
    n = b.bits.shape[0]
    d_bits = ctx.upload_bitset(b.bits)
    set_up(ctx)
    try:
        ctx.set_option("filter_site_order", 1)
        ctx.set_option("reuse_prepared", 1)
        ctx.invalidate()
        assert run(ctx, b, d_bits).tobytes() == exp.tobytes()
        assert ctx.get_option("site_order_on") == 1
        staged = fuzz_cases._staged(ctx, b.sm, b.wps, d_bits, THR, len(exp) + 8, n, 3, 4, [1, 2, 3])
        assert staged.tobytes() == exp.tobytes()
        assert ctx.get_option("site_order_on") == 0
        assert run(ctx, b, d_bits).tobytes() == exp.tobytes()
        assert ctx.get_option("site_order_on") == 1
    finally:
        restore(ctx)


def test_converted_on_one_stream_and_launched_on_another(ctx, material):
    """The ordered copy lives in the converting stream's scratch entry, the layout in the
    context: a call on the current stream reuses what a side stream converted."""
    import torch
    b = material["1100"]
    exp = b.records()
    d_bits = ctx.upload_bitset(b.bits)
    set_up(ctx)
    try:
        ctx.set_option("filter_site_order", 1)
        ctx.set_option("reuse_prepared", 1)
        ctx.invalidate()
        side = torch.cuda.Stream(d_bits.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            first = run(ctx, b, d_bits)
        assert ctx.get_option("site_order_on") == 1
        skipped = ctx.get_option("conversions_skipped")
        again = run(ctx, b, d_bits)
        assert ctx.get_option("conversions_skipped") == skipped + 1
        assert ctx.get_option("site_order_on") == 1
        assert again.tobytes() == first.tobytes() == exp.tobytes()
    finally:
        restore(ctx)


# ---- (e) widths -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide(oracle):
    """200 samples x 163,840 sites (2,560 plane words: beyond 4 samples a byte per site in
    LDS) and x 270,336 sites (4,224 plane words: beyond the gather altogether)."""
    rng = np.random.default_rng(2302)
    out = {}
    for m in (163840, 270336):
        b = out[m] = Block(oracle, cohort(rng, 200, m))
        assert b.wps == 2 * (m // 64) and len(b.records()) >= 3
    return out


def test_bitsets_too_wide_for_four_samples_take_two(ctx, wide):
    b = wide[163840]
    d_bits = ctx.upload_bitset(b.bits)
    set_up(ctx)
    try:
        ctx.set_option("filter_site_order", 1)
        assert run(ctx, b, d_bits).tobytes() == b.records().tobytes()
        assert ctx.get_option("site_order_on") == 1
        ctx.set_option("filter_site_gather", 4)
        with pytest.raises(cuking_amd.CukingError,
                           match="filter_site_gather 4: 5120 words per sample do not fit") as e:
            run(ctx, b, d_bits)
        assert e.value.status == 1                           # CUKING_ERR_INVALID_ARGUMENT
        ctx.set_option("filter_site_gather", -1)
        assert run(ctx, b, d_bits).tobytes() == b.records().tobytes()
        assert ctx.get_option("site_order_on") == 1
        ctx.set_option("filter_site_order", 0)
        assert run(ctx, b, d_bits).tobytes() == b.records().tobytes()
    finally:
        restore(ctx)


def test_bitsets_too_wide_for_the_gather_keep_stored_order(ctx, wide):
    b = wide[270336]
    d_bits = ctx.upload_bitset(b.bits)
    set_up(ctx)
    try:
        ctx.set_option("filter_site_order", 1)
        assert run(ctx, b, d_bits).tobytes() == b.records().tobytes()
        assert ctx.get_option("site_order_on") == 0
    finally:
        restore(ctx)


# ---- (f) degenerate curves ------------------------------------------------------------------
def degenerate_cases():
    rng = np.random.default_rng(2303)
    out = {"2x3000": cohort(rng, 2, 3000)}
    for m in (1, 255, 257):
        out[f"300x{m}"] = cohort(rng, 300, m)
    # hom-ref or missing everywhere: every weight is zero, so is the curve's total
    g = cohort(rng, 600, 3000)
    out["600x3000 monomorphic"] = np.where(g < 0, -1, 0).astype(np.int8)
    g = cohort(rng, 600, 3000)
    g[1] = g[2] = -1
    g[3] = np.where(g[3] == 1, 0, g[3])
    out["600x3000 all-missing samples"] = g
    return out


DEGENERATE = ("2x3000", "300x1", "300x255", "300x257", "600x3000 monomorphic",
              "600x3000 all-missing samples")


@pytest.fixture(scope="module")
def degenerate(oracle):
    return {name: Block(oracle, geno) for name, geno in degenerate_cases().items()}


@pytest.mark.parametrize("name", DEGENERATE)
def test_degenerate_curves(ctx, degenerate, name):
    """Records -- possibly none -- equal the oracle's and stored order's, and no error.  Two
    stored samples is all the order asks for: the layout is ordered in every case."""
    b = degenerate[name]
    exp = b.records()
    d_bits = ctx.upload_bitset(b.bits)
    set_up(ctx)
    try:
        got = {}
        for order in (0, 1):
            ctx.set_option("filter_site_order", order)
            got[order] = run(ctx, b, d_bits)
            assert ctx.get_option("site_order_on") == order, order
        assert got[1].tobytes() == got[0].tobytes()
        assert got[1].tobytes() == exp.tobytes()
    finally:
        restore(ctx)
