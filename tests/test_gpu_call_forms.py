"""The six pair calls -- records, dense kinship matrix, relative counts, kinship summary, PI_HAT
records, counts -- one after the other on ONE context, one bitset and one stream, in that order
and in the reverse order on a fresh context.  Each result is held to what the call's own test
file holds it to (the oracle's records and sums, reducing_cases' restatement of the oracle's
kinship, the PI_HAT host twin's bytes), and the two orders give the same bytes.

What the per-call files cannot see: what one form leaves in the workspace for the next.  The
forms differ in the layout they convert (sorted or in stored order, the four-product kernel's
codes now or later, king_launch_plan.h kCallForms), and each call decides whether the layout
it finds is its own.

300 samples x 1,000 sites cut 172 | 128: partial tiles at the 128- and at the 256-sample edge,
variant 7 on the quadrants of its tiles wherever the filter does not run; the diagonal block
and the off-diagonal one, each whole and as two tile ranges that meet in the middle."""
import functools

import numpy as np
import pytest

import cuking_amd
from conftest import random_genotypes
from reducing_cases import SENTINEL, assert_same, expect_all

N, M, CUT = 300, 1000, 172
THR = 0.0442                                 # records: the third-degree cut-off
THRESHOLDS = (0.0442, 0.0884, 0.177, 0.354)  # relative counts
BINS = (-1.0, 0.5, 1536)
MIN_PI_HAT = 0.05
BLOCKS = {"diagonal": (0, CUT, 0, CUT), "off-diagonal": (0, CUT, CUT, N)}
ORDER = ("records", "matrix", "relative counts", "summary", "pi_hat", "counts")


@functools.lru_cache(maxsize=None)
def genotypes():
    geno = random_genotypes(np.random.default_rng(1000 * N + M), N, M, missing=0.07)
    geno[100] = geno[5]          # a duplicate pair inside the diagonal block ...
    geno[N - 1] = geno[3]        # ... and one across the cut
    geno.setflags(write=False)
    return geno


@functools.lru_cache(maxsize=None)
def block(name):
    """(bits of the block's stored samples, words per sample, the references of every form)."""
    from oracle import pyoracle
    sm = BLOCKS[name]
    idx = list(range(sm[0], sm[1])) + (list(range(sm[2], sm[3])) if sm[0] != sm[2] else [])
    bits = pyoracle.bitset_from_genotypes(np.ascontiguousarray(genotypes()[idx]))
    osm = pyoracle.Submatrix(*sm)
    pairs = pyoracle.all_pairs(osm, bits)
    records, overflow, _ = pyoracle.compute(osm, bits, THR)
    assert not overflow
    wps = bits.shape[1]
    every = pyoracle.bitset_from_genotypes(np.ascontiguousarray(genotypes()))
    model = cuking_amd.pi_hat_model_host(cuking_amd.pihat.site_counts_of_host_bits(every, wps), M)
    pihat = cuking_amd.pi_hat_records_host(cuking_amd.Submatrix.from_ranges(*sm), wps, bits, M,
                                           MIN_PI_HAT, model=model).records
    ref = dict(records=records, pairs=pairs, pihat=pihat, model=model,
               reduced=expect_all(sm, pairs, BINS, THRESHOLDS))
    bits.setflags(write=False)
    return bits, wps, ref


@pytest.mark.parametrize("name", BLOCKS)
def test_thresholded_forms_are_not_vacuous(name):
    """At this seed each thresholded form returns some pairs of the block and not all."""
    _, _, ref = block(name)
    num_pairs = len(ref["pairs"][0])
    assert num_pairs == (CUT * (CUT - 1) // 2 if name == "diagonal" else CUT * (N - CUT))
    assert 0 < len(ref["records"]) < num_pairs
    assert 0 < len(ref["pihat"]) < num_pairs
    listed = int(ref["reduced"].bands.sum()) // 2        # (every pair counts for two samples)
    assert listed == len(ref["records"])


def issue(ctx, form, sm, wps, d_bits, ref, ranges):
    """One form over the tile ranges `ranges` ((None,) = the whole-block entry point): its
    result checked against the reference, and returned as bytes."""
    import torch
    from test_gpu_kin_summary import check_summary
    from test_gpu_pihat import raw_call
    from test_gpu_relative_counts import check_counts
    exp = ref["reduced"]
    if form == "records":
        parts = [ctx.run(sm, wps, d_bits, THR, tile_range=r, sort=False) for r in ranges]
        got = cuking_amd.sort_results(np.ascontiguousarray(np.concatenate(parts)))
        assert got.tobytes() == ref["records"].tobytes()
        return got.tobytes()
    if form == "matrix":
        out = torch.full((sm.NumRows(), sm.NumCols()), float(SENTINEL), dtype=torch.float32,
                         device=f"cuda:{ctx.device}")
        for r in ranges:
            ctx.kin_matrix(sm, wps, d_bits, out=out, tile_range=r)
        torch.cuda.synchronize(ctx.device)
        got = out.cpu().numpy()
        assert_same(got, exp.matrix, "matrix")
        return got.tobytes()
    if form == "relative counts":
        counts = None
        for r in ranges:
            counts = ctx.relative_counts(sm, wps, d_bits, thresholds=THRESHOLDS, tile_range=r,
                                         out=None if counts is None else counts.counts)
        check_counts(counts, exp.bands, "relative counts")
        return counts.bands().tobytes()
    if form == "summary":
        summary = None
        for r in ranges:
            summary = ctx.kin_summary(sm, wps, d_bits, *BINS, tile_range=r,
                                      hist=None if summary is None else summary.hist,
                                      best=None if summary is None else summary.best)
        check_summary(summary, (exp.hist, exp.keys, exp.best_kin, exp.best_partner),
                      len(exp.pairs[0]), "summary")
        return summary.counts().tobytes() + summary.keys().tobytes()
    if form == "pi_hat":
        want = ref["pihat"]
        rows = [raw_call(ctx, sm, wps, d_bits, ref["model"], len(want), r) for r in ranges]
        assert sum(count for _, count, _, _ in rows) == len(want)
        assert not any(overflow for _, _, overflow, _ in rows)
        got = cuking_amd.sort_results(np.concatenate([r[0] for r in rows]))
        assert got.tobytes() == want.tobytes()
        return got.tobytes()
    assert form == "counts"          # (no tile-range entry point: the whole block either way)
    got = ctx.compute_counts(sm, wps, d_bits)
    oi, oj, oc, _ = ref["pairs"]
    sel = got[oi - sm.i_begin, oj - sm.j_begin]
    for field in oc.dtype.names:
        assert np.array_equal(sel[field], oc[field]), field
    return np.ascontiguousarray(sel).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [5, 6, 7])
def test_six_forms_in_sequence_both_orders(variant):
    for name in BLOCKS:
        bits, wps, ref = block(name)
        sm = cuking_amd.Submatrix.from_ranges(*BLOCKS[name])
        for split in (False, True):
            results = []
            for order in (ORDER, ORDER[::-1]):
                ctx = cuking_amd.KingContext(0)
                try:
                    ctx.set_option("variant", variant)
                    d_bits = ctx.upload_bitset(np.array(bits))
                    tiles = ctx.num_tiles(sm)
                    ranges = ((0, tiles // 2), (tiles // 2, tiles)) if split else (None,)
                    results.append({form: issue(ctx, form, sm, wps, d_bits, ref, ranges)
                                    for form in order})
                finally:
                    ctx.close()
            for form in ORDER:
                assert results[0][form] == results[1][form], (name, split, form)
