"""Seeded random GPU-vs-oracle sweeps, shared by `pytest -m gpu`
(tests/test_gpu_fuzz.py) and the command-line fuzzers (tools/fuzz_gpu.py,
tools/fuzz_reducing.py, tools/fuzz_split.py, tools/stress_split.py) that run the
same cases in bulk.

Every failure is reported as a reproducer: the generator function, its seed and
the index of the case, plus the case's parameters -- `python tools/fuzz_gpu.py
SEED CASES FIRST_CASE` replays it (run_reducing: `python tools/fuzz_reducing.py
SEED CASES FIRST_CASE [SIZE_CLASS]`, the size class being the tag's `sweep`; run_pipeline:
`python tools/fuzz_pipeline.py SEED CASES --first-case K --size-class CLASS`; run_site_order:
`python tools/fuzz_site_order.py SEED CASES FIRST_CASE`; run_pcrelate, whose checkers are the
float64 references of tests/pcrelate_cases.py and tests/pcrelate_pairs_cases.py and the host
twins: `python tools/fuzz_pcrelate.py SEED CASES FIRST_CASE SIZE_CLASS`; run_pihat, whose checker
besides the oracle is the numpy restatement of tests/pihat_cases.py: `python tools/fuzz_pihat.py
SEED CASES FIRST_CASE SIZE_CLASS`).
The checker is the CPU oracle (oracle/pyoracle.py); everything checked goes
through the C ABI."""
from __future__ import annotations

import itertools
import time

import numpy as np


class FuzzMismatch(AssertionError):
    pass


def _records(res, cnt):
    import cuking_amd
    return res[:cnt].cpu().numpy().view(np.uint32).reshape(-1).view(
        cuking_amd.KING_RESULT_DTYPE).copy()


def _staged(ctx, sm, wps, d_bits, thr, cap, n, world, chunks, streams):
    """Every rank's staged schedule replayed on this GPU; the ranks' records."""
    import cuking_amd
    from cuking_amd.dist import GpuStagedOps, staged_schedule
    parts = []
    for rank in range(world):
        ops = GpuStagedOps(ctx, sm, wps, d_bits, thr, cap, num_streams=streams[rank])
        ops.begin()
        for (c0, c1), rect in staged_schedule(n, ctx.tile_samples(), world, rank, chunks):
            if rect is None:
                continue
            ops.prepare(c0, c1)
            ops.compute_rect(*rect)
        res, cnt, ovf = ops.finish()
        if ovf:
            raise FuzzMismatch("staged overflow")
        parts.append(_records(res, cnt))
    return cuking_amd.sort_results(np.ascontiguousarray(np.concatenate(parts)))


def _diff(got, exp):
    have = {(int(r["sample_i"]), int(r["sample_j"])) for r in got}
    want = {(int(r["sample_i"]), int(r["sample_j"])) for r in exp}
    return (f"records {len(got)} vs {len(exp)}, missing {sorted(want - have)[:6]}, "
            f"extra {sorted(have - want)[:6]}")


def run_general(ctx, seed: int, cases: int, first_case: int = 0, log=None) -> int:
    """Shapes, shards, kernel variants, lean/full forms, thresholds, tile ranges
    and staged schedules (tools/fuzz_gpu.py).  Returns the number of cases run."""
    import torch
    import cuking_amd
    from cuking_amd.dist import tile_partition
    from conftest import random_genotypes
    from oracle import pyoracle

    rng = np.random.default_rng(seed)
    num_variants = ctx.lib.cuking_num_variants()
    t0, ran = time.time(), 0
    for case in range(cases):
        n = int(rng.integers(2, 700))
        m = int(rng.integers(1, 2500))
        if rng.random() < 0.15:   # enough tiles for the XCD-aware order (launches of >= 64 tiles)
            n = int(rng.integers(1400, 2300))
        big = False
        if n < 1400 and rng.random() < 0.01:
            # the filter variant's give-up decision: more tiles than CUs (> 23 x 23 tiles of
            # 256 samples) and a threshold inside the noise of so few sites, so that most
            # quadrants of the first round go dense and the later tiles hand theirs over
            n, m, big = int(rng.integers(5900, 6600)), int(rng.integers(100, 200)), True
        k = int(rng.integers(1, 4))
        shard = int(rng.integers(0, k * (k + 1) // 2))
        thr = float(rng.choice([-1e30, -0.2, 0.0, 0.03, 0.0884, 0.3]))
        variant = int(rng.integers(0, num_variants))
        mode = int(rng.integers(-1, 2))
        if big:
            # (the whole triangle; every pair of 6,000 samples would not fit the default
            #  --max_results: a threshold about one sigma out; that variant, lean form, in
            #  three of four cases)
            k, shard, thr = 1, 0, 0.0884
            if rng.random() < 0.75 and num_variants > 7:
                variant, mode = 7, 0
        kernel = "stream" if rng.random() < 0.15 else "tiled"
        missing = float(rng.choice([0.0, 0.02, 0.3]))
        geno = random_genotypes(rng, n, m, missing=missing)
        if n > 3:
            geno[n - 1] = geno[0]
            if rng.random() < 0.3:
                geno[1] = -1
            if rng.random() < 0.3:       # a few low-call-rate samples (the sorted layout's case)
                who = rng.choice(n, size=max(1, n // 16), replace=False)
                geno[who] = np.where(rng.random((len(who), m)) < 0.4, -1, geno[who])
        swizzle = int(rng.integers(0, 3))
        band = int(rng.choice([0, 0, 1, 3, 5, 17]))
        wgs = int(rng.choice([0, 256, 256]))
        reuse = int(rng.integers(0, 2))
        w = int(rng.integers(2, 5))
        world = int(rng.integers(1, 9))
        chunks = int(rng.integers(1, 9))
        streams = [int(rng.integers(1, 4)) for _ in range(world)]
        # filter variant: who computes a pair exactly (candidate list / dense quadrants)
        qcap = int(rng.choice([384, 384, 0, 2]))
        ccap = int(rng.choice([1 << 20, 1 << 20, 0, 5]))
        smin = int(rng.choice([8, 1, 1]))      # remainder pieces of k even for short bitsets
        # ... and its check points inside the k loop (forecast: off / short launches / always;
        # rigorous: off / automatic / an entry of the share menu), for bitsets of >= 4 k-steps
        chk0 = int(rng.choice([1, 0, 2, 2]))
        chk1 = int(rng.choice([1, 0, 3, 5, 7, 9]))
        srt, lazy = int(rng.integers(0, 3)), int(rng.integers(0, 2))   # sorted layout, lazy codes
        emit = int(rng.choice([64, 64, 0, 1, 255]))    # live pairs a tile hands over at the check
        # rotated tiles: as shipped (joins the XCD's position) / off / a phase per tile / one phase
        rot = int(rng.choice([1, 0, 2, 2, 3 + int(rng.integers(0, 64))]))
        rng.integers(0, 2)                   # (was the persistent launch: a seed still names the same cases)
        if case < first_case:
            continue
        tag = dict(fuzzer="run_general", seed=seed, case=case, n=n, m=m, split_factor=k,
                   shard=shard, thr=thr, kernel=kernel, variant=variant, counts_mode=mode,
                   xcd_swizzle=swizzle, band_rows=band, split_wgs=wgs, reuse_prepared=reuse,
                   filter_quadrant_cap=qcap, filter_cand_cap=ccap, filter_split_min_steps=smin,
                   filter_check0=chk0, filter_check1=chk1, filter_check_min_steps=4,
                   filter_sort=srt, filter_lazy_codes=lazy, filter_check_emit=emit,
                   filter_rotate=rot, filter_rotate_min_steps=4)
        osm = pyoracle.submatrix(n, k, shard)
        bits = pyoracle.bitset_from_genotypes(geno, osm)
        exp, _, _ = pyoracle.compute(osm, bits, thr, threads=8)
        sm = cuking_amd.Submatrix(n, k, shard)
        ctx.set_kernel(kernel)
        ctx.set_option("variant", variant)
        ctx.set_option("counts_mode", mode)
        ctx.set_option("xcd_swizzle", swizzle)
        ctx.set_option("band_rows", band)
        ctx.set_option("split_wgs", wgs)
        ctx.set_option("filter_quadrant_cap", qcap)
        ctx.set_option("filter_cand_cap", ccap)
        ctx.set_option("filter_split_min_steps", smin)
        ctx.set_option("filter_check0", chk0)
        ctx.set_option("filter_check1", chk1)
        ctx.set_option("filter_check_emit", emit)
        ctx.set_option("filter_rotate", rot)
        ctx.set_option("filter_rotate_min_steps", 4)
        ctx.set_option("filter_rotate_min_tiles", 0)
        ctx.set_option("filter_check_min_steps", 4)
        ctx.set_option("filter_sort", srt)
        ctx.set_option("filter_lazy_codes", lazy)
        # (a new bitset may land on a recycled pointer: tell the library)
        ctx.set_option("reuse_prepared", reuse)
        ctx.invalidate()
        d_bits = (ctx.upload_bitset(bits) if bits.shape[0] else
                  torch.zeros(2, dtype=torch.int64, device=f"cuda:{ctx.device}"))
        wps = cuking_amd.words_per_sample(m)
        for rep in range(2 if reuse else 1):     # the second call reuses the layout
            got = ctx.run(sm, wps, d_bits, thr)
            if got.tobytes() != exp.tobytes():
                raise FuzzMismatch(f"run (rep {rep}): {_diff(got, exp)}; reproduce with {tag}")
        if kernel == "tiled" and bits.shape[0]:
            tiles = ctx.num_tiles(sm)
            if tiles >= 2:
                parts = [ctx.run(sm, wps, d_bits, thr, tile_range=r)
                         for r in tile_partition(tiles, w)]
                merged = cuking_amd.sort_results(np.ascontiguousarray(np.concatenate(parts)))
                if merged.tobytes() != exp.tobytes():
                    raise FuzzMismatch(f"tile ranges ({w}): {_diff(merged, exp)}; reproduce with {tag}")
            if k == 1 and n >= 2:
                ctx.invalidate()
                merged = _staged(ctx, sm, wps, d_bits, thr, max(len(exp), 1) + 8, n, world, chunks,
                                 streams)
                if merged.tobytes() != exp.tobytes():
                    raise FuzzMismatch(f"staged (world {world}, chunks {chunks}, streams {streams}): "
                                       f"{_diff(merged, exp)}; reproduce with {tag}")
        ran += 1
        if log and case % 25 == 0:
            log(f"run_general seed {seed} case {case} ok ({time.time() - t0:.0f}s)")
    ctx.set_option("reuse_prepared", 0)
    ctx.set_option("filter_quadrant_cap", 384)
    ctx.set_option("filter_cand_cap", 1 << 25)
    ctx.set_option("filter_split_min_steps", 8)
    ctx.set_option("filter_check0", 1)
    ctx.set_option("filter_check1", 1)
    ctx.set_option("filter_check_emit", 64)
    ctx.set_option("filter_rotate", 1)
    ctx.set_option("filter_rotate_min_steps", 128)
    ctx.set_option("filter_rotate_min_tiles", 2048)
    ctx.set_option("filter_check_min_steps", 64)
    ctx.set_option("filter_sort", 1)
    ctx.set_option("filter_lazy_codes", 1)
    return ran


# ---- the reducing calls: kin_matrix, kin_summary, relative_counts ---------------------------
NUM_TILED_VARIANTS = 8            # (tests/test_gpu_kin_matrix.py test_variant_count pins it)
STREAM_KERNEL = NUM_TILED_VARIANTS            # the matrix "variant" that stands for the stream kernel
REDUCING_VARIANTS = (5, 6, 7)     # the only contexts kin_summary and relative_counts are served by
SIZE_CLASSES = ("small", "tiles", "giveup")
# (lo, hi, bins): the shipped default, a coarse one whose ends cut into the data, one bin,
# hi above 0.5 (duplicates inside the bins), a power of two
BIN_MENU = [(-1.0, 0.5, 1536), (-0.25, 0.25, 7), (-0.125, 0.375, 1), (0.0, 0.5001, 4096),
            (-0.5, 0.5, 64)]
# ascending; 0.5 is the kinship of the planted duplicate, 0.0 one that random pairs hit: the
# strict `>` decides.  0.001 (class "small" only) sits inside the noise of unrelated pairs:
# the filter variant gives up at once and the gated fallback computes the block
THRESHOLD_MENU = [-0.5, 0.0, 0.0442, 0.0884, 0.177, 0.354, 0.45, 0.5]
CALLS = ("run", "kin_matrix", "kin_summary", "relative_counts")
# the shipped values of everything a case sets
SHIPPED = dict(variant=7, counts_mode=-1, xcd_swizzle=2, band_rows=0, split_wgs=256,
               dyn_tail_tiles=16384, max_launch_blocks=0, reuse_prepared=0,
               filter_quadrant_cap=384, filter_cand_cap=1 << 25, filter_split_min_steps=8,
               filter_check0=1, filter_check1=1, filter_check_emit=64, filter_rotate=1,
               filter_rotate_min_steps=128, filter_rotate_min_tiles=2048,
               filter_check_min_steps=64, filter_sort=1, filter_lazy_codes=1)


def reducing_cases(seed: int, cases: int, first_case: int = 0, size_class=None):
    """The cases of run_reducing, without a context: yields (tag, geno) -- the reproducer (every
    parameter of the case) and the cohort's int8 [n, m] genotypes.  Every random number of a
    case is drawn before the `first_case` skip: a seed names the same cases whatever is
    skipped."""
    from conftest import random_genotypes
    if size_class is not None and size_class not in SIZE_CLASSES:
        raise ValueError(f"size_class {size_class!r}: one of {SIZE_CLASSES} or None")
    rng = np.random.default_rng(seed)
    for case in range(cases):
        n = int(rng.integers(2, 700))
        m = int(rng.integers(1, 2500))
        cls = "small"
        if rng.random() < 0.15:   # enough tiles for the XCD-aware order (launches of >= 64 tiles)
            cls = "tiles"
        if rng.random() < 0.01 and cls == "small":
            cls = "giveup"
        cls = size_class or cls
        n_tiles = int(rng.integers(1400, 2300))
        # the filter variant's give-up decision: more tiles than CUs (> 23 x 23 tiles of 256
        # samples) and a lowest threshold inside the noise of so few sites (run_general)
        n_big, m_big = int(rng.integers(5900, 6600)), int(rng.integers(100, 200))
        # enough k-steps for remainder pieces of the matrix-core kernels' k loop
        pieces = rng.random() < 0.25
        m_long = int(rng.integers(8000, 30000))
        wgs = int(rng.choice([0, 256, 256]))
        wgs_long = int(rng.choice([3, 6, 16]))
        k = int(rng.integers(1, 4))
        shard = int(rng.integers(0, k * (k + 1) // 2))
        matrix_variant = int(rng.integers(0, NUM_TILED_VARIANTS + 1))
        variant = int(rng.choice(REDUCING_VARIANTS))
        filter_mostly = rng.random() < 0.75
        mode = int(rng.integers(-1, 2))
        if cls == "tiles":
            n = n_tiles
        elif cls == "giveup":
            n, m, k, shard = n_big, m_big, 1, 0
            if filter_mostly:
                variant = 7
        elif pieces:
            m, wgs = m_long, wgs_long
        missing = float(rng.choice([0.0, 0.02, 0.3]))
        geno = random_genotypes(rng, n, m, missing=missing)
        low_call = rng.random() < 0.3
        who = rng.choice(n, size=max(1, n // 16), replace=False)
        thin = rng.random((len(who), m)) < 0.4
        if low_call:                 # a few low-call-rate samples (the sorted layout's case)
            geno[who] = np.where(thin, -1, geno[who])
        if n >= 5:
            geno[1] = -1             # nothing defined: NaN with everybody
            geno[2] = 0              # no het site: -inf
        if n > 3:
            geno[n - 1] = geno[0]    # a duplicate pair: 0.5
        swizzle = int(rng.integers(0, 3))
        band = int(rng.choice([0, 0, 1, 3, 5, 17]))
        reuse = int(rng.integers(0, 2))
        w = int(rng.integers(2, 6))
        qcap = int(rng.choice([384, 384, 0, 2]))
        ccap = int(rng.choice([1 << 20, 1 << 20, 0, 5]))
        smin = int(rng.choice([8, 1, 1]))
        chk0 = int(rng.choice([1, 0, 2, 2]))
        chk1 = int(rng.choice([1, 0, 3, 5, 7, 9]))
        srt, lazy = int(rng.integers(0, 3)), int(rng.integers(0, 2))
        emit = int(rng.choice([64, 64, 0, 1, 255]))
        rot = int(rng.choice([1, 0, 2, 2, 3 + int(rng.integers(0, 64))]))
        dyn = int(rng.integers(0, 2))
        blocks = int(rng.choice([0, 0, 3, 17]))
        bins = BIN_MENU[int(rng.integers(0, len(BIN_MENU)))]
        menu = list(THRESHOLD_MENU)
        if cls == "small":
            menu = sorted(menu + [0.001])
        if cls == "giveup":          # (about one sigma out; every pair of 6,000 samples would
            menu = [t for t in menu if t > 0.0884]    # not fit the record call's --max_results)
        count = int(rng.integers(1, 9))
        picked = rng.permutation(len(menu))[:min(count, len(menu))]
        thresholds = sorted(menu[int(p)] for p in picked)
        if cls == "giveup":
            thresholds = [0.0884] + thresholds[:7]
        symmetric = bool(rng.integers(0, 2))
        pad = int(rng.choice([0, 1, 37]))
        side_stream = bool(rng.random() < 0.3)
        order = [CALLS[int(c)] for c in rng.permutation(len(CALLS))]
        if case < first_case:
            continue
        tag = dict(fuzzer="run_reducing", seed=seed, case=case, sweep=size_class or "mixed",
                   size_class=cls, n=n, m=m,
                   split_factor=k, shard=shard, missing=missing, low_call=bool(low_call),
                   matrix_variant="stream" if matrix_variant == STREAM_KERNEL else matrix_variant,
                   variant=variant, counts_mode=mode, bins=bins, thresholds=thresholds,
                   tile_ranges=w, symmetric=symmetric, out_pad=pad, side_stream=side_stream,
                   order=order, xcd_swizzle=swizzle, band_rows=band, split_wgs=wgs,
                   dyn_tail_tiles=dyn, max_launch_blocks=blocks, reuse_prepared=reuse,
                   filter_quadrant_cap=qcap, filter_cand_cap=ccap, filter_split_min_steps=smin,
                   filter_check0=chk0, filter_check1=chk1, filter_check_min_steps=4,
                   filter_sort=srt, filter_lazy_codes=lazy, filter_check_emit=emit,
                   filter_rotate=rot, filter_rotate_min_steps=4, filter_rotate_min_tiles=0)
        yield tag, geno


def reducing_tags(seed: int, cases: int, first_case: int = 0, size_class=None) -> list:
    return [tag for tag, _ in reducing_cases(seed, cases, first_case, size_class)]


def reducing_oracle(tag, geno):
    """(oracle block, its bitset, ONE all_pairs call) of a case."""
    from oracle import pyoracle
    osm = pyoracle.submatrix(tag["n"], tag["split_factor"], tag["shard"])
    bits = pyoracle.bitset_from_genotypes(geno, osm)
    return osm, bits, pyoracle.all_pairs(osm, bits)


def reducing_compared_share(seed: int, cases: int, size_class=None):
    """(pairs of the sweep, those among them whose kinship is not NaN) from the generator and
    the oracle alone: the share assert_same compares bit for bit."""
    pairs = compared = 0
    for tag, geno in reducing_cases(seed, cases, 0, size_class):
        kin = reducing_oracle(tag, geno)[2][3]
        pairs += kin.size
        compared += int((~np.isnan(kin)).sum())
    return pairs, compared


def reducing_calls(ctx, tag, geno, sm, wps, d_bits, stream, exp, records, stats, fail) -> dict:
    """The record call and the three reducing calls of one case, each as a closure that issues
    the call on `stream` and checks what it gives against `exp` (reducing_cases.expect_all of
    tag["bins"] and tag["thresholds"]) and `records` (the oracle's at tag["thresholds"][0]):
    {"run", "kin_matrix", "kin_summary", "relative_counts"}.  `fail(what, detail)` raises the
    runner's FuzzMismatch.  Shared by run_reducing and run_pihat."""
    import torch
    import reducing_cases as rc
    from cuking_amd.dist import tile_partition
    from test_gpu_kin_matrix import symmetric_expectation

    dev = f"cuda:{ctx.device}"
    sentinel = float(rc.SENTINEL)
    thresholds, bins, w = tag["thresholds"], tag["bins"], tag["tile_ranges"]
    block = sm.as_tuple()
    kin = exp.pairs[2]
    above = int((kin > np.float32(thresholds[0])).sum())
    suffix = exp.bands[:, ::-1].astype(np.uint64).cumsum(axis=1)[:, ::-1]
    rows, cols, stored = sm.NumRows(), sm.NumCols(), sm.NumSamples()
    symmetric = tag["symmetric"] and block[0] == block[2]

    def host(t):
        """After ONE wait for the case's stream, nothing else."""
        stream.synchronize()
        return t.cpu().numpy()

    def select(variant):
        if variant == "stream":
            ctx.set_kernel("stream")
        else:
            ctx.set_kernel("tiled")
            ctx.set_option("variant", variant)

    def ranges():
        tiles = ctx.num_tiles(sm) if rows and cols else 0
        return tile_partition(tiles, w) if tiles >= 2 else []

    def matrix_into():
        """(the prefilled buffer, its [rows, cols] view with a row pitch of its own)"""
        buf = torch.full((rows, cols + tag["out_pad"]), sentinel, dtype=torch.float32,
                         device=dev)
        return buf, buf[:, :cols]

    def check_matrix(buf, want, what):
        got = host(buf)
        try:
            rc.assert_same(np.ascontiguousarray(got[:, :cols]), want, what)
        except AssertionError as e:
            fail(what, str(e))
        if not (got[:, cols:] == rc.SENTINEL).all():
            fail(what, "the padding columns of the strided output were written")

    def call_run():
        select(tag["variant"])
        for rep in range(2 if tag["reuse_prepared"] else 1):   # the second call reuses the layout
            got = ctx.run(sm, wps, d_bits, thresholds[0])
            if got.tobytes() != records.tobytes():
                fail(f"run (rep {rep})", _diff(got, records))

    def call_kin_matrix():
        select(tag["matrix_variant"])
        buf, out = matrix_into()
        ctx.kin_matrix(sm, wps, d_bits, out=out, symmetric=symmetric, stream=stream)
        want = exp.matrix
        if symmetric:
            want = symmetric_expectation(exp.matrix, geno[block[0]:block[1]])
        check_matrix(buf, want, f"kin_matrix (symmetric {symmetric})")
        if tag["matrix_variant"] != "stream" and ranges():
            buf, out = matrix_into()
            for r in ranges():
                ctx.kin_matrix(sm, wps, d_bits, out=out, tile_range=r, stream=stream)
            check_matrix(buf, exp.matrix, f"kin_matrix, {w} tile ranges")

    def check_summary(summary, pattern, times, what):
        hist = host(summary.hist).view(np.uint64)
        keys = host(summary.best).view(np.uint64)
        added = hist - pattern
        if not np.array_equal(added, times * exp.hist):
            fail(what, f"histogram differs at slots "
                       f"{np.flatnonzero(added != times * exp.hist)[:8]}")
        if int(added.sum()) != times * kin.size:
            fail(what, f"{int(added.sum())} pairs counted, the block has {kin.size}")
        if not np.array_equal(keys, exp.keys):
            fail(what, f"keys differ at samples {np.flatnonzero(keys != exp.keys)[:8]}")
        best_kin, partner = rc.decode_keys(keys)
        nan = np.isnan(exp.best_kin)
        if not (np.array_equal(partner, exp.best_partner) and np.isnan(best_kin[nan]).all()
                and np.array_equal(best_kin.view(np.uint32)[~nan],
                                   exp.best_kin.view(np.uint32)[~nan])):
            fail(what, "nearest relatives differ")
        api_kin, api_partner = summary.nearest()
        if not (np.array_equal(api_partner, partner) and
                np.array_equal(api_kin.view(np.uint32), best_kin.view(np.uint32))):
            fail(what, "KinSummary.nearest() decodes the keys differently")

    def call_kin_summary():
        select(tag["variant"])
        pattern = (np.arange(bins[2] + 3, dtype=np.uint64) * np.uint64(7) + np.uint64(3))
        kw = dict(lo=bins[0], hi=bins[1], bins=bins[2], stream=stream)

        def outputs():
            return (torch.from_numpy(pattern.view(np.int64).copy()).to(dev),
                    torch.zeros(stored, dtype=torch.int64, device=dev))
        hist, best = outputs()
        summary = ctx.kin_summary(sm, wps, d_bits, hist=hist, best=best, **kw)
        check_summary(summary, pattern, 1, "kin_summary")
        if ranges():
            hist, best = outputs()
            for r in ranges():
                summary = ctx.kin_summary(sm, wps, d_bits, hist=hist, best=best,
                                          tile_range=r, **kw)
            check_summary(summary, pattern, 1, f"kin_summary, {w} tile ranges")

    def check_counts(counts, times, what):
        got = host(counts.counts).view(np.uint32).reshape(stored, len(thresholds))
        if not np.array_equal(got, np.uint32(times) * exp.bands):
            fail(what, f"counts differ at (sample, band) "
                       f"{np.argwhere(got != np.uint32(times) * exp.bands)[:8].tolist()}")
        if not np.array_equal(counts.at_least(), np.uint64(times) * suffix):
            fail(what, "suffix sums differ")
        if counts.num_records(0) != times * above:
            fail(what, f"num_records(0) {counts.num_records(0)}, the oracle has "
                       f"{above} pairs above {thresholds[0]}")

    def call_relative_counts():
        select(tag["variant"])
        giveup = tag["size_class"] == "giveup"
        before = ctx.get_option("filter_dense_quadrants") if giveup else 0
        out = torch.zeros((stored, len(thresholds)), dtype=torch.int32, device=dev)
        counts = ctx.relative_counts(sm, wps, d_bits, thresholds=thresholds, out=out,
                                     stream=stream)
        check_counts(counts, 1, "relative_counts")
        if giveup:
            stats["giveup_dense_quadrants"] += \
                ctx.get_option("filter_dense_quadrants") - before
        ctx.relative_counts(sm, wps, d_bits, thresholds=thresholds, out=out, stream=stream)
        check_counts(counts, 2, "relative_counts, a second call into the same tensor")
        if ranges():
            out = torch.zeros((stored, len(thresholds)), dtype=torch.int32, device=dev)
            for r in ranges():
                counts = ctx.relative_counts(sm, wps, d_bits, thresholds=thresholds,
                                             out=out, tile_range=r, stream=stream)
            check_counts(counts, 1, f"relative_counts, {w} tile ranges")

    return dict(run=call_run, kin_matrix=call_kin_matrix, kin_summary=call_kin_summary,
                relative_counts=call_relative_counts)


def run_reducing(ctx, seed: int, cases: int, first_case: int = 0, log=None, size_class=None,
                 stats=None) -> int:
    """The three reducing calls and the record call, interleaved in a random order over one
    bitset (and with reuse_prepared one prepared layout): shapes up to launches of >= 64 tiles
    and more tiles than CUs, every block of a split, every option run_general draws plus the
    launch shapes, bins, thresholds, tile ranges, a strided output, a side stream
    (tools/fuzz_reducing.py).  Everything is compared exactly with what ONE oracle.all_pairs
    call gives (tests/reducing_cases.py).  Returns the number of cases run; `stats`, a dict,
    gains the sweep's `pairs`, `compared` (those whose kinship is not NaN: compared bit for
    bit) and `giveup_dense_quadrants` (the filter_dense_quadrants counter's rise over the
    relative_counts calls of the class "giveup")."""
    import torch
    import cuking_amd
    import reducing_cases as rc
    from oracle import pyoracle

    stats = stats if stats is not None else {}
    for key in ("pairs", "compared", "giveup_dense_quadrants"):
        stats.setdefault(key, 0)
    dev = f"cuda:{ctx.device}"
    t0, ran = time.time(), 0
    try:
        for tag, geno in reducing_cases(seed, cases, first_case, size_class):
            n, m, k, shard = tag["n"], tag["m"], tag["split_factor"], tag["shard"]
            thresholds, bins = tag["thresholds"], tag["bins"]
            osm, bits, all_pairs = reducing_oracle(tag, geno)
            block = osm.as_tuple()
            exp = rc.expect_all(block, all_pairs, bins, thresholds)
            kin = exp.pairs[2]
            stats["pairs"] += kin.size
            stats["compared"] += int((~np.isnan(kin)).sum())
            records, _, _ = pyoracle.compute(osm, bits, thresholds[0], threads=8)
            above = int((kin > np.float32(thresholds[0])).sum())
            if above != len(records):
                raise FuzzMismatch(f"the oracle disagrees with itself: {above} pairs above "
                                   f"{thresholds[0]}, {len(records)} records; {tag}")
            sm = cuking_amd.Submatrix(n, k, shard)
            assert sm.as_tuple() == block

            for key in SHIPPED:
                if key != "variant":
                    ctx.set_option(key, tag[key])
            # (a new bitset may land on a recycled pointer: tell the library)
            ctx.invalidate()
            d_bits = (ctx.upload_bitset(bits) if bits.shape[0] else
                      torch.zeros(2, dtype=torch.int64, device=dev))
            wps = cuking_amd.words_per_sample(m)
            stream = torch.cuda.Stream(dev) if tag["side_stream"] else torch.cuda.current_stream()
            stream.wait_stream(torch.cuda.current_stream())

            def fail(what, detail=""):
                raise FuzzMismatch(f"{what}: {detail}; reproduce with {tag} (tools/fuzz_reducing.py "
                                   f"{seed} {tag['case'] + 1} {tag['case']} {tag['sweep']})")

            calls = reducing_calls(ctx, tag, geno, sm, wps, d_bits, stream, exp, records, stats,
                                   fail)
            with torch.cuda.stream(stream):
                for name in tag["order"]:
                    calls[name]()
            stream.synchronize()
            ran += 1
            if log and tag["case"] % 10 == 0:
                log(f"run_reducing seed {seed} case {tag['case']} ok ({time.time() - t0:.0f}s)")
    finally:
        ctx.set_kernel("tiled")
        for key, value in SHIPPED.items():
            ctx.set_option(key, value)
        ctx.invalidate()
    return ran


# ---- the filter path with the site order on --------------------------------------------------
def run_site_order(ctx, seed: int, cases: int, first_case: int = 0, log=None, stats=None) -> int:
    """The filter variant with "filter_site_order" 1 / 2 / -1 (tests/site_order_cases.py): every
    block of a split, lengths from one site to 94 k-steps, thresholds the filter runs for and
    does not, lean and full forms, every gather form, everything run_general draws for the
    filter, and three to six of -- the record call, the record call at a second threshold, tile
    ranges, relative_counts, kin_matrix, a staged pass -- in a random order over one bitset, on
    a side stream in some cases (tools/fuzz_site_order.py).  Everything is compared exactly
    with what ONE oracle.all_pairs call gives.  Behind every whole-block call for which
    prepare() makes it plain (site_order_cases.expected_flag) "site_order_on" must be what
    the rule says: a silent fall-back to stored order is a mismatch.  Returns the number of
    cases run; `stats`, a dict, gains the calls per kind, `expected_ordered` and `ordered`
    (whole-block calls the rule expects an ordered layout behind, and those of them that left
    one), `automatic_ordered` (calls under a rule the sweep only records that left one),
    `early_exits` (the rise of filter_early_exits) and `gathers` (the values of
    "filter_site_gather" a call ordered a layout under)."""
    import torch
    import cuking_amd
    import reducing_cases as rc
    import site_order_cases as so
    from cuking_amd.dist import tile_partition

    stats = stats if stats is not None else {}
    for key in so.KINDS + ("expected_ordered", "ordered", "automatic_ordered", "early_exits"):
        stats.setdefault(key, 0)
    stats.setdefault("gathers", [])
    shipped = dict(SHIPPED, **so.SHIPPED)
    dev = f"cuda:{ctx.device}"
    t0, ran = time.time(), 0
    exits0 = ctx.get_option("filter_early_exits")
    try:
        for tag, geno in so.site_order_cases(seed, cases, first_case):
            n, m, k, shard = tag["n"], tag["m"], tag["split_factor"], tag["shard"]
            thresholds, w = tag["thresholds"], tag["tile_ranges"]
            osm, bits, all_pairs = so.site_order_oracle(tag, geno)
            block = osm.as_tuple()
            exp = rc.expect_all(block, all_pairs, BIN_MENU[0], thresholds)
            records = {t: so.records_of(all_pairs, t) for t in (tag["thr"], tag["thr2"])}
            sm = cuking_amd.Submatrix(n, k, shard)
            assert sm.as_tuple() == block and bits.shape[0] == sm.NumSamples() >= 2
            rows, cols, stored = sm.NumRows(), sm.NumCols(), sm.NumSamples()

            ctx.set_kernel("tiled")
            for key in shipped:
                if key in tag:
                    ctx.set_option(key, tag[key])
            ctx.set_option("variant", 7)
            # (a new bitset may land on a recycled pointer: tell the library)
            ctx.invalidate()
            d_bits = ctx.upload_bitset(bits)
            wps = cuking_amd.words_per_sample(m)
            stream = torch.cuda.Stream(dev) if tag["side_stream"] else torch.cuda.current_stream()
            stream.wait_stream(torch.cuda.current_stream())

            def fail(what, detail=""):
                raise FuzzMismatch(f"{what}: {detail}; reproduce with {tag} "
                                   f"(tools/fuzz_site_order.py {seed} {tag['case'] + 1} "
                                   f"{tag['case']})")

            def flag(kind):
                """"site_order_on" behind a whole-block call, against the rule."""
                got = ctx.get_option("site_order_on")
                want = so.expected_flag(tag, kind, so.call_threshold(tag, kind))
                if want is None:
                    stats["automatic_ordered"] += got
                else:
                    stats["expected_ordered"] += want
                    stats["ordered"] += got
                    if got != want:
                        fail(kind, f"site_order_on {got}, the rule says {want}")
                if got and tag["filter_site_gather"] not in stats["gathers"]:
                    stats["gathers"] = sorted(stats["gathers"] + [tag["filter_site_gather"]])

            def call_run(kind="run"):
                thr = so.call_threshold(tag, kind)
                for rep in range(2 if tag["reuse_prepared"] else 1):   # the second call reuses the layout
                    got = ctx.run(sm, wps, d_bits, thr)
                    if got.tobytes() != records[thr].tobytes():
                        fail(f"{kind} at {thr} (rep {rep})", _diff(got, records[thr]))
                    flag(kind)

            def call_tile_ranges():
                tiles = ctx.num_tiles(sm)
                parts = [ctx.run(sm, wps, d_bits, tag["thr"], tile_range=r)
                         for r in tile_partition(tiles, w)]
                merged = cuking_amd.sort_results(np.ascontiguousarray(np.concatenate(parts)))
                if merged.tobytes() != records[tag["thr"]].tobytes():
                    fail(f"{w} tile ranges", _diff(merged, records[tag["thr"]]))

            def call_relative_counts():
                out = torch.zeros((stored, len(thresholds)), dtype=torch.int32, device=dev)
                for times in (1, 2):                 # the call accumulates
                    counts = ctx.relative_counts(sm, wps, d_bits, thresholds=thresholds, out=out,
                                                 stream=stream)
                    stream.synchronize()
                    got = counts.bands()
                    if not np.array_equal(got, np.uint32(times) * exp.bands):
                        fail(f"relative_counts (call {times})", f"counts differ at (sample, band) "
                             f"{np.argwhere(got != np.uint32(times) * exp.bands)[:8].tolist()}")
                    if counts.num_records(0) != times * len(records[tag["thr"]]):
                        fail("relative_counts", f"num_records(0) {counts.num_records(0)}, the "
                             f"oracle has {len(records[tag['thr']])} records")
                    flag("relative_counts")

            def call_kin_matrix():
                out = torch.full((rows, cols), float(rc.SENTINEL), dtype=torch.float32, device=dev)
                ctx.kin_matrix(sm, wps, d_bits, out=out, stream=stream)
                stream.synchronize()
                try:
                    rc.assert_same(out.cpu().numpy(), exp.matrix, "kin_matrix")
                except AssertionError as e:
                    fail("kin_matrix", str(e))
                if ctx.get_option("site_order_on"):
                    fail("kin_matrix", "the dense layout claims the site order")

            def call_staged():
                want = records[tag["thr"]]
                merged = _staged(ctx, sm, wps, d_bits, tag["thr"], max(len(want), 1) + 8, n,
                                 tag["world"], tag["chunks"], tag["streams"])
                if merged.tobytes() != want.tobytes():
                    fail(f"staged (world {tag['world']}, chunks {tag['chunks']}, streams "
                         f"{tag['streams']})", _diff(merged, want))
                if ctx.get_option("site_order_on"):
                    fail("staged", "a staged pass claims the site order")

            calls = dict(run=call_run, run2=lambda: call_run("run2"),
                         tile_ranges=call_tile_ranges, relative_counts=call_relative_counts,
                         kin_matrix=call_kin_matrix, staged=call_staged)
            with torch.cuda.stream(stream):
                for kind in tag["calls"]:
                    calls[kind]()
                    stats[kind] += 1
            stream.synchronize()
            ran += 1
            if log and tag["case"] % 10 == 0:
                log(f"run_site_order seed {seed} case {tag['case']} ok ({time.time() - t0:.0f}s)")
    finally:
        stats["early_exits"] += ctx.get_option("filter_early_exits") - exits0
        ctx.set_kernel("tiled")
        for key, value in shipped.items():
            ctx.set_option(key, value)
        ctx.invalidate()
    return ran


# ---- PC-Relate: matrix, records and listed pairs over one bitset and one model -----------------
PCR_GUARD = 0x7FC00123                 # a NaN of its own: a kernel's NaN in a guard shows


def run_pcrelate(ctx, seed: int, cases: int, first_case: int = 0, log=None, size_class=None,
                 stats=None, twin_every: int = 1) -> int:
    """The three PC-Relate calls (tests/pcrelate_fuzz_cases.py has the cases and the size
    classes "small", "tiles" and "exact"): per case, on the case's stream and under its launch
    cap, the matrix of the block, the matrix of a sub-block, the records and the listed pairs in
    the drawn order, checked after one wait at the end -- against the float64 references of
    pcrelate_cases.py and pcrelate_pairs_cases.py within their tolerances, against each other
    on bytes (the sub-block and the records against the matrix, a reordered part of the list
    against the list) and against the host twins (on every `twin_every`-th case; on bytes in the
    class "exact").  The record call returns its count, so it waits by itself; and its two
    thresholds that pairs sit ON -- the median and the 95th-percentile value of the device
    matrix -- need the matrix on the host: those two calls follow the wait.  Returns the number
    of cases run; `stats`, a dict, gains the calls per kind, `d_seen` (per kernel the sorted D
    buckets launched), `split_launches` (calls under a launch cap that really split them),
    `entries` and `compared` (matrix entries, and those of them that are not NaN and so were
    held to a tolerance or to bytes)."""
    import torch
    import cuking_amd
    import pcrelate_cases as pc
    import pcrelate_fuzz_cases as pf
    import pcrelate_pairs_cases as pp
    import pcrelate_records_cases as rc
    from cuking_amd import pcrelate as pcr

    stats = stats if stats is not None else {}
    for key in ("matrix", "matrix_sub", "records", "pairs", "split_launches", "entries",
                "compared", "twins"):
        stats.setdefault(key, 0)
    stats.setdefault("d_seen", {kind: [] for kind in pf.KINDS})
    dev = f"cuda:{ctx.device}"
    t0, ran = time.time(), 0
    try:
        for tag, inp in pf.pcrelate_sweep_cases(seed, cases, first_case, size_class):
            exact = tag["size_class"] == "exact"
            sites, block, sub = tag["sites"], inp.block, inp.sub_block
            rows, cols = block[1] - block[0], block[3] - block[2]
            splits = pf.split_launches(tag)

            def fail(what, detail=""):
                raise FuzzMismatch(f"{what}: {detail}; reproduce with {tag} "
                                   f"(tools/fuzz_pcrelate.py {seed} {tag['case'] + 1} "
                                   f"{tag['case']} {tag['size_class']})")

            def held(what, check, *args, **kw):
                try:
                    return check(*args, **kw)
                except AssertionError as e:
                    fail(what, str(e)[:400])

            def padded(a):   # the host's pitch, NaN between the columns and the pitch
                wide = np.full((a.shape[0], a.strides[0] // 4), np.float32(np.nan), np.float32)
                wide[:, :a.shape[1]] = a
                return torch.from_numpy(wide).to(dev)[:, :a.shape[1]]

            def guarded(shape):
                return torch.full(shape, PCR_GUARD, dtype=torch.int32, device=dev)

            # (a new bitset may land on a recycled pointer: tell the library)
            ctx.invalidate()
            bits = ctx.upload_bitset(inp.bits.copy())
            x, beta = padded(inp.x), padded(inp.beta)
            f = None if inp.f is None else torch.from_numpy(inp.f).to(dev)
            words = np.ascontiguousarray(inp.pairs).view(np.int32).reshape(-1, tag["stride"] // 4)
            d_list = torch.from_numpy(words.copy()).to(dev)
            d_part = torch.from_numpy(words[inp.part].copy()).to(dev)
            head = (bits, inp.wps, sites, x, beta, inp.lo, inp.hi)
            wide = guarded((rows + 2, cols + tag["pads"][2]))
            sub_rows, sub_cols = sub[1] - sub[0], sub[3] - sub[2]
            sub_wide = guarded((sub_rows + 2, sub_cols + tag["pads"][2]))
            room = max(rc.num_pairs(block), 1)
            rec_buf = guarded((room + 3, 6))
            got = {}
            stream = torch.cuda.Stream(dev) if tag["side_stream"] else torch.cuda.current_stream()
            stream.wait_stream(torch.cuda.current_stream())

            def records_at(min_kin, **kw):
                recs, count = ctx.pcrelate_records_raw(*head, min_kin, block=block, stream=stream,
                                                       **kw)
                return pcr.records_to_host(recs, count), count

            def call_matrix():
                ctx.pcrelate_matrix(*head, block=block, stream=stream,
                                    out=wide.view(torch.float32)[1:rows + 1, :cols])

            def call_matrix_sub():
                ctx.pcrelate_matrix(*head, block=sub, stream=stream,
                                    out=sub_wide.view(torch.float32)[1:sub_rows + 1, :sub_cols])

            def call_records():
                got["records"] = records_at(-np.inf, max_records=room, out=rec_buf)
                got["none"] = records_at(np.inf)
                total = got["records"][1]
                if tag["short_buffer"] and total > 0:
                    short = guarded((total + 2, 6))
                    try:
                        records_at(-np.inf, max_records=total - 1, out=short)
                        fail("records", f"a buffer of {total - 1} records took {total}")
                    except cuking_amd.ResourceExhaustedError as e:
                        if e.num_records != total:
                            fail("records", f"a short buffer counted {e.num_records}, not {total}")
                    got["short"] = short

            def call_pairs():
                got["pairs"] = ctx.pcrelate_pairs_raw(*head, d_list, f, stream=stream)
                got["part"] = ctx.pcrelate_pairs_raw(*head, d_part, f, stream=stream)

            calls = dict(matrix=call_matrix, matrix_sub=call_matrix_sub, records=call_records,
                         pairs=call_pairs)
            ctx.set_option("max_launch_blocks", tag["max_launch_blocks"])
            with torch.cuda.stream(stream):
                for kind in tag["calls"]:
                    calls[kind]()
                    stats[kind] += 1
                    stats["split_launches"] += bool(splits[kind])
                    seen = stats["d_seen"][kind.split("_")[0]]
                    if pf.bucket(tag["d"]) not in seen:
                        seen.append(pf.bucket(tag["d"]))
                        seen.sort()
            stream.synchronize()                 # THE wait

            # ---- the matrix
            host = wide.cpu().numpy()
            kin = np.ascontiguousarray(host[1:rows + 1, :cols]).view(np.float32)
            touched = host.copy()
            touched[1:rows + 1, :cols] = PCR_GUARD
            if (touched != PCR_GUARD).any():
                fail("matrix", f"guard rows or pitch written at {np.argwhere(touched != PCR_GUARD)[:5].tolist()}")
            stats["entries"] += kin.size
            stats["compared"] += int((~np.isnan(kin)).sum())
            if exact:
                want = pc.exact_expected_of(inp.code, inp.beta, block)
                if kin.tobytes() != want.tobytes():
                    fail("matrix", "differs from the integer formula at "
                         f"{np.argwhere(kin.view(np.uint32) != want.view(np.uint32))[:5].tolist()}")
            else:
                held("matrix against the float64 reference", pc.check_reference_of, inp.ref, kin,
                     "matrix", quiet=True)
            if rc.is_diagonal(block) and not np.array_equal(kin.view(np.uint32),
                                                            kin.view(np.uint32).T):
                fail("matrix", "a diagonal block is not bytewise symmetric")
            sub_host = sub_wide.cpu().numpy()
            sub_kin = sub_host[1:sub_rows + 1, :sub_cols].copy()
            sub_host[1:sub_rows + 1, :sub_cols] = PCR_GUARD
            if (sub_host != PCR_GUARD).any():
                fail("matrix_sub", "guard rows or pitch written")
            same = kin.view(np.int32)[sub[0] - block[0]:sub[1] - block[0],
                                      sub[2] - block[2]:sub[3] - block[2]]
            if not np.array_equal(sub_kin, same):
                fail("matrix_sub", f"block {sub} differs from the same entries of {block} at "
                     f"{np.argwhere(sub_kin != same)[:5].tolist()}")

            # ---- the records: the matrix thresholded, on bytes
            def records_hold(recs, count, min_kin, what):
                want = rc.threshold_matrix(kin, block, min_kin)
                if count != recs.shape[0] or count != want.shape[0]:
                    fail(what, f"count {count}, {recs.shape[0]} records, the matrix gives "
                         f"{want.shape[0]}")
                held(what, rc.check_records, recs, block)
                held(what, rc.same_records, recs, want)

            everything, total = got["records"]
            records_hold(everything, total, -np.inf, "records at -inf")
            records_hold(*got["none"], np.inf, "records at +inf")
            if not exact:
                held("records at -inf against the float64 reference", rc.check_records_reference,
                     inp.ref, block, everything, "records", quiet=True)
            if (rec_buf[total:].cpu().numpy() != PCR_GUARD).any():
                fail("records", "written behind the count")
            if "short" in got:
                short = got["short"].cpu().numpy()
                if (short[total - 1:] != PCR_GUARD).any():
                    fail("records", "a short buffer was written behind max_records")
                stored = np.ascontiguousarray(short[:total - 1]).view(
                    cuking_amd.KING_RESULT_DTYPE).reshape(-1)
                held("records in a short buffer", rc.check_records, stored, block)
            values = np.sort(kin[rc.pair_mask(block) & ~np.isnan(kin)])
            on_value = [float(values[int(q * values.size)]) for q in (0.5, 0.95)] \
                if values.size else []
            with torch.cuda.stream(stream):
                for t in on_value:               # (a pair sits on t: the strict > decides)
                    records_hold(*records_at(t), t, f"records at the value {t!r}")
                    stats["records"] += 1

            # ---- the listed pairs
            rows_got = pcr.pairs_to_host(got["pairs"])
            held("pairs", pp.check_rows_of, inp.index, rows_got)
            if exact:
                want = pp.exact_expected_of(inp)
                if rows_got.tobytes() != want.tobytes():
                    fail("pairs", "differ from the integer formula")
            else:
                held("pairs against the float64 reference", pp.check_reference_of, inp.pair_ref,
                     inp.index, rows_got, "pairs", quiet=True)
                # the kin of a listed pair of the block against the matrix entry
                i, j = inp.index[:, 0].astype(np.int64), inp.index[:, 1].astype(np.int64)
                ok = (i >= block[0]) & (i < block[1]) & (j >= block[2]) & (j < block[3])
                entry = kin[i[ok] - block[0], j[ok] - block[2]]
                mine = rows_got["kin"][ok]
                if not np.array_equal(np.isnan(entry), np.isnan(mine)):
                    fail("pairs", "NaN where the matrix has none, or the reverse")
                fin = ~np.isnan(entry)
                tol = inp.ref.twin_tolerance()[i[ok] - block[0], j[ok] - block[2]]
                if (np.abs(mine.astype(np.float64) - entry)[fin] > tol[fin]).any():
                    fail("pairs", "kin further than the twin tolerance from the matrix entry")
            part_got = pcr.pairs_to_host(got["part"])
            if part_got.tobytes() != rows_got[inp.part].tobytes():
                fail("pairs", "a reordered part of the list gives other row bytes")

            # ---- the host twins
            if tag["case"] % twin_every == 0:
                stats["twins"] += 1
                model = (inp.bits, inp.wps, sites, inp.x, inp.beta, inp.lo, inp.hi)
                twin = pcr.pcrelate_matrix_host(*model, block=block)
                if exact:
                    if twin.tobytes() != kin.tobytes():
                        fail("matrix", "differs from the host twin's bytes")
                else:
                    held("matrix against the host twin", pc.check_twin_of, inp.ref, kin, twin,
                         "matrix", quiet=True)
                for t, (recs, _) in ((-np.inf, got["records"]), (np.inf, got["none"])):
                    twin_recs, _ = pcr.pcrelate_records_raw_host(*model, t, block=block)
                    if rc.pair_set(twin_recs) != rc.pair_set(recs):
                        fail(f"records at {t}", "another pair set than the host twin's")
                    if exact:
                        held(f"records at {t} against the host twin", rc.same_records, recs,
                             twin_recs)
                twin_rows = pcr.pcrelate_pairs_raw_host(*model, inp.pairs, inp.f)
                if twin_rows.tobytes() != rows_got.tobytes():
                    fail("pairs", "differ from the host twin's bytes")
            ran += 1
            if log and tag["case"] % 10 == 0:
                log(f"run_pcrelate seed {seed} case {tag['case']} ok ({time.time() - t0:.0f}s)")
    finally:
        ctx.set_option("max_launch_blocks", 0)
        ctx.invalidate()
    return ran


# ---- PI_HAT among the pair calls ----------------------------------------------------------------
def run_pihat(ctx, seed: int, cases: int, first_case: int = 0, log=None, size_class=None,
              stats=None, twin_every: int = 1) -> int:
    """The PI_HAT scan among the other pair calls (tests/pihat_fuzz_cases.py has the cases and
    the size classes "small", "edges" and "tiles"): per case one bitset, uploaded once, and on the
    case's stream, in the drawn order -- pi_hat_records at the case's threshold, model and
    `bounded`; the other setting of `bounded` at -1.0 (every pair that is not NaN is a record);
    the raw tile-range entry point over tile_partition, each range into a buffer of its own; the
    count alone (capacity 0); a buffer one record short; compute_counts; the KING records; and
    kin_matrix or relative_counts (reducing_calls), which leave another layout and other codes in
    the workspace between the PI_HAT calls.  Everything is compared on bytes with what ONE
    pyoracle.all_pairs call gives: the oracle's sums, and the numpy restatement of the pair math
    over their IBS counts (pihat_cases.records_np); every `twin_every`-th case the host twin is
    held to the same bytes (tools/fuzz_pihat.py).  Returns the number of cases run; `stats`, a
    dict, gains `pairs`, `records` (of the thresholded call), `twins`, `branches` (the bounding
    steps of pihat_cases.BRANCHES that pairs of the blocks took), `models`, `variants`,
    `split_launches` (PI_HAT launches whose plan by king_launch_plan.h has remainder pieces) and
    `ties` (per threshold value, the pairs whose float32 PI_HAT equals it: the strict > decides)."""
    import torch
    import cuking_amd
    import pihat_cases as pc
    import pihat_fuzz_cases as pf
    import reducing_cases as rc
    from cuking_amd import _lib
    from cuking_amd.dist import tile_partition
    from oracle import pyoracle

    stats = stats if stats is not None else {}
    for key in ("pairs", "records", "twins", "split_launches"):
        stats.setdefault(key, 0)
    for key in ("branches", "models", "variants"):
        stats.setdefault(key, [])
    stats.setdefault("ties", {})
    dev = f"cuda:{ctx.device}"
    t0, ran = time.time(), 0

    def seen(key, value):
        if value not in stats[key]:
            stats[key] = sorted(stats[key] + [value], key=str)

    try:
        for tag, geno, spec in pf.cases(seed, cases, first_case, size_class):
            n, m, k, shard = tag["n"], tag["m"], tag["split_factor"], tag["shard"]
            thr, bounded, w = tag["thr"], tag["bounded"], tag["tile_ranges"]
            model = pf.model_of(tag, geno)
            ref = pf.reference(tag, geno, model)
            osm, bits = ref.osm, ref.bits
            block = osm.as_tuple()
            oi, oj, oc, _ = ref.all_pairs
            want, other = ref.records[(thr, bounded)], ref.records[(-1.0, not bounded)]
            listed = {r.tobytes() for r in want}
            exp = rc.expect_all(block, ref.all_pairs, tag["bins"], tag["thresholds"])
            records, _, _ = pyoracle.compute(osm, bits, tag["thresholds"][0], threads=8)
            sm = cuking_amd.Submatrix(n, k, shard)
            assert sm.as_tuple() == block and bits.shape[0] == sm.NumSamples() >= 2
            if pf.planted_pairs(tag)["all_missing"] and not len(other) < sm.NumPairs():
                raise FuzzMismatch(f"the reference lists a pair of the all-missing sample; {tag}")

            ctx.set_kernel("tiled")
            for key in SHIPPED:
                if key in tag:
                    ctx.set_option(key, tag[key])
            # (a new bitset may land on a recycled pointer: tell the library)
            ctx.invalidate()
            d_bits = ctx.upload_bitset(bits)
            d_founders = ctx.upload_bitset(pf.host_bits(pf.model_rows(tag, geno))) \
                if spec == "founders" else None
            wps = cuking_amd.words_per_sample(m)
            stream = torch.cuda.Stream(dev) if tag["side_stream"] else torch.cuda.current_stream()
            stream.wait_stream(torch.cuda.current_stream())

            def fail(what, detail=""):
                raise FuzzMismatch(f"{what}: {detail}; reproduce with {tag} (tools/fuzz_pihat.py "
                                   f"{seed} {tag['case'] + 1} {tag['case']} {tag['size_class']})")

            def use():
                """The case's variant (the lean call may have left another kernel selected)."""
                ctx.set_kernel("tiled")
                ctx.set_option("variant", tag["variant"])

            def model_args():
                if spec == "block":
                    return {}
                if spec == "founders":
                    return dict(counts=ctx.site_counts(d_founders, wps, stream=stream))
                return dict(model=model)

            def scan(min_pi_hat, bound, expect, what):
                use()
                got = ctx.pi_hat_records(sm, wps, d_bits, m, min_pi_hat, bounded=bound,
                                         stream=stream, **model_args())
                rows = got.sorted()
                if got.num_records != len(expect) or rows.tobytes() != expect.tobytes():
                    fail(what, _diff(rows, expect))
                if spec in ("block", "founders") and not (
                        got.model.sites_used == model.sites_used and np.array_equal(
                            pc.bits(got.model.as_tuple()[:5]), pc.bits(model.as_tuple()[:5]))):
                    fail(what, f"model {got.model}, pi_hat_model_host of the same rows {model}")

            def raw(capacity, tile_range=None):
                use()
                return pc.raw_call(ctx, sm, wps, d_bits, model, capacity, tile_range,
                                   stream=stream, min_pi_hat=float(np.float32(thr)),
                                   flags=0 if bounded else _lib.PIHAT_UNBOUNDED)

            def untouched(behind, what):
                if not (behind == 0x55555555).all():
                    fail(what, "the rows behind the buffer were written")

            def call_tiles():
                use()
                tiles = ctx.num_tiles(sm)
                if tiles != pf.num_tiles(tag):
                    fail("pi_hat tiles", f"{tiles} tiles, pihat_fuzz_cases.num_tiles says "
                                         f"{pf.num_tiles(tag)}")
                parts = [raw(max(len(want), 1), r) for r in tile_partition(tiles, w)]
                if sum(count for _, count, _, _ in parts) != len(want):
                    fail(f"pi_hat, {w} tile ranges", f"the counts "
                         f"{[count for _, count, _, _ in parts]} do not add up to {len(want)}")
                if any(overflow for _, _, overflow, _ in parts):
                    fail(f"pi_hat, {w} tile ranges", "an overflow flag is set")
                for _, _, _, behind in parts:
                    untouched(behind, f"pi_hat, {w} tile ranges")
                merged = cuking_amd.sort_results(np.ascontiguousarray(
                    np.concatenate([rows for rows, _, _, _ in parts])))
                if merged.tobytes() != want.tobytes():
                    fail(f"pi_hat, {w} tile ranges", _diff(merged, want))

            def call_count():
                rows, count, overflow, behind = raw(0)
                if (len(rows), count, overflow) != (0, len(want), int(len(want) > 0)):
                    fail("pi_hat count", f"capacity 0 gives count {count}, flag {overflow}; the "
                                         f"reference has {len(want)} records")
                untouched(behind, "pi_hat count")

            def call_one_short():
                total = len(want)
                if total == 0:
                    return
                rows, count, overflow, behind = raw(total - 1)
                if (count, overflow) != (total, 1):
                    fail("pi_hat one short", f"count {count}, flag {overflow}; the reference has "
                                             f"{total} records")
                untouched(behind, "pi_hat one short")
                stored = [r.tobytes() for r in rows]
                if len(stored) != total - 1 or len(set(stored)) != len(stored) or \
                        not all(r in listed for r in stored):
                    fail("pi_hat one short", "a stored row is not one of the reference's, or is "
                                             "stored twice")

            def call_counts():
                use()
                got = ctx.compute_counts(sm, wps, d_bits, stream=stream)
                sel = got[oi - sm.i_begin, oj - sm.j_begin]
                for field in oc.dtype.names:
                    if not np.array_equal(sel[field], oc[field]):
                        at = np.flatnonzero(sel[field] != oc[field])[:5]
                        fail("counts", f"{field} differs at pairs "
                                       f"{[(int(oi[a]), int(oj[a])) for a in at]}")

            shared = reducing_calls(ctx, tag, geno, sm, wps, d_bits, stream, exp, records, stats,
                                    fail)
            calls = {"pi_hat": lambda: scan(thr, bounded, want, "pi_hat"),
                     "pi_hat unbounded or bounded":
                         lambda: scan(-1.0, not bounded, other,
                                      f"pi_hat at -1.0, bounded {not bounded}"),
                     "pi_hat tiles": call_tiles, "pi_hat count": call_count,
                     "pi_hat one short": call_one_short, "counts": call_counts,
                     "run": shared["run"], "lean": shared[tag["lean"]]}
            with torch.cuda.stream(stream):
                for name in tag["order"]:
                    calls[name]()
            stream.synchronize()

            if tag["case"] % twin_every == 0:
                stats["twins"] += 1
                for t, b in ((thr, bounded), (-1.0, not bounded)):
                    twin = cuking_amd.pi_hat_records_host(sm, wps, bits, m, t, model=model,
                                                          bounded=b).records
                    if twin.tobytes() != ref.records[(t, b)].tobytes():
                        fail(f"the host twin at {t}, bounded {b}",
                             _diff(twin, ref.records[(t, b)]))
            stats["pairs"] += len(oi)
            stats["records"] += len(want)
            stats["split_launches"] += pf.split_launches([tag])[0]
            seen("models", spec)
            seen("variants", tag["variant"])
            for step in pc.BRANCHES:
                if ref.taken.get(step):
                    seen("branches", step)
            if ref.ties:
                stats["ties"][thr] = stats["ties"].get(thr, 0) + ref.ties
            ran += 1
            if log and tag["case"] % 10 == 0:
                log(f"run_pihat seed {seed} case {tag['case']} ok ({time.time() - t0:.0f}s)")
    finally:
        ctx.set_kernel("tiled")
        for key, value in SHIPPED.items():
            ctx.set_option(key, value)
        ctx.invalidate()
    return ran


# ---- the input pipeline: bed, site QC, LD, unrelated set -------------------------------------
GUARD64 = -0x5A5A5A5A5A5A5A5B          # 0xA5A5A5A5A5A5A5A5 as int64
GUARD32 = -0x5A5A5A5B                  # 0xA5A5A5A5 as int32


def run_pipeline(ctx, seed: int, cases: int, first_case: int = 0, log=None, size_class=None,
                 stats=None) -> int:
    """The calls in front of the pair kernels -- pack_bed, site_counts, sample_counts,
    compact_sites, filter_sites, transpose_sites, ld_edges, ld_prune, unrelated_set, prune and a
    pair-kernel call on the filtered bits -- 4 to 10 of them in a random order over one cohort,
    each on a stream of a pool of 10 (the context keeps scratch for 8: entries are evicted) and
    with a launch cap of its own (tools/fuzz_pipeline.py).  Every output is compared exactly,
    guard words included, with the numpy expectation of tests/pipeline_cases.py and with the
    library's host function.  The checks of the asynchronous calls wait until the case's last
    call has been issued.  Returns the number of cases run; `stats`, a dict, gains the calls
    per kind and `evictions`: a stream that returns after eight others were used since."""
    import torch
    import cuking_amd
    import pipeline_cases as pc
    from cuking_amd import api

    stats = stats if stats is not None else {}
    for key in pc.KINDS + ("evictions",):
        stats.setdefault(key, 0)
    dev = f"cuda:{ctx.device}"
    pool = [torch.cuda.Stream(dev) for _ in range(pc.NUM_STREAMS)]
    recent = []                        # streams by last use, the latest last
    t0, ran = time.time(), 0

    def touch(index):
        if index in recent:
            stats["evictions"] += len(recent) - 1 - recent.index(index) >= pc.MAX_STREAMS
            recent.remove(index)
        recent.append(index)

    def host_records(t, count):
        return cuking_amd.sort_results(_records(t, count))

    def device_records(recs, rng):
        words = np.ascontiguousarray(recs[rng.permutation(len(recs))]).view(np.int32)
        return torch.from_numpy(words.reshape(-1, 6).copy()).to(dev)

    try:
        for tag, geno in pc.pipeline_cases(seed, cases, first_case, size_class):
            n, m = geno.shape
            wps = cuking_amd.words_per_sample(m)
            q = cuking_amd.ld_site_words(n)
            bits = pc.pack(geno)
            host_site_bits = None
            ctx.invalidate()
            d_bits = ctx.upload_bitset(bits)
            torch.cuda.synchronize()
            pending = []
            result = dict(bits=d_bits, wps=wps, stream=None)    # of filter_sites / ld_prune
            edges = None               # the current LD edges on the device: (tensor, count)

            for number, (call, e) in enumerate(zip(tag["calls"], pc.expect_calls(tag, geno))):
                kind, stream = call["kind"], pool[call["stream"]]

                def fail(what, call=call, number=number):
                    raise FuzzMismatch(
                        f"{call['kind']} (call {number}): {what}; {call}; reproduce with "
                        f"n={n} m={m} cohort={tag['cohort']} (tools/fuzz_pipeline.py {seed} "
                        f"{tag['case'] + 1} --first-case {tag['case']} --size-class "
                        f"{tag['sweep']})")

                def same(got, want, what, fail=fail):
                    if got.shape != want.shape or got.tobytes() != want.tobytes():
                        where = (np.argwhere(got != want)[:4].tolist()
                                 if got.shape == want.shape else [got.shape, want.shape])
                        fail(f"{what} differs at {where}")

                def later(stream, whole, lo, hi, want, what, guard, same=same, fail=fail):
                    """Once the case's calls are issued: rows [lo, hi) of `whole` equal `want`,
                    the rows around them still hold the guard."""
                    def check():
                        stream.synchronize()
                        host = whole.cpu().numpy()
                        if not ((host[:lo] == guard).all() and (host[hi:] == guard).all()):
                            fail(f"{what}: guard words were written")
                        same(host[lo:hi].view(want.dtype).reshape(want.shape), want, what)
                    pending.append(check)

                def transposed():
                    nonlocal host_site_bits
                    if host_site_bits is None:
                        host_site_bits = pc.site_bits_numpy(geno)
                    return host_site_bits

                touch(call["stream"])
                stats[kind] += 1
                ctx.set_option("max_launch_blocks", call["max_launch_blocks"])
                with torch.cuda.stream(stream):
                    if kind == "pack_bed":
                        sm = cuking_amd.Submatrix(n, call["split"], call["shard"])
                        stored, rows = sm.NumSamples(), e["rows"]
                        rb = rows.shape[1]
                        want = np.full((stored, wps), np.uint64(0xA5A5A5A5A5A5A5A5), np.uint64)
                        for begin, end in e["chunks"]:
                            cuking_amd.pack_bed_host(sm, want, rows[begin:end], rb, begin, end, m)
                        same(want, e["bits"], "pack_bed_host against the numpy decode")
                        whole = torch.full((stored + 2, wps), GUARD64, dtype=torch.int64,
                                           device=dev)
                        buf = torch.zeros(call["offset"] + rows.size, dtype=torch.uint8, device=dev)
                        d_rows = buf[call["offset"]:]
                        d_rows.copy_(torch.from_numpy(rows.reshape(-1)))
                        stream.synchronize()
                        for (begin, end), s in zip(e["chunks"], call["chunk_streams"]):
                            touch(s)
                            ctx.pack_bed(sm, wps, d_rows[begin * rb:end * rb], rb, begin, end, m,
                                         whole[1:stored + 1], stream=pool[s])
                        for s in call["chunk_streams"]:
                            stream.wait_stream(pool[s])
                        later(stream, whole, 1, stored + 1, e["bits"], "the bitset", GUARD64)
                    elif kind == "site_counts":
                        slots = wps // 2 * 64
                        whole = torch.full((slots + 16, 4), GUARD32, dtype=torch.int32, device=dev)
                        whole[:slots] = 0
                        stream.synchronize()
                        last = stream
                        for (begin, end), s in zip(call["ranges"], call["range_streams"]):
                            last.synchronize()     # one `out`, two streams: in turn
                            last = pool[s] if s >= 0 else stream
                            if s >= 0:
                                touch(s)
                            ctx.site_counts(d_bits[begin:end], wps, out=whole[:slots], stream=last)
                        later(last, whole, 0, slots, e["counts"], "site counts", GUARD32)
                    elif kind == "sample_counts":
                        whole = torch.full((n + 2, 4), GUARD32, dtype=torch.int32, device=dev)
                        ctx.sample_counts(d_bits, wps, m, out=whole[1:n + 1], stream=stream)
                        later(stream, whole, 1, n + 1, e["counts"], "sample counts", GUARD32)
                    elif kind == "compact_sites":
                        words = cuking_amd.site_mask_words(e["keep"])
                        want, want_wps, want_kept = cuking_amd.compact_sites_host(bits, wps, words, m)
                        same(want, e["bits"], "compact_sites_host against pack(geno[:, keep])")
                        if call["guarded"]:
                            whole = torch.full((n + 2, want_wps), GUARD64, dtype=torch.int64,
                                               device=dev)
                            _, got_wps, kept = ctx.compact_sites(d_bits, wps, words, m,
                                                                 out=whole[1:n + 1], stream=stream)
                            later(stream, whole, 1, n + 1, e["bits"], "compacted bits", GUARD64)
                        else:
                            out, got_wps, kept = ctx.compact_sites(d_bits, wps, words, m,
                                                                   stream=stream)
                            later(stream, out, 0, n, e["bits"], "compacted bits", GUARD64)
                        if (got_wps, kept) != (want_wps, want_kept):
                            fail(f"words_per_sample, kept {(got_wps, kept)}")
                    elif kind == "filter_sites":
                        args = (call["min_call_rate"], call["min_maf"], call["min_mac"], e["also"])
                        words, _ = cuking_amd.site_mask_host(pc.site_counts_numpy(geno, wps // 2),
                                                             m, *args)
                        same(cuking_amd.site_mask_bool(words, m), e["keep"],
                             "site_mask_host against rule_numpy")
                        try:
                            qc = ctx.filter_sites(d_bits, wps, m, *args, stream=stream)
                        except cuking_amd.CukingError as err:
                            if not (e["fails"] and "no site passes" in str(err)):
                                fail(f"raised {err}")
                        else:
                            if e["fails"]:
                                fail("no site passes, but no error")
                            same(qc.keep(), e["keep"], "kept sites")
                            same(qc.counts(), e["counts"], "site counts")
                            if (qc.num_sites, qc.words_per_sample) != \
                                    (int(e["keep"].sum()), e["bits"].shape[1]):
                                fail(f"num_sites, words_per_sample "
                                     f"{(qc.num_sites, qc.words_per_sample)}")
                            later(stream, qc.bits, 0, n, e["bits"], "filtered bits", GUARD64)
                            result = dict(bits=qc.bits, wps=qc.words_per_sample, stream=stream)
                    elif kind == "transpose_sites":
                        same(cuking_amd.transpose_sites_host(bits, wps, m), e["site_bits"],
                             "transpose_sites_host against site_bits_numpy")
                        whole = torch.full((m + 2, 2, q), GUARD64, dtype=torch.int64, device=dev)
                        ctx.transpose_sites(d_bits, wps, m, out=whole[1:m + 1], stream=stream)
                        later(stream, whole, 1, m + 1, e["site_bits"], "site-major bits", GUARD64)
                    elif kind == "ld_edges":
                        want, count = cuking_amd.ld_edges_host(transposed(), m, n, call["window"],
                                                               call["r2"], group=e["group"])
                        same(want, e["edges"], "ld_edges_host against ld_edges_fast")
                        site_bits = ctx.transpose_sites(d_bits, wps, m, stream=stream)
                        group = None if e["group"] is None else \
                            torch.from_numpy(e["group"]).to(dev)
                        kw = dict(window=call["window"], r2=call["r2"], group=group, stream=stream)
                        if e["room"] is None:
                            records, got = ctx.ld_edges(site_bits, m, n, **kw)
                            if got != count:
                                fail(f"{got} edges, not {count}")
                            same(host_records(records, got), e["edges"], "edges")
                            edges = (records, got)
                        else:
                            room = e["room"]
                            whole = torch.full((room + 8, 6), GUARD32, dtype=torch.int32,
                                               device=dev)
                            try:
                                _, got = ctx.ld_edges(site_bits, m, n, out=whole[:room], **kw)
                            except cuking_amd.ResourceExhaustedError as err:
                                if not e["exhausted"] or err.num_records != count:
                                    fail(f"ResourceExhaustedError, num_records {err.num_records}, "
                                         f"{count} edges, room {room}")
                                got = room
                            else:
                                if e["exhausted"] or got != count:
                                    fail(f"{got} edges in a buffer of {room}, not {count}")
                            host = whole.cpu().numpy()
                            if not (host[room:] == GUARD32).all():
                                fail("guard records were written")
                            stored = host_records(whole, got)
                            if e["exhausted"]:
                                have = {r.tobytes() for r in stored}
                                if len(have) != room or not have <= {r.tobytes() for r in e["edges"]}:
                                    fail("the stored records are no subset of the edges")
                                edges = None
                            else:
                                same(stored, e["edges"], "edges")
                                edges = (whole[:room], got)
                    elif kind == "ld_prune":
                        keep, _ = api.unrelated_set_host(e["edges"], m, priority=e["used"],
                                                         families=False)
                        same(keep == 1, e["keep"], "unrelated_set_host against greedy_numpy")
                        priority = e["priority"]
                        if priority is not None and call["place"] == "device":
                            priority = torch.from_numpy(priority).to(dev)
                        got = ctx.ld_prune(d_bits, wps, m, window=call["window"], r2=call["r2"],
                                           group=e["group"], priority=priority,
                                           compact=call["compact"])
                        if got.num_edges != len(e["edges"]):
                            fail(f"{got.num_edges} edges, not {len(e['edges'])}")
                        same(got.edges(), e["edges"], "edges")
                        same(got.keep(), e["keep"], "kept sites")
                        if e["bits"] is None:
                            if got.bits is not d_bits or (got.words_per_sample, got.num_sites) != \
                                    (wps, m):
                                fail("the input bits were to come back")
                        else:
                            if (got.num_sites, got.words_per_sample) != \
                                    (int(e["keep"].sum()), e["bits"].shape[1]):
                                fail(f"num_sites, words_per_sample "
                                     f"{(got.num_sites, got.words_per_sample)}")
                            later(stream, got.bits, 0, n, e["bits"], "pruned bits", GUARD64)
                        result = dict(bits=got.bits, wps=got.words_per_sample, stream=stream)
                    elif kind in ("unrelated_set", "prune"):
                        keep, family = api.unrelated_set_host(e["records"], e["count"], e["thr"],
                                                              priority=e["priority"])
                        same(keep, e["keep"], "unrelated_set_host's keep against the yardstick")
                        same(family, e["family"], "unrelated_set_host's family")
                        priority = None if e["priority"] is None else \
                            torch.from_numpy(e["priority"]).to(dev)
                        if kind == "prune":
                            got = ctx.prune(cuking_amd.Submatrix(n), wps, d_bits, e["thr"],
                                            priority=priority, families=call["families"])
                        else:
                            if e["source"] == "edges" and edges is not None and \
                                    edges[1] == len(e["records"]):
                                records = edges[0]      # where ld_edges left them
                            else:
                                records = device_records(e["records"],
                                                         np.random.default_rng(call["seed"]))
                            got = ctx.unrelated_set(records, len(e["records"]), e["count"], e["thr"],
                                                    priority=priority, families=call["families"],
                                                    stream=stream)
                        same(got.keep.cpu().numpy(), e["keep"], "keep")
                        if call["families"]:
                            same(got.family.cpu().numpy().view(np.uint32), e["family"], "family")
                        elif got.family is not None:
                            fail("families=False returned a family vector")
                    elif kind == "pair":
                        if result["stream"] is not None:
                            stream.wait_stream(result["stream"])
                        sm = cuking_amd.Submatrix(n)
                        ctx.invalidate()
                        if call["call"] == "run":
                            got = ctx.run(sm, result["wps"], result["bits"], call["thr"])
                            if got.tobytes() != e["records"].tobytes():
                                fail(_diff(got, e["records"]))
                        else:
                            out = ctx.kin_matrix(sm, result["wps"], result["bits"], symmetric=True,
                                                 stream=stream)
                            stream.synchronize()
                            try:
                                import reducing_cases
                                reducing_cases.assert_same(out.cpu().numpy(), e["matrix"],
                                                           "kin_matrix")
                            except AssertionError as err:
                                fail(str(err))
            for check in pending:
                check()
            torch.cuda.synchronize()
            ran += 1
            if log and tag["case"] % 10 == 0:
                log(f"run_pipeline seed {seed} case {tag['case']} ok ({time.time() - t0:.0f}s)")
    finally:
        ctx.set_option("max_launch_blocks", 0)
        ctx.invalidate()
    return ran


def run_split(ctx, seed: int, cases: int, first_case: int = 0, log=None) -> int:
    """The matrix-core variants' remainder splitting (king_mfma.hip): blocks large
    enough that pieces of k-steps, scratch slabs and tickets are really exercised
    -- whole blocks, tile sub-ranges and staged rectangles on several streams at
    once (tools/fuzz_split.py)."""
    import torch
    import cuking_amd
    from cuking_amd.dist import tile_partition
    from cuking_amd.synth import cohort_to_device, plan_cohort
    from oracle import pyoracle

    rng = np.random.default_rng(seed)
    matrix_variants = [v for v in range(ctx.lib.cuking_num_variants())
                       if "mfma" in ctx.variant_name(v)]
    ctx.set_kernel("tiled")
    t0, ran = time.time(), 0
    for case in range(cases):
        n = int(rng.integers(130, 3000))
        m = int(rng.integers(3000, 40000))
        thr = float(rng.choice([0.03, 0.0884, 0.3]))
        mode = int(rng.choice([-1, -1, 0, 1]))
        wgs = int(rng.choice([3, 16, 64, 256, 256]))
        w = int(rng.integers(2, 6))
        world = int(rng.integers(1, 5))
        chunks = int(rng.integers(1, 6))
        streams = [int(rng.integers(1, 4)) for _ in range(world)]
        variant = int(rng.choice(matrix_variants))
        if case < first_case:
            continue
        tag = dict(fuzzer="run_split", seed=seed, case=case, n=n, m=m, thr=thr, counts_mode=mode,
                   split_wgs=wgs, variant=variant)
        ctx.set_option("variant", variant)
        ctx.set_option("split_wgs", wgs)
        ctx.set_option("counts_mode", mode)
        ctx.invalidate()
        cohort = plan_cohort(n, seed * 1000 + case)
        kind, pa, pb = cohort_to_device(cohort, ctx.device)
        wps = cuking_amd.words_per_sample(m)
        d_bits = torch.zeros((n, wps), dtype=torch.int64, device=f"cuda:{ctx.device}")
        ctx.synth_bitset(seed * 1000 + case, kind, pa, pb, 0, n, m, out=d_bits)
        torch.cuda.synchronize()
        bits = np.ascontiguousarray(d_bits.cpu().numpy().view(np.uint64))
        exp, _, _ = pyoracle.compute(pyoracle.submatrix(n), bits, thr, threads=16)
        sm = cuking_amd.Submatrix(n)
        for rep in range(2):
            got = ctx.run(sm, wps, d_bits, thr)
            if got.tobytes() != exp.tobytes():
                raise FuzzMismatch(f"run (rep {rep}): {_diff(got, exp)}; reproduce with {tag}")
        tiles = ctx.num_tiles(sm)
        parts = [ctx.run(sm, wps, d_bits, thr, tile_range=r) for r in tile_partition(tiles, w)]
        merged = cuking_amd.sort_results(np.ascontiguousarray(np.concatenate(parts)))
        if merged.tobytes() != exp.tobytes():
            raise FuzzMismatch(f"tile ranges ({w}): {_diff(merged, exp)}; reproduce with {tag}")
        merged = _staged(ctx, sm, wps, d_bits, thr, max(len(exp), 1) + 8, n, world, chunks, streams)
        if merged.tobytes() != exp.tobytes():
            raise FuzzMismatch(f"staged (world {world}, chunks {chunks}, streams {streams}): "
                               f"{_diff(merged, exp)}; reproduce with {tag}")
        ran += 1
        if log and case % 5 == 0:
            log(f"run_split seed {seed} case {case} ok, {len(exp)} records ({time.time() - t0:.0f}s)")
    return ran


def run_stress(ctx, reps: int, thr: float = 0.03, log=None):
    """One staged configuration repeated `reps` times per (form, split, streams)
    combination of every matrix-core variant: rare, timing-dependent failures
    (tools/stress_split.py).  Returns [(label, wrong, reps), ...]."""
    import torch
    import cuking_amd
    from cuking_amd.synth import cohort_to_device, plan_cohort
    from oracle import pyoracle

    ctx.set_kernel("tiled")
    n, m, chunks = 1015, 33744, 3
    cohort = plan_cohort(n, 4242)
    kind, pa, pb = cohort_to_device(cohort, ctx.device)
    wps = cuking_amd.words_per_sample(m)
    d_bits = torch.zeros((n, wps), dtype=torch.int64, device=f"cuda:{ctx.device}")
    ctx.synth_bitset(4242, kind, pa, pb, 0, n, m, out=d_bits)
    torch.cuda.synchronize()
    bits = np.ascontiguousarray(d_bits.cpu().numpy().view(np.uint64))
    exp, _, _ = pyoracle.compute(pyoracle.submatrix(n), bits, thr, threads=16)
    sm = cuking_amd.Submatrix(n)
    matrix_variants = [v for v in range(ctx.lib.cuking_num_variants())
                       if "mfma" in ctx.variant_name(v)]
    out = []
    for variant, mode, wgs, streams in itertools.product(matrix_variants, (1, 0), (16, 0, 256),
                                                         (1, 3)):
        ctx.set_option("variant", variant)
        ctx.set_option("counts_mode", mode)
        ctx.set_option("split_wgs", wgs)
        ctx.invalidate()
        bad, first = 0, ""
        for _ in range(reps):
            got = _staged(ctx, sm, wps, d_bits, thr, len(exp) + 8, n, 1, chunks, [streams])
            if got.tobytes() != exp.tobytes():
                bad += 1
                first = first or _diff(got, exp)
        label = (f"variant {ctx.variant_name(variant)} form {'full' if mode else 'lean'} "
                 f"split_wgs {wgs} streams {streams}")
        out.append((label, bad, reps, first))
        if log:
            log(f"run_stress {label}: {bad} of {reps} wrong {first}")
    return out
