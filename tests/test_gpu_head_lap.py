"""The head lap of the filter kernel on a site-ordered layout (king_filter.hip plan_checks):
a tile rotates inside the head of the order and is checked after one lap of it.  Its sums at
the check are over exactly the head's sites -- exact integers, whatever the order -- so against
the unrotated tile ("filter_site_order" 1 at "filter_rotate" 0) the lap ("filter_site_order" 2)
must give the same tiles that leave, the same candidates and the same records: counters EQUAL,
records byte-identical to each other and to the oracle.

The launches here are a round or two long, where "filter_check0" 1 adds the forecast check for
bitsets this short -- and a launch with a forecast check takes no lap.  The tests switch the
forecast off, so that the lap they are about runs, and say so where they assert it."""
import numpy as np
import pytest

import cuking_amd
from cuking_amd.synth import cohort_to_device, plan_cohort
from conftest import random_genotypes

pytestmark = pytest.mark.gpu

THR = 0.0884
RESTORE = (("filter_site_order", -1), ("filter_check_min_steps", 64), ("filter_rotate", 1),
           ("filter_rotate_min_steps", 128), ("filter_rotate_min_tiles", 2048),
           ("filter_sort", 1), ("filter_check0", 1), ("split_wgs", 256), ("counts_mode", -1))
COUNTERS = ("filter_early_exits", "filter_candidates", "filter_dense_quadrants",
            "filter_rotated_tiles")
HOOKS = (2, 3 + 1, 3 + 77, 3 + 127)      # (3 + 127: a phase outside any head, reduced)


def plant(geno):
    """A duplicate, a parent-child-like and a sibling-like pair across tile boundaries."""
    n = geno.shape[0]
    geno[n - 1] = geno[3]
    half = geno.shape[1] // 2
    geno[n // 2, :half] = geno[5, :half]
    geno[n - 7, ::2] = geno[260 % n, ::2]
    return geno


def staying_tiles(rng):
    """1,280 samples (5 tile rows, 15 tiles) x 20,480 sites, stored sample order.  In every third
    off-diagonal tile nine row samples and nine column samples are sibling-like to one founder
    each way (every other site shared): 81 live pairs in one quadrant, more than a tile may
    hand over at the check, so those tiles go on into the tail.  Returns the genotypes and the
    planted (row sample, column sample) pairs."""
    geno = random_genotypes(rng, 1280, 20480, missing=0.01)
    pairs, k = [], 0
    tiles = [(tr, tc) for tr in range(5) for tc in range(tr + 1, 5)]
    for t, (tr, tc) in enumerate(tiles):
        if t % 3:
            continue
        rows = [256 * tr + 9 * k + i for i in range(9)]
        cols = [256 * tc + 9 * k + i for i in range(9)]
        founder = geno[rows[0]].copy()
        for s in rows[1:] + cols:
            geno[s, ::2] = founder[::2]
        pairs += [(r, c) for r in rows for c in cols]
        k += 1
    return geno, pairs


def cases():
    rng = np.random.default_rng(2011)
    out = {}
    # 80 k-steps: a check exists and tiles leave
    out["1100x20480"] = plant(random_genotypes(rng, 1100, 20480, missing=0.01))
    # neither a multiple of 256 samples nor of 256 sites, the last word padded; 12 k-steps: too
    # short for a lap under the default rotate_min_steps, long enough with 4
    out["600x3000"] = plant(random_genotypes(rng, 600, 3000, missing=0.01))
    # ties and a zero-weight tail: the head can be the whole informative part
    g = random_genotypes(rng, 700, 8192, missing=0.01)
    mono = rng.random(8192) < 0.3
    g[:, mono] = np.where(g[:, mono] < 0, -1, 0)
    out["700x8192_monomorphic"] = plant(g)
    out["staying_tiles"], out["staying_pairs"] = staying_tiles(rng)
    return out


@pytest.fixture(scope="module")
def material(oracle):
    """Bitsets and the oracle's records, computed once."""
    c, out = cases(), {}
    for name in ("1100x20480", "600x3000", "700x8192_monomorphic", "staying_tiles"):
        bits = oracle.bitset_from_genotypes(c[name])
        exp, _, _ = oracle.compute(oracle.submatrix(c[name].shape[0]), bits, THR, threads=16)
        assert len(exp) >= 2, name
        out[name] = (bits, exp)
    out["staying_pairs"] = c["staying_pairs"]
    return out


def prepare_ctx(ctx):
    ctx.set_kernel("tiled")
    ctx.set_option("variant", 7)
    ctx.set_option("counts_mode", 0)
    ctx.set_option("filter_check_min_steps", 4)
    ctx.set_option("filter_rotate_min_steps", 4)
    ctx.set_option("filter_rotate_min_tiles", 0)
    ctx.set_option("filter_check0", 0)  # (a launch with a forecast check takes no lap)
    ctx.set_option("split_wgs", 0)      # whole tiles only: remainder pieces have no check points


def restore(ctx):
    for k, v in RESTORE:
        ctx.set_option(k, v)


def run_counted(ctx, sm, sites, d_bits, order, rotate):
    """One call; the records and what the counters moved by."""
    ctx.set_option("filter_site_order", order)
    ctx.set_option("filter_rotate", rotate)
    before = [ctx.get_option(k) for k in COUNTERS]
    got = ctx.run(sm, sites, d_bits, THR, max_results=1 << 20)
    return got, dict(zip(COUNTERS, (ctx.get_option(k) - b for k, b in zip(COUNTERS, before))))


def same_work(a, b):
    return all(a[k] == b[k] for k in COUNTERS[:3])


@pytest.mark.parametrize("name", ["1100x20480", "600x3000", "700x8192_monomorphic"])
def test_lap_equals_the_unrotated_tile_at_every_hook_phase(ctx, material, name):
    bits, exp = material[name]
    sm = cuking_amd.Submatrix(bits.shape[0])
    d_bits = ctx.upload_bitset(bits)
    prepare_ctx(ctx)
    try:
        flat, want = run_counted(ctx, sm, bits.shape[1], d_bits, 1, 0)
        assert flat.tobytes() == exp.tobytes(), name
        assert want["filter_rotated_tiles"] == 0
        if name == "1100x20480":
            assert want["filter_early_exits"] > 0
        for rotate in HOOKS:
            lap, got = run_counted(ctx, sm, bits.shape[1], d_bits, 2, rotate)
            print(name, rotate, want, got)
            assert lap.tobytes() == exp.tobytes(), (name, rotate)
            assert same_work(got, want), (name, rotate, got, want)
            if name != "600x3000" and rotate != 3 + 127:
                assert got["filter_rotated_tiles"] > 0, (name, rotate)   # the lap ran
        if name == "600x3000":
            # the default rotate_min_steps: no lap, the same records
            ctx.set_option("filter_rotate_min_steps", 128)
            short, got = run_counted(ctx, sm, bits.shape[1], d_bits, 2, 3 + 77)
            assert short.tobytes() == exp.tobytes()
            assert got["filter_rotated_tiles"] == 0 and same_work(got, want)
    finally:
        restore(ctx)


def test_tiles_that_stay_run_the_tail_behind_the_lap(ctx, material):
    bits, exp = material["staying_tiles"]
    # the planted pairs are above the threshold: the oracle's records hold every one
    found = set(zip(exp["sample_i"].tolist(), exp["sample_j"].tolist()))
    assert all(p in found for p in material["staying_pairs"])
    sm = cuking_amd.Submatrix(bits.shape[0])
    d_bits = ctx.upload_bitset(bits)
    prepare_ctx(ctx)
    try:
        ctx.set_option("filter_sort", 0)          # tiles of the stored sample order
        tiles = ctx.num_tiles(sm)
        flat, want = run_counted(ctx, sm, bits.shape[1], d_bits, 1, 0)
        assert flat.tobytes() == exp.tobytes()
        assert 0 < want["filter_early_exits"] < tiles
        for rotate in (2, 3 + 77):
            lap, got = run_counted(ctx, sm, bits.shape[1], d_bits, 2, rotate)
            print(rotate, tiles, want, got)
            assert lap.tobytes() == exp.tobytes(), rotate
            assert same_work(got, want), (rotate, got, want)
            assert got["filter_rotated_tiles"] > 0
    finally:
        restore(ctx)


def test_the_real_path_joins_the_position_of_the_xcd(ctx, oracle):
    """6,400 samples x 8,192 sites: 325 tiles of 32 k-steps, more than one per CU, so later
    tiles join the position the tiles of their XCD have published -- inside the head."""
    import torch
    n, m, seed = 6400, 8192, 23
    cohort = plan_cohort(n, seed)
    kind, pa, pb = cohort_to_device(cohort)
    d_bits = ctx.synth_bitset(seed, kind, pa, pb, 0, n, m)
    torch.cuda.synchronize()
    host = d_bits.cpu().numpy().view(np.uint64)
    exp, _, _ = oracle.compute(oracle.submatrix(n), host, THR, threads=16)
    sm = cuking_amd.Submatrix(n)
    prepare_ctx(ctx)
    try:
        assert ctx.num_tiles(sm) == 325
        flat, want = run_counted(ctx, sm, d_bits.shape[1], d_bits, 1, 1)
        lap, got = run_counted(ctx, sm, d_bits.shape[1], d_bits, 2, 1)
        print(want, got)
        assert flat.tobytes() == exp.tobytes() and lap.tobytes() == exp.tobytes()
        assert want["filter_rotated_tiles"] == 0 and want["filter_early_exits"] > 0
        assert same_work(got, want), (got, want)
        assert got["filter_rotated_tiles"] > 0
    finally:
        restore(ctx)
