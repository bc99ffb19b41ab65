"""Site order of the filter variant's kernel layout ("filter_site_order", king_sort.hip):
the sites sorted by the X they contribute to unrelated pairs, the check share taken from
the cohort's measured curve.  Records must not depend on it: byte-identical to stored order
and to the oracle."""
import numpy as np
import pytest

import cuking_amd
from cuking_amd.synth import cohort_to_device, plan_cohort
from conftest import random_genotypes

pytestmark = pytest.mark.gpu

RESTORE = (("filter_site_order", -1), ("filter_site_order_min_tiles", 24576), ("filter_check_min_steps", 64), ("filter_rotate", 1),
           ("filter_rotate_min_steps", 128), ("filter_rotate_min_tiles", 2048),
           ("reuse_prepared", 0), ("split_wgs", 256), ("counts_mode", -1))


def plant(geno):
    """A duplicate, a parent-child-like and a sibling-like pair across tile boundaries."""
    n = geno.shape[0]
    geno[n - 1] = geno[3]
    half = geno.shape[1] // 2
    geno[n // 2, :half] = geno[5, :half]
    geno[n - 7, ::2] = geno[260 % n, ::2]
    return geno


def cases():
    rng = np.random.default_rng(1811)
    out = {}
    # neither a multiple of 256 samples nor of 256 sites, the last word padded
    out["600x3000"] = (plant(random_genotypes(rng, 600, 3000, missing=0.01)), 0.0884)
    # 80 k-steps: a check point exists and tiles leave
    out["1100x20480"] = (plant(random_genotypes(rng, 1100, 20480, missing=0.01)), 0.0884)
    # ties and zero-weight sites: the stable tail
    g = random_genotypes(rng, 700, 8192, missing=0.01)
    mono = rng.random(8192) < 0.3
    g[:, mono] = np.where(g[:, mono] < 0, -1, 0)
    out["700x8192_monomorphic"] = (plant(g), 0.0884)
    return out


@pytest.fixture(scope="module")
def material(oracle):
    """Bitsets and the oracle's records, computed once."""
    out = {}
    for name, (geno, thr) in cases().items():
        bits = oracle.bitset_from_genotypes(geno)
        exp, _, _ = oracle.compute(oracle.submatrix(geno.shape[0]), bits, thr, threads=16)
        assert len(exp) >= 2, name
        out[name] = (bits, thr, exp)
    return out


def prepare_ctx(ctx):
    ctx.set_kernel("tiled")
    ctx.set_option("variant", 7)
    ctx.set_option("counts_mode", 0)
    ctx.set_option("filter_check_min_steps", 4)
    ctx.set_option("filter_rotate_min_steps", 4)
    ctx.set_option("filter_rotate_min_tiles", 0)
    ctx.set_option("split_wgs", 0)      # whole tiles only: remainder pieces have no check points


def restore(ctx):
    for k, v in RESTORE:
        ctx.set_option(k, v)


@pytest.mark.parametrize("name", ["600x3000", "1100x20480", "700x8192_monomorphic"])
def test_site_order_records_match_stored_order_and_oracle(ctx, material, name):
    """Order on against order off against the oracle, unrotated and with the rotation's test
    hooks (a phase per tile; one fixed phase: the wrap-around with the order on)."""
    bits, thr, exp = material[name]
    n = bits.shape[0]
    sm = cuking_amd.Submatrix(n)
    d_bits = ctx.upload_bitset(bits)
    prepare_ctx(ctx)
    try:
        for rotate in (0, 2, 3 + 77):
            ctx.set_option("filter_rotate", rotate)
            got = {}
            for order in (0, 1):
                ctx.set_option("filter_site_order", order)
                x0 = ctx.get_option("filter_early_exits")
                got[order] = ctx.run(sm, bits.shape[1], d_bits, thr, max_results=1 << 20)
                exits = ctx.get_option("filter_early_exits") - x0
                # (with the order on also under the hooks: the share of a range that starts
                #  at another phase and goes around the end must still be a check)
                if name == "1100x20480" and (rotate == 0 or order == 1):
                    assert exits > 0, (order, rotate, exits)
            assert got[1].tobytes() == got[0].tobytes(), (name, rotate)
            assert got[1].tobytes() == exp.tobytes(), (name, rotate)
    finally:
        restore(ctx)


def test_site_order_exome_model(ctx, oracle):
    """520 x 4,160 of the generator's exome-like spectrum at threshold 0.05."""
    n, m, seed, thr = 520, 4160, 11, 0.05
    cohort = plan_cohort(n, seed)
    kind, pa, pb = cohort_to_device(cohort)
    d_bits = ctx.synth_bitset(seed, kind, pa, pb, 0, n, m, model="exome")
    import torch
    torch.cuda.synchronize()
    host = d_bits.cpu().numpy().view(np.uint64)
    exp, _, _ = oracle.compute(oracle.submatrix(n), host, thr, threads=16)
    sm = cuking_amd.Submatrix(n)
    prepare_ctx(ctx)
    try:
        for rotate in (0, 1, 2):               # (2: the hook, a phase per tile)
            ctx.set_option("filter_rotate", rotate)
            for order in (0, 1, 2):            # (2: the order with rotated tiles kept)
                ctx.set_option("filter_site_order", order)
                got = ctx.run(sm, d_bits.shape[1], d_bits, thr, max_results=1 << 20)
                assert got.tobytes() == exp.tobytes(), (rotate, order)
                assert ctx.get_option("site_order_on") == int(order != 0), (rotate, order)
    finally:
        restore(ctx)


def test_site_order_tile_ranges_and_option_flips(ctx, material):
    """Two tile ranges of one block give the one-call records (every chunk of a block sees
    the same order), and flipping the option between calls with reuse_prepared = 1 converts
    again each time and returns the same records."""
    bits, thr, exp = material["1100x20480"]
    n = bits.shape[0]
    sm = cuking_amd.Submatrix(n)
    d_bits = ctx.upload_bitset(bits)
    prepare_ctx(ctx)
    try:
        ctx.set_option("filter_site_order", 1)
        tiles = ctx.num_tiles(sm)
        cut = tiles // 2 + 1
        parts = [ctx.run(sm, bits.shape[1], d_bits, thr, max_results=1 << 20, tile_range=r)
                 for r in ((0, cut), (cut, tiles))]
        union = cuking_amd.sort_results(np.concatenate(parts))
        assert union.tobytes() == exp.tobytes()
        ctx.set_option("reuse_prepared", 1)
        ctx.invalidate()
        for order in (1, 0, 1, -1):
            skipped = ctx.get_option("conversions_skipped")
            ctx.set_option("filter_site_order", order)
            got = ctx.run(sm, bits.shape[1], d_bits, thr, max_results=1 << 20)
            assert got.tobytes() == exp.tobytes(), order
            assert ctx.get_option("conversions_skipped") == skipped, order
        # (the same value again: the layout is reused)
        got = ctx.run(sm, bits.shape[1], d_bits, thr, max_results=1 << 20)
        assert got.tobytes() == exp.tobytes()
        assert ctx.get_option("conversions_skipped") == skipped + 1
    finally:
        restore(ctx)


NUM_PHASES = 128                 # king_common.h kNumPhases


def replay(geno, thr):
    """numpy: weight, stable descending order, curve, sigma and the two shares of
    site_order_forecast (king_sort.hip) for genotypes whose sites fill whole k-steps."""
    n, m = geno.shape
    assert m % 256 == 0
    r, h, a, mis = ((geno == k).sum(axis=0).astype(np.int64) for k in (0, 1, 2, -1))
    w = r * h + h * a + 4 * r * a
    ws = w[np.argsort(-w, kind="stable")]
    steps = m // 256
    run = np.concatenate([[0], np.cumsum(ws)])
    cum = run[[256 * (steps * (x + 1) // NUM_PHASES) for x in range(NUM_PHASES)]]
    pairs = 0.5 * n * (n - 1)
    p1, p4 = (r * h + h * a) / pairs, r * a / pairs
    sigma = np.sqrt((p1 + 16 * p4 - (p1 + 4 * p4) ** 2).sum()) / (4 * (h / n).sum())
    mr, hr = mis.sum() / (n * m), h.sum() / (n * m)
    mean = mr * (1 + mr / (2 * hr * (1 - mr)))

    def shares(tilt):
        k_lin, k_ord = mean + 4.6 / np.sqrt(m) + 0.003, mean + 4.6 * sigma + 0.003
        f64 = 64 * (1 - 2 * thr) / (1 - 2 * k_lin) * tilt
        stored = (max(int(np.ceil(f64)), 32) if f64 <= 62 else 0) if k_lin < 0.5 else 0
        need = (1 - 2 * thr) / (1 - 2 * k_ord) * tilt
        order = next((s for s in range(32, 63) if cum[2 * s - 1] >= need * cum[-1]), 0) \
            if k_ord < 0.5 else 0
        return stored, order
    # (the library's float32 arithmetic: a few 1e-7 relative per step, 1e-5 covers a chain)
    return sigma, shares(1 - 1e-5), shares(1 + 1e-5)


def test_device_curve_share_and_automatic_rule_match_numpy(ctx):
    """The device's counts, sort, curve and sigma, read back through the forecast: the
    shares and sigma equal the numpy replay's, and the automatic rule takes the order exactly
    when the replay's curve share is at least 2/64 under stored order's -- on a cohort whose
    allele frequencies spread (it does) and on one where every site weighs the same and 3 %
    of the calls are missing (it does not: nothing to sort)."""
    thr = 0.0884
    prepare_ctx(ctx)
    try:
        ctx.set_option("filter_site_order_min_tiles", 0)
        seen = set()
        # (the second: 61/64 against 60/64 in the replay, one 64th is not worth a conversion)
        for lo, hi, missing in ((0.05, 0.5, 0.01), (0.5, 0.5, 0.03)):
            rng = np.random.default_rng(1812)
            geno = random_genotypes(rng, 1100, 20480, missing=missing, af_lo=lo, af_hi=hi)
            sigma, low, high = replay(geno, thr)
            assert low == high, "a share on a rounding edge: take another seed"
            stored, order = low
            import oracle.pyoracle as po
            bits = po.bitset_from_genotypes(geno)
            d_bits = ctx.upload_bitset(bits)
            sm = cuking_amd.Submatrix(1100)
            got = {}
            for opt in (1, -1, 0):
                ctx.set_option("filter_site_order", opt)
                got[opt] = ctx.run(sm, bits.shape[1], d_bits, thr, max_results=1 << 20)
                if opt == 0:
                    assert ctx.get_option("site_order_on") == 0
                    continue
                assert ctx.get_option("site_order_share") == order, (lo, opt)
                assert ctx.get_option("site_order_stored_share") == stored, (lo, opt)
                # (read back in millionths of a float32)
                assert abs(ctx.get_option("site_order_sigma_e6") - 1e6 * sigma) <= 1 + 1e-5 * 1e6 * sigma
                want = 1 if opt == 1 else int(order != 0 and (stored == 0 or order + 2 <= stored))
                assert ctx.get_option("site_order_on") == want, (lo, opt, stored, order)
                if opt == -1:
                    seen.add(want)
                    # a "no" is remembered for the block: the next conversion neither builds
                    # the curve nor waits for it; a "yes" builds it every time
                    syncs = ctx.get_option("host_syncs")
                    again = ctx.run(sm, bits.shape[1], d_bits, thr, max_results=1 << 20)
                    assert again.tobytes() == got[-1].tobytes()
                    assert ctx.get_option("host_syncs") - syncs == want, (lo, want)
                    assert ctx.get_option("site_order_on") == want
            assert got[1].tobytes() == got[0].tobytes() == got[-1].tobytes()
        assert seen == {0, 1}
    finally:
        restore(ctx)
