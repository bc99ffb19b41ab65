"""The gather of the site order ("filter_site_gather", king_sort.hip gather_sites_kernel): a
workgroup stages 4 or 2 samples in LDS with a byte or a nibble per site and assembles the
output words by bit-matrix transposes.  Every form must write the bytes of the earlier ballot
kernel -- here against a numpy gather of the same bitset --, and the records of a call must not
depend on the form."""
import ctypes as C

import numpy as np
import pytest

import cuking_amd
from cuking_amd.api import check
from conftest import random_genotypes

pytestmark = pytest.mark.gpu

THR = 0.0884
SAMPLES = (1, 2, 3, 5, 9)            # remainders of both G; 9 = 2 * 4 + 1: a group of repeats but one
WORDS_PER_SAMPLE = (2, 6, 14, 130, 640, 15)   # planes of 1, 3, 7, 65, 320 words; 15: one word behind
ORDERS = ("identity", "reversal", "random", "sorted weights")
SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)
RESTORE = (("filter_site_gather", -1), ("filter_site_order", -1),
           ("filter_site_order_min_tiles", 24576), ("filter_check_min_steps", 64),
           ("filter_rotate_min_steps", 128), ("filter_rotate_min_tiles", 2048),
           ("filter_check0", 1), ("split_wgs", 256), ("counts_mode", -1))
COUNTERS = ("filter_candidates", "filter_early_exits", "filter_dense_quadrants")


def make_order(kind, sites, rng):
    order = np.arange(sites, dtype=np.uint32)
    if kind == "reversal":
        order = order[::-1].copy()
    elif kind == "random":
        order = rng.permutation(sites).astype(np.uint32)
    elif kind == "sorted weights":
        # a descending stable sort of weights with many ties; the padding sites of the last
        # word weigh nothing and land behind them
        weight = rng.integers(0, 5, sites)
        weight[sites - 37:] = 0
        order = np.argsort(-weight, kind="stable").astype(np.uint32)
    return order


def numpy_gather(bits, order):
    """out[s][plane] bit d = bits[s][plane] bit order[d]; a word behind the planes: SENTINEL."""
    n, wps = bits.shape
    p = wps // 2
    out = np.full((n, wps), SENTINEL, dtype=np.uint64)
    for plane in range(2):
        words = np.ascontiguousarray(bits[:, plane * p:(plane + 1) * p])
        sites = np.unpackbits(words.view(np.uint8).reshape(n, p * 8), axis=1, bitorder="little")
        packed = np.ascontiguousarray(np.packbits(sites[:, order], axis=1, bitorder="little"))
        out[:, plane * p:(plane + 1) * p] = packed.view(np.uint64).reshape(n, p)
    return out


@pytest.fixture(scope="module")
def shapes():
    """Bitsets, orders and the numpy gather of each, computed once."""
    rng = np.random.default_rng(2101)
    out = []
    for n in SAMPLES:
        for wps in WORDS_PER_SAMPLE:
            bits = rng.integers(0, 1 << 63, (n, wps), dtype=np.uint64) << np.uint64(1) | \
                rng.integers(0, 2, (n, wps), dtype=np.uint64)
            for kind in ORDERS:
                order = make_order(kind, 64 * (wps // 2), rng)
                out.append((n, wps, kind, bits, order, numpy_gather(bits, order)))
    return out


def run_gather(ctx, bits, order, gather, stats=0):
    """cuking_test_site_gather on a sentinel-filled copy and a sentinel-filled statistics
    region: (the copy, the region's bytes, its layout)."""
    import torch
    n, wps = bits.shape
    d_bits = ctx.upload_bitset(bits)
    d_order = torch.from_numpy(order.view(np.int32)).to(d_bits.device)
    d_out = torch.from_numpy(np.full((n, wps), SENTINEL, dtype=np.uint64).view(np.int64)) \
        .to(d_bits.device)
    layout = (C.c_uint64 * 5)()
    stream = int(torch.cuda.current_stream().cuda_stream)
    # (the layout first: a call without statistics fills it)
    check(ctx.lib.cuking_test_site_gather(ctx.handle, d_bits.data_ptr(), n, wps,
                                          d_order.data_ptr(), gather, d_out.data_ptr(), 0, None,
                                          0, layout, stream))
    region = None
    if stats:
        d_stats = torch.full((int(layout[4]),), 0xA5, dtype=torch.uint8, device=d_bits.device)
        check(ctx.lib.cuking_test_site_gather(ctx.handle, d_bits.data_ptr(), n, wps,
                                              d_order.data_ptr(), gather, d_out.data_ptr(), stats,
                                              d_stats.data_ptr(), int(layout[4]), layout, stream))
        torch.cuda.synchronize()
        region = d_stats.cpu().numpy()
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(np.uint64), region, [int(x) for x in layout]


@pytest.mark.parametrize("gather", [0, 2, 4])
def test_gather_bytes_equal_numpy(ctx, shapes, gather):
    for n, wps, kind, bits, order, want in shapes:
        got, _, _ = run_gather(ctx, bits, order, gather)
        assert got.tobytes() == want.tobytes(), (gather, n, wps, kind)


def compare_statistics(ctx, bits, order, label):
    """The statistics counted inside the gather against ballot gather + sample_stats_kernel:
    every byte of the region (stats, all rows of cum, the three sums, steps_out)."""
    n = bits.shape[0]
    copy, want, layout = run_gather(ctx, bits, order, 0, stats=2)
    s_stride, off_cum, off_sums, off_steps, _ = layout
    assert not (want[:off_sums].view(np.uint32) == 0xA5A5A5A5).any(), label   # all of it written
    sums = want[off_sums:off_sums + 24].view(np.uint64)
    for gather in (2, 4):
        got_copy, got, _ = run_gather(ctx, bits, order, gather, stats=1)
        assert got_copy.tobytes() == copy.tobytes(), (label, gather)
        for name, a, b in (("stats", 0, off_cum), ("cum", off_cum, off_sums),
                           ("sums", off_sums, off_sums + 24),
                           ("steps_out", off_steps, off_steps + 32)):
            assert got[a:b].tobytes() == want[a:b].tobytes(), (label, gather, name)
        assert got.tobytes() == want.tobytes(), (label, gather)
    return s_stride, sums


def test_fused_statistics_equal_the_separate_kernel(ctx, shapes):
    """The shapes of the gather test with at least 4 words per plane (a k-step is 4 words).
    A block is padded to 256 plane samples, 64 statistics workgroups: the cohort's sums take
    the first workgroup's four samples."""
    for n, wps, kind, bits, order, _ in shapes:
        if wps // 2 < 4:
            continue
        s_stride, sums = compare_statistics(ctx, bits, order, (n, wps, kind))
        assert s_stride == 256 and sums[0] == min(n, 4)


def test_fused_statistics_every_16th_workgroup(ctx):
    """1,100 samples: 320 statistics workgroups of four, the sums take every 16th -- samples
    64 j .. 64 j + 3 -- and genotype-like bits, so that the counts differ by sample."""
    rng = np.random.default_rng(2103)
    n = 1100
    for wps in (130, 15):
        p = wps // 2
        het = rng.integers(0, 1 << 62, (n, p), dtype=np.uint64) & \
            rng.integers(0, 1 << 62, (n, p), dtype=np.uint64)
        hom = rng.integers(0, 1 << 62, (n, p), dtype=np.uint64) & \
            rng.integers(0, 1 << 62, (n, p), dtype=np.uint64) & \
            rng.integers(0, 1 << 62, (n, p), dtype=np.uint64)
        bits = np.full((n, wps), SENTINEL, dtype=np.uint64)
        bits[:, :p], bits[:, p:2 * p] = het, hom
        order = make_order("sorted weights", 64 * p, rng)
        s_stride, sums = compare_statistics(ctx, bits, order, (n, wps))
        assert s_stride == 1280
        picked = [s for s in range(n) if (s // 4) % 16 == 0]
        assert sums[0] == len(picked) == 72
        missing = sum(bin(int(a & b)).count("1") for s in picked for a, b in zip(het[s], hom[s]))
        assert sums[1] == missing


def test_the_entry_point_refuses_what_it_cannot_serve(ctx):
    rng = np.random.default_rng(2104)
    bits = rng.integers(0, 1 << 62, (2, 14), dtype=np.uint64)
    order = np.arange(64 * 7, dtype=np.uint32)
    for gather, stats, word in ((1, 0, "form 1"), (3, 0, "form 3"), (-1, 0, "form -1"),
                                (0, 1, "statistics 1"), (4, 3, "statistics 3")):
        with pytest.raises(cuking_amd.CukingError, match=word):
            run_gather_raw(ctx, bits, order, gather, stats)
    # 4 samples a byte per site: 4,864 words per sample are beyond the LDS; 2 serves them
    wide = np.zeros((1, 4866), dtype=np.uint64)
    wide_order = np.arange(64 * 2433, dtype=np.uint32)
    with pytest.raises(cuking_amd.CukingError, match="form 4 does not serve 4866"):
        run_gather(ctx, wide, wide_order, 4)
    got, _, _ = run_gather(ctx, wide, wide_order, 2)
    assert not got.any()


def run_gather_raw(ctx, bits, order, gather, stats):
    import torch
    d_bits = ctx.upload_bitset(bits)
    d_order = torch.from_numpy(order.view(np.int32)).to(d_bits.device)
    d_out = torch.zeros_like(d_bits)
    d_stats = torch.zeros(1 << 20, dtype=torch.uint8, device=d_bits.device)
    check(ctx.lib.cuking_test_site_gather(ctx.handle, d_bits.data_ptr(), bits.shape[0],
                                          bits.shape[1], d_order.data_ptr(), gather,
                                          d_out.data_ptr(), stats, d_stats.data_ptr(), 1 << 20,
                                          None, int(torch.cuda.current_stream().cuda_stream)))


def plant(geno):
    """A duplicate, a parent-child-like and a sibling-like pair across tile boundaries."""
    n = geno.shape[0]
    geno[n - 1] = geno[3]
    half = geno.shape[1] // 2
    geno[n // 2, :half] = geno[5, :half]
    geno[n - 7, ::2] = geno[260 % n, ::2]
    return geno


def test_records_do_not_depend_on_the_gather(ctx, oracle):
    """1,100 x 20,480 with the order on: records byte-equal for "filter_site_gather" 0 / 2 / 4
    and to the oracle, the filter's counters equal."""
    rng = np.random.default_rng(2102)
    geno = plant(random_genotypes(rng, 1100, 20480, missing=0.01))
    bits = oracle.bitset_from_genotypes(geno)
    exp, _, _ = oracle.compute(oracle.submatrix(1100), bits, THR, threads=16)
    assert len(exp) >= 2
    sm = cuking_amd.Submatrix(1100)
    d_bits = ctx.upload_bitset(bits)
    ctx.set_kernel("tiled")
    ctx.set_option("variant", 7)
    try:
        ctx.set_option("counts_mode", 0)
        ctx.set_option("filter_check_min_steps", 4)
        ctx.set_option("filter_rotate_min_steps", 4)
        ctx.set_option("filter_rotate_min_tiles", 0)
        ctx.set_option("split_wgs", 0)
        ctx.set_option("filter_site_order", 1)
        ctx.set_option("filter_site_order_min_tiles", 0)
        ctx.set_option("filter_check0", 0)
        moved = {}
        for gather in (0, 2, 4):
            ctx.set_option("filter_site_gather", gather)
            before = [ctx.get_option(c) for c in COUNTERS]
            got = ctx.run(sm, bits.shape[1], d_bits, THR, max_results=1 << 20)
            moved[gather] = [ctx.get_option(c) - b for c, b in zip(COUNTERS, before)]
            assert ctx.get_option("site_order_on") == 1
            assert got.tobytes() == exp.tobytes(), gather
        assert moved[0] == moved[2] == moved[4], moved
        assert moved[0][1] > 0          # (tiles left at the check: the order was read)
    finally:
        for k, v in RESTORE:
            ctx.set_option(k, v)


def test_the_option_takes_its_four_values_only(ctx):
    try:
        for v in (-1, 0, 2, 4):
            ctx.set_option("filter_site_gather", v)
            assert ctx.get_option("filter_site_gather") == v
        for v in (-2, 1, 3, 5):
            with pytest.raises(cuking_amd.CukingError, match="filter_site_gather"):
                ctx.set_option("filter_site_gather", v)
    finally:
        ctx.set_option("filter_site_gather", -1)
