"""Dense kinship matrix (cuking_compute_kin_matrix, KingContext.kin_matrix) against the
CPU oracle's kinship of every pair (oracle.all_pairs).

The comparison is on the uint32 view, bit for bit, no tolerance: the library promises the
float a record of compute_king carries.  Where the oracle's value is NaN (0/0: a sample
without a het site) any NaN is accepted -- sign and payload of 0/0 differ between FPUs.
Outputs are prefilled with a finite sentinel, and every entry a call must leave alone is
checked to still hold it.

Shapes: the smallest that cross a 128-sample tile (130), a 256-sample tile (257) and a
k-step of 256 sites (257, 1000, 3000 sites); every cohort from 5 samples on has an
all-missing sample, a sample without hets and a duplicate pair, so that NaN, -inf and 0.5
all occur."""
import functools

import numpy as np
import pytest

import cuking_amd
from cuking_amd import _lib
from conftest import random_genotypes
from reducing_cases import assert_same

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.0)
NUM_VARIANTS = 8
# the context as it comes, every tiled variant, the stream kernel
KERNELS = [("default", None)] + [("tiled", v) for v in range(NUM_VARIANTS)] + [("stream", None)]
SHAPES = [(2, 1), (5, 32), (65, 257), (130, 1000), (257, 3000)]


def select(ctx, kernel, variant):
    if kernel == "default":
        return
    ctx.set_kernel(kernel)
    if variant is not None:
        ctx.set_option("variant", variant)


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


@functools.lru_cache(maxsize=None)
def cohort(n, m, split_factor=1, shard_index=0, low_call=()):
    """(bits of the block's samples, its (i_begin, i_end, j_begin, j_end), the expected
    matrix with SENTINEL wherever the oracle lists no pair).  Computed once per shape."""
    from oracle import pyoracle
    geno = make_genotypes(n, m, 1000 * n + m, low_call)
    osm = pyoracle.submatrix(n, split_factor, shard_index)
    sm = (osm.i_begin, osm.i_end, osm.j_begin, osm.j_end)
    idx = list(range(sm[0], sm[1]))
    if sm[0] != sm[2]:
        idx += list(range(sm[2], sm[3]))
    bits = pyoracle.bitset_from_genotypes(np.ascontiguousarray(geno[idx]))
    oi, oj, _, ok = pyoracle.all_pairs(osm, bits)
    exp = np.full((sm[1] - sm[0], sm[3] - sm[2]), SENTINEL, dtype=np.float32)
    exp[oi - sm[0], oj - sm[2]] = ok
    exp.setflags(write=False)
    bits.setflags(write=False)
    return bits, sm, exp


def prefilled(shape):
    import torch
    return torch.full(shape, float(SENTINEL), dtype=torch.float32, device="cuda:0")


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def run_upper(ctx, n, m, **kw):
    bits, sm, exp = cohort(n, m)
    d_bits = ctx.upload_bitset(np.array(bits))
    out = prefilled(exp.shape)
    got = ctx.kin_matrix(cuking_amd.Submatrix(n), bits.shape[1], d_bits, out=out, **kw)
    assert got is out
    return host(out), exp


def symmetric_expectation(exp, geno):
    full = np.array(exp)
    low = np.tril_indices(exp.shape[0], -1)
    full[low] = exp.T[low]
    has_het = (geno == 1).any(axis=1)
    full[np.diag_indices(exp.shape[0])] = np.where(has_het, np.float32(0.5), np.float32("nan"))
    return full


def test_variant_count():
    assert _lib.load().cuking_num_variants() == NUM_VARIANTS


@pytest.mark.parametrize("kernel,variant", KERNELS)
def test_every_pair(restored, kernel, variant):
    """Upper entries equal the oracle, the diagonal and the lower ones are untouched."""
    select(restored, kernel, variant)
    values = set()
    for n, m in SHAPES:
        got, exp = run_upper(restored, n, m)
        assert_same(got, exp, f"{n} x {m}")
        assert (got[np.tril_indices(n)] == SENTINEL).all()
        values.update(np.unique(got[np.triu_indices(n, 1)]).tolist())
    assert 0.5 in values and float("-inf") in values and any(np.isnan(v) for v in values)


@pytest.mark.parametrize("kernel,variant", [("default", None), ("tiled", 2), ("tiled", 5),
                                            ("stream", None)])
def test_off_diagonal_block(restored, kernel, variant):
    select(restored, kernel, variant)
    bits, sm, exp = cohort(300, 1000, 2, 1)
    assert exp.shape == (150, 150) and not (exp == SENTINEL).any()
    block = cuking_amd.Submatrix(300, split_factor=2, shard_index=1)
    assert block.as_tuple() == sm
    out = prefilled(exp.shape)
    restored.kin_matrix(block, bits.shape[1], restored.upload_bitset(np.array(bits)), out=out)
    assert_same(host(out), exp)


@pytest.mark.parametrize("kernel,variant", [("default", None), ("tiled", 6), ("tiled", 5),
                                            ("tiled", 0), ("stream", None)])
def test_symmetric(restored, kernel, variant):
    select(restored, kernel, variant)
    n, m = 257, 3000
    bits, _, exp = cohort(n, m)
    full = symmetric_expectation(exp, make_genotypes(n, m, 1000 * n + m))
    assert not (full == SENTINEL).any()
    assert np.isnan(full[1, 1]) and np.isnan(full[2, 2]) and full[0, 0] == 0.5
    out = prefilled((n, n))
    restored.kin_matrix(cuking_amd.Submatrix(n), bits.shape[1],
                        restored.upload_bitset(np.array(bits)), out=out, symmetric=True)
    got = host(out)
    assert_same(got, full)
    finite = ~np.isnan(got)
    assert np.array_equal(finite, finite.T)
    assert np.array_equal(got.view(np.uint32)[finite], got.T.view(np.uint32)[finite])


def test_symmetric_refusals(ctx):
    bits, _, exp = cohort(300, 1000, 2, 1)
    d_bits = ctx.upload_bitset(np.array(bits))
    block = cuking_amd.Submatrix(300, split_factor=2, shard_index=1)
    with pytest.raises(ValueError):
        ctx.kin_matrix(block, bits.shape[1], d_bits, symmetric=True)
    bits, _, _ = cohort(130, 1000)
    d_bits = ctx.upload_bitset(np.array(bits))
    with pytest.raises(ValueError):
        ctx.kin_matrix(cuking_amd.Submatrix(130), bits.shape[1], d_bits, symmetric=True,
                       tile_range=(0, 1))
    # ... and the library itself says the same
    lib, out = ctx.lib, prefilled((150, 150))
    import ctypes as C
    st = lib.cuking_compute_kin_matrix(ctx.handle, C.byref(block.c), bits.shape[1],
                                       d_bits.data_ptr(), out.data_ptr(), 150,
                                       _lib.KIN_SYMMETRIC, None)
    assert st == _lib.ERR_INVALID_ARGUMENT and b"diagonal" in lib.cuking_last_error()
    sm = cuking_amd.Submatrix(130)
    out = prefilled((130, 130))
    st = lib.cuking_compute_kin_matrix_tiles(ctx.handle, C.byref(sm.c), bits.shape[1],
                                             d_bits.data_ptr(), 0, 1, out.data_ptr(), 130,
                                             _lib.KIN_SYMMETRIC, None)
    assert st == _lib.ERR_INVALID_ARGUMENT and b"tile range" in lib.cuking_last_error()
    for ld, flags in ((129, _lib.KIN_UPPER), (130, 2)):
        st = lib.cuking_compute_kin_matrix(ctx.handle, C.byref(sm.c), bits.shape[1],
                                           d_bits.data_ptr(), out.data_ptr(), ld, flags, None)
        assert st == _lib.ERR_INVALID_ARGUMENT
    assert (host(out) == SENTINEL).all()


def test_allocated_result_and_out_checks(ctx):
    import torch
    n, m = 65, 257
    bits, _, exp = cohort(n, m)
    d_bits = ctx.upload_bitset(np.array(bits))
    sm = cuking_amd.Submatrix(n)
    got = ctx.kin_matrix(sm, bits.shape[1], d_bits)
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, n) and got.is_cuda
    got = host(got)
    upper = np.triu_indices(n, 1)
    want = np.full((n, n), np.float32("nan"))
    want[upper] = exp[upper]
    assert_same(got, want)                      # untouched entries are NaN
    for bad in (torch.zeros((n, n), dtype=torch.float64, device="cuda:0"),
                torch.zeros((n, n + 1), dtype=torch.float32, device="cuda:0"),
                torch.zeros((n, n), dtype=torch.float32),
                torch.zeros((n, 2 * n), dtype=torch.float32, device="cuda:0")[:, ::2]):
        with pytest.raises(ValueError):
            ctx.kin_matrix(sm, bits.shape[1], d_bits, out=bad)


@pytest.mark.parametrize("kernel,variant", [("default", None), ("tiled", 3), ("stream", None)])
def test_strided_out(restored, kernel, variant):
    select(restored, kernel, variant)
    n, m = 130, 1000
    bits, _, exp = cohort(n, m)
    buf = prefilled((n, n + 37))
    restored.kin_matrix(cuking_amd.Submatrix(n), bits.shape[1],
                        restored.upload_bitset(np.array(bits)), out=buf[:, :n])
    got = host(buf)
    assert_same(np.ascontiguousarray(got[:, :n]), exp)
    assert (got[:, n:] == SENTINEL).all()       # the 37 padding columns


@pytest.mark.parametrize("variant", [None, 6, 2])
def test_tile_ranges(restored, variant):
    """Three disjoint ranges into one buffer equal the whole call; one range alone leaves
    entries outside it untouched."""
    if variant is not None:
        restored.set_option("variant", variant)
    n, m = 600, 2000
    bits, _, exp = cohort(n, m)
    sm = cuking_amd.Submatrix(n)
    d_bits = restored.upload_bitset(np.array(bits))
    tiles = restored.num_tiles(sm)
    assert tiles >= 3
    parts = (np.zeros(6, dtype=np.uint64))
    restored.lib.cuking_schedule_tile_partition(tiles, 3, parts.ctypes.data)
    ranges = [(int(parts[2 * r]), int(parts[2 * r + 1])) for r in range(3)]
    assert ranges[0][0] == 0 and ranges[2][1] == tiles
    out = prefilled((n, n))
    restored.kin_matrix(sm, bits.shape[1], d_bits, out=out, tile_range=ranges[0])
    first = host(out)
    upper = np.triu_indices(n, 1)
    written = first[upper] != SENTINEL
    assert written.any() and not written.all()
    assert_same(np.where(first != SENTINEL, first, exp), exp)   # what is written is right
    for r in ranges[1:]:
        restored.kin_matrix(sm, bits.shape[1], d_bits, out=out, tile_range=r)
    assert_same(host(out), exp)


def test_sorted_layout(restored):
    """A cohort whose low-call-rate samples the default context sorts to the end of its
    layout: the matrix still lands at the stored samples' positions, and thresholded runs
    on the same context before and after still give the oracle's records (with and without
    the reuse of a prepared layout)."""
    from oracle import pyoracle
    n, m, thr = 600, 2000, 0.0884
    low = tuple(range(7, 600, 50))
    assert len(low) == 12
    bits, _, exp = cohort(n, m, low_call=low)
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
            out = prefilled((n, n))
            restored.kin_matrix(sm, bits.shape[1], d_bits, out=out)
            assert_same(host(out), exp, f"reuse_prepared {reuse}")
            assert restored.run(sm, bits.shape[1], d_bits, thr).tobytes() == records.tobytes()
            out = prefilled((n, n))
            restored.kin_matrix(sm, bits.shape[1], d_bits, out=out)
            assert_same(host(out), exp, f"reuse_prepared {reuse}, second call")
    finally:
        restored.set_option("reuse_prepared", 0)
        restored.invalidate()


def test_launch_shapes(restored):
    """Several launches, remainder pieces, the dynamic tail: the same matrix each time."""
    n, m = 600, 2000
    bits, _, exp = cohort(n, m)
    sm = cuking_amd.Submatrix(n)
    d_bits = restored.upload_bitset(np.array(bits))

    def check(what):
        out = prefilled((n, n))
        restored.kin_matrix(sm, bits.shape[1], d_bits, out=out)
        assert_same(host(out), exp, what)
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


@pytest.mark.parametrize("sites", [(1 << 22) + 64, (1 << 24) + 64])
def test_wide_bitset_route(ctx, sites):
    """From 2^22 sites on the default context hands the block to the five-product kernel,
    from 2^24 on to a VALU shape: the same matrix.  (Random planes: a quarter of the calls
    missing; the sites behind the last one are missing.)"""
    from oracle import pyoracle
    n = 6
    wps = cuking_amd.words_per_sample(sites)
    rng = np.random.default_rng(sites)
    bits = rng.integers(0, 1 << 63, size=(n, wps), dtype=np.uint64) << np.uint64(1) | \
        rng.integers(0, 2, size=(n, wps), dtype=np.uint64)
    bits[:, wps // 2 - 1] = ~np.uint64(0)      # the het plane's last word ...
    bits[:, wps - 1] = ~np.uint64(0)           # ... and the hom_var plane's: missing
    bits[1] = ~np.uint64(0)
    osm = pyoracle.submatrix(n)
    oi, oj, _, ok = pyoracle.all_pairs(osm, bits)
    exp = np.full((n, n), SENTINEL, dtype=np.float32)
    exp[oi, oj] = ok
    out = prefilled((n, n))
    ctx.kin_matrix(cuking_amd.Submatrix(n), wps, ctx.upload_bitset(bits), out=out)
    assert_same(host(out), exp)
