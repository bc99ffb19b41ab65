"""PI_HAT records on the device (cuking_compute_pihat, KingContext.pi_hat_records): the device
records, sorted, equal the host twin's bytes -- no tolerance, the pair math of csrc/king_pihat.h
is one sequence of IEEE double operations on both sides.  Variants 5, 6 and 7; shapes 2 x 64,
129 x 520 (one past a tile edge, a word count that is no multiple of 8), 333 x 5000 (the
smoke() cohort: the diagonal block and the off-diagonal blocks of split_factor 2 and 3); the
launch shapes test_gpu_kin_matrix.py forces; tile ranges; counting and overflow; a second
stream; compute_king before and after; the wrapper's retry and a shared model across blocks."""
import ctypes as C
import functools

import numpy as np
import pytest

import cuking_amd
from cuking_amd import _lib

import pihat_cases as pc
from pihat_cases import raw_call   # (tests/test_gpu_call_forms.py takes it from here)

pytestmark = pytest.mark.gpu

VARIANTS = (5, 6, 7)
MIN_PI_HAT = 0.05


@pytest.fixture
def restored(ctx):
    """The shared context, put back the way it came."""
    variant = ctx.get_option("variant")
    yield ctx
    ctx.set_kernel("tiled")
    ctx.set_option("variant", variant)


def block_bits(host, sm):
    if sm.i_begin == sm.j_begin:
        return np.ascontiguousarray(host[sm.i_begin:sm.i_end])
    return np.ascontiguousarray(np.concatenate([host[sm.i_begin:sm.i_end],
                                                host[sm.j_begin:sm.j_end]]))


@functools.lru_cache(maxsize=None)
def cohort(n, m):
    """(host bits [n, wps], wps, the model of all n samples).  Computed once per shape."""
    if (n, m) == (pc.SMOKE["n"], pc.SMOKE["m"]):
        _, host, wps = pc.smoke_cohort()
    else:
        wps = cuking_amd.words_per_sample(m)
        host = pc.random_bits(np.random.default_rng(1000 * n + m), n, m, wps)
        host.setflags(write=False)
    counts = cuking_amd.pihat.site_counts_of_host_bits(np.array(host), wps)
    return host, wps, cuking_amd.pi_hat_model_host(counts, m)


@functools.lru_cache(maxsize=None)
def expected(n, m, split_factor=1, shard=0, min_pi_hat=MIN_PI_HAT, bounded=True):
    """The host twin's records of a block (ascending (i, j)), computed once and left alone."""
    host, wps, model = cohort(n, m)
    sm = cuking_amd.Submatrix(n, split_factor, shard)
    got = cuking_amd.pi_hat_records_host(sm, wps, block_bits(host, sm), m, min_pi_hat,
                                         model=model, bounded=bounded)
    got.records.setflags(write=False)
    return got.records


def device_block(ctx, n, m, split_factor=1, shard=0):
    host, wps, model = cohort(n, m)
    sm = cuking_amd.Submatrix(n, split_factor, shard)
    return sm, wps, ctx.upload_bitset(block_bits(host, sm)), model


# (every shard of split_factor 2 and 3: their diagonal blocks and all four off-diagonal ones)
BLOCKS = [(2, 64, 1, 0), (129, 520, 1, 0), (333, 5000, 1, 0)] + \
    [(333, 5000, 2, k) for k in range(3)] + [(333, 5000, 3, k) for k in range(6)]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n,m,split_factor,shard", BLOCKS)
def test_device_equals_host_twin(restored, variant, n, m, split_factor, shard):
    restored.set_option("variant", variant)
    sm, wps, d_bits, model = device_block(restored, n, m, split_factor, shard)
    # (at -1 every pair of the block is a record: every pair's float and counts are compared)
    for thr, bounded in ((MIN_PI_HAT, True), (MIN_PI_HAT, False), (-1.0, True)):
        want = expected(n, m, split_factor, shard, thr, bounded)
        got = restored.pi_hat_records(sm, wps, d_bits, m, thr, model=model, bounded=bounded)
        assert got.num_records == len(want)
        assert got.sorted().tobytes() == want.tobytes(), (variant, thr, bounded)
    assert len(want) == sm.NumPairs() > 0


def test_off_diagonal_blocks_are_covered():
    shapes = [cuking_amd.Submatrix(333, sf, k) for sf in (2, 3) for k in range(sf * (sf + 1) // 2)]
    assert sum(sm.i_begin != sm.j_begin for sm in shapes) == 4
    assert len(expected(333, 5000)) > 20


def test_smoke_cohort_planted_pairs(restored):
    """The scan at the middle of the gap measured on the CPU (pihat_cases.SMOKE_GAP) returns
    exactly the planted pairs; the model is the default, of the block's own samples."""
    n, m = pc.SMOKE["n"], pc.SMOKE["m"]
    cohort_plan, _, _ = pc.smoke_cohort()
    sm, wps, d_bits, model = device_block(restored, n, m)
    thr = sum(pc.SMOKE_GAP) / 2
    for variant in VARIANTS:
        restored.set_option("variant", variant)
        got = restored.pi_hat_records(sm, wps, d_bits, m, thr)
        assert got.model == model          # (site_counts on the device, the model on the host)
        planted = {(min(a, b), max(a, b)) for a, b, _ in cohort_plan.planted}
        assert {(int(a), int(b)) for a, b in got.pairs()} == planted
        assert got.sorted().tobytes() == expected(n, m, 1, 0, thr).tobytes()
        z = got.z()
        assert z.shape == (17, 4) and z[:, 2].max() == 1.0


def test_launch_shapes(restored):
    """Several launches, remainder pieces (the SPLIT launch), the dynamic tail, plain tile
    order: the same records each time, from the whole-tile and the split kernels."""
    n, m = 600, 2000
    sm, wps, d_bits, model = device_block(restored, n, m)
    # (random unrelated samples: at -1 every pair is a record, its float and counts compared)
    want = expected(n, m, 1, 0, -1.0)
    assert len(want) == n * (n - 1) // 2

    def check(what):
        got = restored.pi_hat_records(sm, wps, d_bits, m, -1.0, model=model)
        assert got.sorted().tobytes() == want.tobytes(), what
    try:
        restored.set_option("variant", 7)
        restored.set_option("max_launch_blocks", 3)
        check("max_launch_blocks 3")
        restored.set_option("variant", 5)
        check("max_launch_blocks 3, variant 5")
        restored.set_option("max_launch_blocks", 0)
        restored.set_option("split_wgs", 6)
        for variant in (6, 5, 7):
            restored.set_option("variant", variant)
            check(f"split_wgs 6, variant {variant}")
        restored.set_option("split_wgs", 0)
        for variant in (6, 5):
            restored.set_option("variant", variant)
            check(f"split_wgs 0 (whole tiles only), variant {variant}")
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


@pytest.mark.parametrize("variant", VARIANTS)
def test_counting_overflow_tile_ranges_streams(restored, variant):
    import torch
    restored.set_option("variant", variant)
    n, m = 333, 5000
    sm, wps, d_bits, model = device_block(restored, n, m)
    want = expected(n, m)
    total = len(want)
    assert total > 20
    # max_results = 0 gives the count alone
    rows, count, overflow, behind = raw_call(restored, sm, wps, d_bits, model, 0)
    assert (len(rows), count, overflow) == (0, total, 1) and (behind == 0x55555555).all()
    # exact
    rows, count, overflow, behind = raw_call(restored, sm, wps, d_bits, model, total)
    assert (count, overflow) == (total, 0) and (behind == 0x55555555).all()
    assert cuking_amd.sort_results(rows.copy()).tobytes() == want.tobytes()
    # one short: the flag, the exact count, nothing past the buffer, every row a real record
    rows, count, overflow, behind = raw_call(restored, sm, wps, d_bits, model, total - 1)
    assert (count, overflow) == (total, 1) and (behind == 0x55555555).all()
    listed = {r.tobytes() for r in want}
    assert len(rows) == total - 1 and all(r.tobytes() in listed for r in rows)
    # two disjoint tile ranges that cover the block equal the whole call
    tiles = restored.num_tiles(sm)
    assert tiles >= 2
    cut = tiles // 2
    a, ca, _, _ = raw_call(restored, sm, wps, d_bits, model, total, (0, cut))
    b, cb, _, _ = raw_call(restored, sm, wps, d_bits, model, total, (cut, tiles))
    assert ca + cb == total and 0 < ca < total
    assert cuking_amd.sort_results(np.concatenate([a, b])).tobytes() == want.tobytes()
    _, none, _, _ = raw_call(restored, sm, wps, d_bits, model, total, (cut, cut))
    assert none == 0
    # a second stream and a repeated call
    side = torch.cuda.Stream(device=restored.device)
    for _ in range(2):
        rows, count, overflow, _ = raw_call(restored, sm, wps, d_bits, model, total, stream=side)
        assert (count, overflow) == (total, 0)
        assert cuking_amd.sort_results(rows.copy()).tobytes() == want.tobytes()
    via = restored.pi_hat_records(sm, wps, d_bits, m, MIN_PI_HAT, model=model, stream=side)
    assert via.sorted().tobytes() == want.tobytes()


@pytest.mark.parametrize("variant", VARIANTS)
def test_next_to_compute_king(restored, variant):
    """compute_king before and after on the same context returns its usual records (the layout
    is handed back), and the ibs fields of the pairs both calls list are equal."""
    from oracle import pyoracle
    restored.set_option("variant", variant)
    n, m = 333, 5000
    sm, wps, d_bits, model = device_block(restored, n, m)
    host, _, _ = cohort(n, m)
    king, _, _ = pyoracle.compute(pyoracle.submatrix(n), np.array(host), 0.05)
    assert restored.run(sm, wps, d_bits, 0.05).tobytes() == king.tobytes()
    got = restored.pi_hat_records(sm, wps, d_bits, m, MIN_PI_HAT, model=model)
    assert got.sorted().tobytes() == expected(n, m).tobytes()
    assert restored.run(sm, wps, d_bits, 0.05).tobytes() == king.tobytes()
    # every pair's ibs fields against those of the KING records at the lowest threshold
    every_king = restored.run(sm, wps, d_bits, -1e30)
    every = restored.pi_hat_records(sm, wps, d_bits, m, -1.0, model=model).sorted()
    by_pair = {(int(r["sample_i"]), int(r["sample_j"])): r for r in every_king}
    shared = 0
    for r in every:
        k = by_pair.get((int(r["sample_i"]), int(r["sample_j"])))
        if k is not None:
            shared += 1
            assert (r["ibs0"], r["ibs1"], r["ibs2"]) == (k["ibs0"], k["ibs1"], k["ibs2"])
    assert shared > n * (n - 1) // 4
    # ... and pi_hat_of_records re-scores the KING buffer with no GPU code at all
    z = cuking_amd.pi_hat_of_records(king, model)
    assert z.shape == (len(king), 4)
    pihat = {(int(r["sample_i"]), int(r["sample_j"])): r["kin"] for r in every}
    for r, row in zip(king, z):
        assert np.float32(row[3]) == pihat[(int(r["sample_i"]), int(r["sample_j"]))]


def test_wrapper_buffer_rule_and_shared_model(restored):
    restored.set_option("variant", 7)
    n, m = 333, 5000
    sm, wps, d_bits, model = device_block(restored, n, m)
    # more records than the default buffer (16 per sample) holds: one repeat with the exact count
    everything = expected(n, m, 1, 0, -1.0)
    assert len(everything) == n * (n - 1) // 2 > 16 * 2 * n
    got = restored.pi_hat_records(sm, wps, d_bits, m, -1.0, model=model)
    assert got.num_records == len(everything) and got.sorted().tobytes() == everything.tobytes()
    # max_results given: the error carries the count; 0 counts
    want = expected(n, m)
    for cap in (0, len(want) - 1):
        with pytest.raises(cuking_amd.ResourceExhaustedError) as e:
            restored.pi_hat_records(sm, wps, d_bits, m, MIN_PI_HAT, model=model, max_results=cap)
        assert e.value.num_records == len(want)
    exact = restored.pi_hat_records(sm, wps, d_bits, m, MIN_PI_HAT, model=model,
                                    max_results=len(want))
    assert exact.sorted().tobytes() == want.tobytes()
    # model= across the blocks of a split cohort reproduces the whole-cohort call's records
    whole = restored.pi_hat_records(sm, wps, d_bits, m, MIN_PI_HAT)
    assert whole.model == model
    rows = []
    for shard in range(3):
        bsm, _, b_bits, _ = device_block(restored, n, m, 2, shard)
        rows.append(restored.pi_hat_records(bsm, wps, b_bits, m, MIN_PI_HAT,
                                            model=whole.model).sorted())
    assert cuking_amd.sort_results(np.concatenate(rows)).tobytes() == whole.sorted().tobytes()
    # counts= of other rows (the first 200 samples as "founders") is what the model comes from
    founders = restored.site_counts(d_bits[:200], wps)
    by_counts = restored.pi_hat_records(sm, wps, d_bits, m, MIN_PI_HAT, counts=founders)
    host, _, _ = cohort(n, m)
    f_model = cuking_amd.pi_hat_model_host(
        cuking_amd.pihat.site_counts_of_host_bits(np.array(host[:200]), wps), m)
    assert by_counts.model == f_model and f_model != model


def test_refused_contexts(restored):
    """Every context without a matrix-core kernel is refused as kin_summary refuses it."""
    sm, wps, d_bits, model = device_block(restored, 2, 64)
    for kernel, variant in (("tiled", 0), ("tiled", 2), ("stream", None)):
        restored.set_kernel(kernel)
        if variant is not None:
            restored.set_option("variant", variant)
        with pytest.raises(_lib.CukingError, match="variant 5, 6 or 7"):
            restored.pi_hat_records(sm, wps, d_bits, 64, model=model)
    restored.set_kernel("tiled")
    restored.set_option("variant", 7)
    with pytest.raises(_lib.CukingError, match="unknown flags"):
        import torch
        words = torch.zeros(2, dtype=torch.int32, device=f"cuda:{restored.device}")
        _lib.check(restored.lib.cuking_compute_pihat(
            restored.handle, C.byref(sm.c), wps, d_bits.data_ptr(), C.byref(model.c), 0.1, 2, 0,
            None, words[0:1].data_ptr(), words[1:2].data_ptr(), None))


@pytest.mark.parametrize("sites", [(1 << 22) + 64, (1 << 24) + 64])
def test_wide_bitsets(restored, sites):
    """From 2^22 sites on the default context hands the block to the five-product form: the
    same records; from 2^24 sites on the call is refused (the matrix cores count in float32).
    (Random planes: a quarter of the calls missing; the sites behind the last one are missing.)"""
    from cuking_amd.pihat import PiHatModel
    restored.set_option("variant", 7)
    n = 6
    wps = cuking_amd.words_per_sample(sites)
    rng = np.random.default_rng(sites)
    bits = rng.integers(0, 1 << 63, size=(n, wps), dtype=np.uint64) << np.uint64(1) | \
        rng.integers(0, 2, size=(n, wps), dtype=np.uint64)
    bits[:, wps // 2 - 1] = ~np.uint64(0)      # the het plane's last word ...
    bits[:, wps - 1] = ~np.uint64(0)           # ... and the hom_var plane's: missing
    model = PiHatModel(0.08, 0.42, 0.5, 0.36, 0.64, sites)
    sm = cuking_amd.Submatrix(n)
    d_bits = restored.upload_bitset(bits)
    if sites > 1 << 24:
        with pytest.raises(_lib.CukingError, match="2\\^24 sites"):
            restored.pi_hat_records(sm, wps, d_bits, sites, -1.0, model=model)
        return
    want = cuking_amd.pi_hat_records_host(sm, wps, bits, sites, -1.0, model=model).records
    got = restored.pi_hat_records(sm, wps, d_bits, sites, -1.0, model=model)
    assert got.num_records == len(want) == 15
    assert got.sorted().tobytes() == want.tobytes()


def test_wrapper_on_a_side_stream_first(restored):
    """The wrapper's own zero-fills (record buffer, counter words, site counts) run on the current
    stream and the call on `stream`: the first call on a fresh bitset, with nothing in front of
    it on the side stream, returns the host twin's records and the model of the block."""
    import torch
    restored.set_option("variant", 6)
    n, m = 333, 5000
    sm, wps, d_bits, model = device_block(restored, n, m)
    side = torch.cuda.Stream(device=restored.device)
    for _ in range(3):
        fresh = d_bits.clone()
        got = restored.pi_hat_records(sm, wps, fresh, m, MIN_PI_HAT, stream=side)
        assert got.model == model
        assert got.sorted().tobytes() == expected(n, m).tobytes()
