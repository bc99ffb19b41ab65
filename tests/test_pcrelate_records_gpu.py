"""PC-Relate records on the GPU: pcrelate_records_kernel against the device's own
pcrelate_matrix of the same block thresholded -- the same pairs and the same kin bytes, so no
tolerance --, the strict comparison, the host twin's set at the gap thresholds, calls, streams
and sub-blocks, the overflow rule, the refusals on a live context, and the end-to-end fixture
through ctx.pca -> ctx.pcrelate_records -> pcrelate_pairs / unrelated_set."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import pcrelate_cases as pc
import pcrelate_records_cases as rc

import cuking_amd
from cuking_amd import KING_RESULT_DTYPE, _lib
from cuking_amd.pcrelate import pcrelate_records_raw_host, records_to_host

pytestmark = pytest.mark.gpu

_CTX = []


@pytest.fixture(autouse=True)
def _context(ctx):
    if not _CTX:
        _CTX.append(ctx)


@lru_cache(maxsize=None)
def uploaded(case):
    """(bits, x, beta) on the device, x and beta with the host's pitch and NaN in the pad."""
    import torch
    ctx = _CTX[0]
    inp = pc.inputs(case)
    dev = f"cuda:{ctx.device}"

    def padded(a):
        pitch = a.strides[0] // 4
        wide = np.full((a.shape[0], pitch), np.float32(np.nan), dtype=np.float32)
        wide[:, :a.shape[1]] = a
        return torch.from_numpy(wide).to(dev)[:, :a.shape[1]]
    return ctx.upload_bitset(inp.bits.copy()), padded(inp.x), padded(inp.beta)


@lru_cache(maxsize=None)
def device_matrix(case, block=None):
    import torch
    inp = pc.inputs(case)
    bits, x, beta = uploaded(case)
    out = _CTX[0].pcrelate_matrix(bits, inp.wps, case.sites, x, beta, inp.lo, inp.hi,
                                  block=case.block if block is None else block)
    torch.cuda.synchronize()
    return out.cpu().numpy().copy()


def device_records(case, min_kin, block=None, **kw):
    """(sorted host records, count) of one call."""
    inp = pc.inputs(case)
    bits, x, beta = uploaded(case)
    records, count = _CTX[0].pcrelate_records_raw(
        bits, inp.wps, case.sites, x, beta, inp.lo, inp.hi, min_kin,
        block=case.block if block is None else block, **kw)
    return records_to_host(records, count), count


@pytest.mark.parametrize("case", rc.CASES, ids=lambda c: c.name)
def test_device_records_equal_the_device_matrix_thresholded(case):
    kin = device_matrix(case)
    pairs = rc.pair_mask(case.block) & ~np.isnan(kin)
    extra = ()
    if pairs.any():     # the exact float of one entry: that pair is absent (catches >=)
        values = np.sort(kin[pairs])
        extra = (float(values[values.size // 2]),)
    for t in rc.thresholds(case) + extra:
        got, count = device_records(case, t)
        want = rc.threshold_matrix(kin, case.block, t)
        assert count == got.shape[0] == want.shape[0], (t, count, want.shape[0])
        rc.check_records(got, case.block)
        rc.same_records(got, want)
    if extra:
        t = np.float32(extra[0])
        got, _ = device_records(case, extra[0])
        assert not (got["kin"] == t).any() and (kin[pairs] == t).any()
        assert got.shape[0] == int((kin[pairs] > t).sum())


@pytest.mark.parametrize("d", range(1, 33))
def test_ladder_device_records_against_float64_reference(d):
    """Every d from 1 to 32 -- each instantiation of pcrelate_records_kernel at its width, below
    it and at the first d of the next -- at 130 samples x 97 sites, the whole block and (5, 70,
    97, 130): at -inf the records are the reference's pairs of defined kinship, each within
    tolerance, and the device matrix thresholded on bytes; at the median VALUE of the device
    matrix, which a pair sits on, the strict comparison decides."""
    for block in pc.LADDER_BLOCKS:
        case = pc.ladder_case(d, block)
        kin = device_matrix(case)
        got, count = device_records(case, -rc.INF)
        assert count == got.shape[0]
        rc.check_records_reference(pc.reference(case), block, got, case.name, "device")
        rc.same_records(got, rc.threshold_matrix(kin, block, -rc.INF))
        values = np.sort(kin[rc.pair_mask(block) & ~np.isnan(kin)])
        t = float(values[values.size // 2])
        got, count = device_records(case, t)
        assert count == got.shape[0] < values.size
        rc.same_records(got, rc.threshold_matrix(kin, block, t))


@pytest.mark.parametrize("case", rc.CASES, ids=lambda c: c.name)
def test_device_set_equals_the_host_twin_at_the_gap_thresholds(case):
    inp = pc.inputs(case)
    for gap in rc.gap_thresholds(case):
        got, _ = device_records(case, gap.threshold)
        host, _ = pcrelate_records_raw_host(inp.bits, inp.wps, case.sites, inp.x, inp.beta, inp.lo,
                                            inp.hi, gap.threshold, block=case.block)
        assert np.array_equal(got["sample_i"], host["sample_i"])
        assert np.array_equal(got["sample_j"], host["sample_j"])


def test_counts_at_the_infinities_and_no_work_cases():
    for case in rc.CASES:
        kin = device_matrix(case)
        nan_pairs = int((rc.pair_mask(case.block) & np.isnan(kin)).sum())
        assert device_records(case, -rc.INF)[1] == rc.num_pairs(case.block) - nan_pairs
        assert device_records(case, rc.INF)[1] == 0
    case = pc.CASES[4]
    assert device_records(case, -rc.INF, block=(4, 4, 9, 20))[1] == 0
    assert device_records(case, -rc.INF, block=(7, 8, 7, 8))[1] == 0
    inp = pc.inputs(case)
    bits, x, beta = uploaded(case)
    assert _CTX[0].pcrelate_records_raw(bits, inp.wps, 0, x, beta, inp.lo, inp.hi,
                                        -rc.INF)[1] == 0


def test_calls_streams_and_sub_blocks_give_the_same_set():
    import torch
    case = next(c for c in rc.CASES if c.name == "257x700 d3")
    t = rc.gap_thresholds(case)[1].threshold
    first, _ = device_records(case, t)
    second, _ = device_records(case, t)
    rc.same_records(second, first)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    other, _ = device_records(case, t, stream=stream)
    rc.same_records(other, first)
    # the diagonal block assembled from two diagonal blocks and the off-diagonal one between
    parts = [device_records(case, t, block=b)[0]
             for b in ((0, 130, 0, 130), (130, 257, 130, 257), (0, 130, 130, 257))]
    joined = cuking_amd.sort_results(np.concatenate(parts))
    rc.same_records(joined, first)
    # and at -inf, where every wavefront reserves slots
    everything, count = device_records(case, -rc.INF)
    parts = [device_records(case, -rc.INF, block=b)[0]
             for b in ((0, 130, 0, 130), (130, 257, 130, 257), (0, 130, 130, 257))]
    rc.same_records(cuking_amd.sort_results(np.concatenate(parts)), everything)


def test_launches_are_split(ctx):
    """A cap of two workgroups per launch sends the six tiles of the 257-sample triangle out in
    three launches, the last with block_base = 4; the off-diagonal block has 2 x 1 tiles, which
    a cap of one splits as well.  At a gap threshold and at -inf: the sorted records and the
    count of the one launch."""
    case = next(c for c in rc.CASES if c.name == "257x700 d3")
    calls = [(t, block) for t in (rc.gap_thresholds(case)[1].threshold, -rc.INF)
             for block in (None, (0, 130, 130, 257))]
    whole = [device_records(case, t, block=block) for t, block in calls]
    assert whole[0][1] > 64 and whole[3][1] > 64
    for cap in (2, 1):
        ctx.set_option("max_launch_blocks", cap)
        try:
            split = [device_records(case, t, block=block) for t, block in calls]
        finally:
            ctx.set_option("max_launch_blocks", 0)
        for (got, count), (want, want_count) in zip(split, whole):
            assert count == want_count == want.shape[0]
            assert np.array_equal(got.view(np.uint8), want.view(np.uint8))


def test_overflow_counts_exactly_and_writes_nothing_behind_the_buffer(ctx):
    import torch
    case = next(c for c in rc.CASES if c.name == "257x700 d3")
    inp = pc.inputs(case)
    bits, x, beta = uploaded(case)
    t = rc.gap_thresholds(case)[1].threshold
    full, total = device_records(case, t)
    assert total > 64
    true_set = {(int(r["sample_i"]), int(r["sample_j"])): r["kin"].tobytes() for r in full}
    before = ctx.get_option("host_syncs")
    _, count = ctx.pcrelate_records_raw(bits, inp.wps, case.sites, x, beta, inp.lo, inp.hi, t,
                                        block=case.block, max_records=total)
    assert count == total
    assert ctx.get_option("host_syncs") - before == 1   # (the count, and nothing else)
    for room in (total - 1, total // 2, 0):
        buf = torch.full((room + 3, 6), -1414812757, dtype=torch.int32,
                         device=f"cuda:{ctx.device}")      # (0xABABABAB)
        with pytest.raises(cuking_amd.ResourceExhaustedError) as e:
            ctx.pcrelate_records_raw(bits, inp.wps, case.sites, x, beta, inp.lo, inp.hi, t,
                                     block=case.block, max_records=room, out=buf)
        assert e.value.num_records == total
        host = buf.cpu().numpy()
        assert (host[room:] == -1414812757).all()
        stored = np.ascontiguousarray(host[:room]).view(KING_RESULT_DTYPE).reshape(-1)
        rc.check_records(stored, case.block)            # (duplicate-free)
        for r in stored:                                # a subset of the true set, same bytes
            assert true_set[(int(r["sample_i"]), int(r["sample_j"]))] == r["kin"].tobytes()
    # the counting call proper: no buffer at all
    count = C.c_uint64(7)
    block = _lib.CSubmatrix(*case.block)
    st = ctx.lib.cuking_pcrelate_records(
        ctx.handle, bits.data_ptr(), case.n, inp.wps, case.sites, x.data_ptr(), x.stride(0),
        beta.data_ptr(), beta.stride(0), case.d, inp.lo, inp.hi, C.byref(block), t, None, 0,
        C.byref(count), int(torch.cuda.current_stream().cuda_stream))
    assert st == _lib.ERR_RESOURCE_EXHAUSTED and count.value == total
    # the retrying wrapper: more records than the default buffer's 16 per sample
    everything, count = device_records(case, -rc.INF)
    assert count > 16 * 2 * case.n
    rc.same_records(everything, rc.threshold_matrix(device_matrix(case), case.block, -rc.INF))


REFUSALS = {k: {n: v for n, v in over.items() if n != "ldo"} for k, over in pc.REFUSALS.items()
            if k not in ("pitch below the columns", "null out")}
REFUSALS.update({
    "min_kin NaN": dict(min_kin=float("nan")),
    "null num_records": dict(num_records=None),
    "null records with room": dict(records=None),
})


@pytest.mark.parametrize("name", REFUSALS)
def test_device_refusals_leave_the_buffer_untouched(ctx, name):
    import torch
    case = pc.CASES[4]
    inp = pc.inputs(case)
    bits, x, beta = uploaded(case)
    buf = torch.full((528, 6), -7, dtype=torch.int32, device=f"cuda:{ctx.device}")
    count = C.c_uint64(12345)
    a = dict(bits=bits.data_ptr(), num_stored=case.n, wps=inp.wps, sites=case.sites,
             x=x.data_ptr(), ldx=x.stride(0), beta=beta.data_ptr(), ldbeta=beta.stride(0),
             d=case.d, lo=inp.lo, hi=inp.hi, block=(0, case.n, 0, case.n), min_kin=-rc.INF,
             records=buf.data_ptr(), max_records=528, num_records=C.byref(count))
    a.update(REFUSALS[name])
    block = _lib.CSubmatrix(*a["block"])
    st = ctx.lib.cuking_pcrelate_records(
        ctx.handle, a["bits"], a["num_stored"], a["wps"], a["sites"], a["x"], a["ldx"],
        a["beta"], a["ldbeta"], a["d"], a["lo"], a["hi"], C.byref(block), a["min_kin"],
        a["records"], a["max_records"], a["num_records"],
        int(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert st == _lib.ERR_INVALID_ARGUMENT, name
    assert (buf == -7).all()
    assert count.value == (12345 if name == "null num_records" else 0)


def test_wrapper_refusals(ctx):
    import torch
    case = pc.CASES[4]
    inp = pc.inputs(case)
    bits, x, beta = uploaded(case)
    args = (bits, inp.wps, 63, x, beta, inp.lo, inp.hi)
    with pytest.raises(ValueError, match="NaN"):
        ctx.pcrelate_records_raw(*args, float("nan"))
    with pytest.raises(cuking_amd.CukingError):
        ctx.pcrelate_records_raw(*args, 0.0, block=(0, 40, 0, 40))
    with pytest.raises(ValueError):
        ctx.pcrelate_records_raw(*args, 0.0, max_records=9,
                                 out=torch.zeros((8, 6), dtype=torch.int32, device=bits.device))
    with pytest.raises(ValueError, match="either scores or model"):
        ctx.pcrelate_records(bits, inp.wps, 63)


def test_end_to_end_on_the_device(ctx):
    """At min_kinship = 0.125 the records are exactly the 30 planted first-degree pairs (the
    fixture's conditions put every pair further from 0.125 than any tolerance); they go to
    pcrelate_pairs and unrelated_set as they stand."""
    import torch
    from site_qc_cases import pack
    geno, population, fit, related = pc.e2e_cohort()
    host_bits = pack(np.asarray(geno))
    wps = host_bits.shape[1]
    bits = ctx.upload_bitset(host_bits)
    pca = ctx.pca(bits, wps, pc.E2E_SITES, k=pc.E2E_K, fit=fit)
    got = ctx.pcrelate_records(bits, wps, pc.E2E_SITES, scores=pca.scores[:, :pc.E2E_K],
                               fit=pca.fit, min_kinship=0.125)
    assert got.records.is_cuda and got.num_records == 30
    rows = got.sorted()
    rc.check_records(rows, (0, 132, 0, 132))
    assert rc.pair_set(rows) == {(min(i, j), max(i, j)) for i, j in related}
    # the same bytes as the matrix of the same model
    lo, hi = float(np.float32(0.01)), float(np.float32(1.0) - np.float32(0.01))
    d_x, d_beta = (torch.from_numpy(a).to(bits.device) for a in (got.x, got.beta))
    kin = ctx.pcrelate_matrix(bits, wps, pc.E2E_SITES, d_x, d_beta, lo, hi).cpu().numpy()
    rc.same_records(rows, rc.threshold_matrix(kin, (0, 132, 0, 132), 0.125))
    # accepted as they stand
    pairs = ctx.pcrelate_pairs(bits, wps, pc.E2E_SITES, got.records, model=got,
                               num_records=got.num_records)
    assert rc.pair_set(pairs.rows) == rc.pair_set(rows)
    assert (pairs.relationship() >= cuking_amd.pcrelate.FULL_SIBLING).all()
    chosen = ctx.unrelated_set(got.records, got.num_records, 132)
    kept = chosen.keep.cpu().numpy() == 1
    assert not any(kept[i] and kept[j] for i, j in related)
    # the default threshold is the third-degree cut-off, and a model is reused
    again = ctx.pcrelate_records(bits, wps, pc.E2E_SITES, model=got)
    assert again.min_kinship == float(np.float32(cuking_amd.KING_CUTOFFS[0]))
    assert rc.pair_set(again.sorted()) >= rc.pair_set(rows)
