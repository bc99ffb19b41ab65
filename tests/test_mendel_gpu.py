"""Mendelian errors on the GPU: the device rows, error masks and site counts against the host
twin's and the naive walk's bytes for every case and fuzz seed of mendel_cases.py and with both
paddings, the chunked wrapper, a second stream, split launches, duos against trios with a missing
parent, accumulating site counts, the refusals through the raw ABI, and the chain from
compute_king to confirmed trios on a small family cohort."""
import numpy as np
import pytest

import mendel_cases as mc

import cuking_amd
from cuking_amd import _lib, mendel, pcrelate
from cuking_amd.mendel import NO_PARENT

pytestmark = pytest.mark.gpu


def to_device(host):
    import torch
    return torch.from_numpy(np.ascontiguousarray(host).view(np.int64)).to("cuda:0")


def run_device(ctx, case, ones_padding=False, stream=None):
    """``(rows, error_bits, site_counts)`` of the two device calls, on the host."""
    inp = mc.inputs(case)
    rows, mask = ctx.mendel_errors_raw(to_device(inp.bits(ones_padding)), inp.wps, case.sites,
                                       inp.trios, error_bits=True, stream=stream)
    counts = mendel.site_counts_device(ctx, mask, stream=stream)
    if stream is not None:
        stream.synchronize()
    return (mendel.rows_to_host(rows), mask.cpu().numpy().view(np.uint64),
            counts.cpu().numpy().view(np.uint32))


def same(got, want):
    return all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(got, want))


@pytest.mark.parametrize("case", mc.CASES, ids=lambda c: c.name)
def test_device_equals_the_host_twin_and_the_naive_walk(ctx, case):
    want = mc.run_host(case)
    got = run_device(ctx, case)
    assert same(got, want), case.name
    mc.check_against(case, *got, "device")
    # all-ones padding beyond num_sites: the same bytes
    assert same(run_device(ctx, case, ones_padding=True), want), case.name
    # without the mask: the same rows
    inp = mc.inputs(case)
    rows, mask = ctx.mendel_errors_raw(to_device(inp.bits()), inp.wps, case.sites, inp.trios)
    assert mask is None and mendel.rows_to_host(rows).tobytes() == want[0].tobytes()


@pytest.mark.parametrize("seed", mc.FUZZ_SEEDS)
def test_device_fuzz(ctx, seed):
    case = mc.fuzz_case(seed)
    want = mc.run_host(case)
    for ones in (False, True):
        got = run_device(ctx, case, ones_padding=ones)
        assert same(got, want), case.name
        mc.check_against(case, *got, "device")


def test_the_chunked_wrapper(ctx):
    """A chunk of 1 trio, ragged chunks and one piece: the same bytes."""
    case = next(c for c in mc.CASES if c.name == "24 samples, 20 trios")
    inp = mc.inputs(case)
    bits = to_device(inp.bits())
    want_rows, _, want_counts = mc.reference(case)
    whole = ctx.mendel_errors(bits, inp.wps, case.sites, inp.trios, site_counts=True)
    assert isinstance(whole, cuking_amd.MendelErrors)
    assert whole.rows.tobytes() == want_rows.tobytes()
    assert whole.site_errors.dtype == np.uint32 and whole.site_errors.shape == (case.sites,)
    assert whole.site_errors.tobytes() == want_counts[:case.sites].tobytes()
    for chunk in (1, 3, 7, 19, 20, 64):
        got = ctx.mendel_errors(bits, inp.wps, case.sites, inp.trios, site_counts=True,
                                _chunk_trios=chunk)
        assert got.rows.tobytes() == whole.rows.tobytes(), chunk
        assert got.site_errors.tobytes() == whole.site_errors.tobytes(), chunk
    rows_only = ctx.mendel_errors(bits, inp.wps, case.sites, inp.trios)
    assert rows_only.site_errors is None and rows_only.rows.tobytes() == want_rows.tobytes()
    host = cuking_amd.mendel_errors_host(inp.bits(), inp.wps, case.sites, inp.trios,
                                         site_counts=True)
    assert host.rows.tobytes() == whole.rows.tobytes()
    assert host.site_errors.tobytes() == whole.site_errors.tobytes()
    assert whole.rate().tobytes() == host.rate().tobytes()
    assert whole.per_sample(case.samples).tolist() == host.per_sample(case.samples).tolist()
    # a device tensor as the list, and no trio at all
    listed = to_device_i32(inp.trios)
    again = ctx.mendel_errors(bits, inp.wps, case.sites, listed, site_counts=True)
    assert again.rows.tobytes() == whole.rows.tobytes()
    none = ctx.mendel_errors(bits, inp.wps, case.sites, [], site_counts=True)
    assert len(none.rows) == 0 and not none.site_errors.any()


def to_device_i32(trios):
    import torch
    return torch.from_numpy(np.ascontiguousarray(trios).view(np.int32)).to("cuda:0")


def test_a_second_stream_and_no_wait(ctx):
    import torch
    case = next(c for c in mc.CASES if c.name == "planted, a step and 65")
    want = mc.run_host(case)
    side = torch.cuda.Stream()
    for stream in (side, None, side):
        assert same(run_device(ctx, case, stream=stream), want)
    inp = mc.inputs(case)
    got = ctx.mendel_errors(to_device(inp.bits()), inp.wps, case.sites, inp.trios,
                            site_counts=True, stream=side, _chunk_trios=2)
    assert got.rows.tobytes() == want[0].tobytes()
    assert got.site_errors.tobytes() == want[2][:case.sites].tobytes()
    # the raw calls do not wait for the device
    bits = to_device(inp.bits())
    before = ctx.get_option("host_syncs")
    rows, mask = ctx.mendel_errors_raw(bits, inp.wps, case.sites, inp.trios, error_bits=True)
    counts = mendel.site_counts_device(ctx, mask)
    assert ctx.get_option("host_syncs") == before
    assert mendel.rows_to_host(rows).tobytes() == want[0].tobytes()
    assert counts.cpu().numpy().view(np.uint32).tobytes() == want[2].tobytes()


def test_launches_are_split(ctx):
    """A cap of one workgroup per launch: the bytes of the one launch."""
    case = next(c for c in mc.CASES if c.name == "a step and a spare word")
    want = mc.run_host(case)
    assert len(mc.inputs(case).trios) > 2 * 4 and mc.inputs(case).plane > 64
    ctx.set_option("max_launch_blocks", 1)
    try:
        got = run_device(ctx, case)
    finally:
        ctx.set_option("max_launch_blocks", 0)
    assert same(got, want) and want[2].sum() > 0


def test_a_duo_is_the_trio_with_a_missing_parent(ctx):
    """``called`` and ``errors`` of (c, f, NO_PARENT) are those of (c, f, m) with m's row missing
    everywhere -- but for ``called``, which a listed parent that is missing brings to 0."""
    case = next(c for c in mc.CASES if c.name == "24 samples, 20 trios")
    inp = mc.inputs(case)
    n = case.samples
    code = np.vstack([inp.code, np.full((1, case.sites), mc.MISSING, dtype=np.uint8)])
    bits = to_device(mc.pack_codes(code, inp.plane))
    children = np.arange(12, dtype=np.uint32)
    fathers = (children + 5) % n
    no = np.full(12, NO_PARENT, dtype=np.uint32)
    gone = np.full(12, n, dtype=np.uint32)       # the row that is missing everywhere
    for duo, trio in (((children, fathers, no), (children, fathers, gone)),
                      ((children, no, fathers), (children, gone, fathers))):
        a = ctx.mendel_errors(bits, inp.wps, case.sites, np.stack(duo, axis=1))
        b = ctx.mendel_errors(bits, inp.wps, case.sites, np.stack(trio, axis=1))
        assert a.errors.tobytes() == b.errors.tobytes() and a.total().sum() > 100
        assert not b.called.any() and (a.called > 0).all()
        # ... and called of the duo is what the child and the one parent are both called at
        both = ((inp.code[children] != mc.MISSING) &
                (inp.code[fathers] != mc.MISSING)).sum(axis=1)
        assert a.called.tolist() == both.tolist()


def test_site_counts_accumulate_over_two_calls(ctx):
    import torch
    case = next(c for c in mc.CASES if c.name == "random, 4097 sites")
    inp = mc.inputs(case)
    want = mc.reference(case)
    half = len(inp.trios) // 2
    bits = to_device(inp.bits())
    counts = torch.zeros(64 * inp.plane, dtype=torch.int32, device="cuda:0")
    for part in (inp.trios[:half], inp.trios[half:]):
        _, mask = ctx.mendel_errors_raw(bits, inp.wps, case.sites, part, error_bits=True)
        assert mendel.site_counts_device(ctx, mask, counts) is counts
    assert counts.cpu().numpy().view(np.uint32).tobytes() == want[2].tobytes()
    _, mask = ctx.mendel_errors_raw(bits, inp.wps, case.sites, inp.trios, error_bits=True)
    mendel.site_counts_device(ctx, mask, counts)
    assert counts.cpu().numpy().view(np.uint32).tolist() == (2 * want[2]).tolist()


def test_more_trios_than_a_wavefront_counts(ctx):
    """2500 trios of one mask: several chunks of workgroups per word column, and counts beyond
    the 504 a wavefront's counter holds.  Then a mask of one word for 4.2 million trios: the
    launch wants more than 504 trios per wavefront there and must not take them."""
    case = next(c for c in mc.CASES if c.name == "random, 127 sites")
    inp = mc.inputs(case)
    rng = np.random.default_rng(8)
    trios = rng.integers(0, case.samples, size=(2500, 3)).astype(np.uint32)
    got = ctx.mendel_errors(to_device(inp.bits()), inp.wps, case.sites, trios, site_counts=True)
    host = cuking_amd.mendel_errors_host(inp.bits(), inp.wps, case.sites, trios,
                                         site_counts=True)
    assert got.rows.tobytes() == host.rows.tobytes()
    assert got.site_errors.tobytes() == host.site_errors.tobytes() and got.site_errors.max() > 504
    count = 2048 * 4 * 504 + 70000
    mask = rng.integers(0, 1 << 64, size=(count, 1), dtype=np.uint64)
    mask &= rng.integers(0, 1 << 64, size=(count, 1), dtype=np.uint64)
    counts = mendel.site_counts_device(ctx, to_device(mask))
    assert counts.cpu().numpy().view(np.uint32).tobytes() == \
        mendel.site_counts_host(mask).tobytes()


# ---- the raw ABI ----------------------------------------------------------------------------------
def raw_trios(ctx, inp, **over):
    import torch
    out = torch.full((len(inp.trios), 12), 0x2B2B2B2B, dtype=torch.int32, device="cuda:0")
    mask = torch.full((len(inp.trios), inp.plane), 0x2C2C2C2C, dtype=torch.int64,
                      device="cuda:0")
    bits, trios = to_device(inp.bits()), to_device_i32(inp.trios)
    pointers = dict(bits=bits.data_ptr(), trios=trios.data_ptr(), out=out.data_ptr(),
                    error_bits=mask.data_ptr())
    st = ctx.lib.cuking_mendel_trios(ctx.handle, *mc.trio_arguments(inp, pointers, **over), None)
    torch.cuda.synchronize()
    return st, out.cpu().numpy(), mask.cpu().numpy()


@pytest.mark.parametrize("name", mc.TRIO_REFUSALS)
def test_device_refusals_leave_the_outputs_untouched(ctx, name):
    over, word = mc.TRIO_REFUSALS[name]
    st, out, mask = raw_trios(ctx, mc.inputs(mc.REFUSAL_CASE), **over)
    assert st == _lib.ERR_INVALID_ARGUMENT, name
    assert word in ctx.lib.cuking_last_error().decode()
    assert (out == 0x2B2B2B2B).all() and (mask == 0x2C2C2C2C).all()


@pytest.mark.parametrize("name", mc.SITE_REFUSALS)
def test_device_site_count_refusals(ctx, name):
    import torch
    over, word = mc.SITE_REFUSALS[name]
    inp = mc.inputs(mc.REFUSAL_CASE)
    mask = to_device(mc.reference(mc.REFUSAL_CASE)[1])
    counts = torch.full((64 * inp.plane,), 7, dtype=torch.int32, device="cuda:0")
    pointers = dict(error_bits=mask.data_ptr(), counts=counts.data_ptr())
    st = ctx.lib.cuking_mendel_site_counts(ctx.handle, *mc.site_arguments(inp, pointers, **over),
                                           None)
    torch.cuda.synchronize()
    assert st == _lib.ERR_INVALID_ARGUMENT, name
    assert word in ctx.lib.cuking_last_error().decode()
    assert (counts == 7).all()


def test_the_raw_call_and_a_null_context(ctx):
    inp = mc.inputs(mc.REFUSAL_CASE)
    want = mc.reference(mc.REFUSAL_CASE)
    st, out, mask = raw_trios(ctx, inp)
    assert st == _lib.OK
    assert np.ascontiguousarray(out).view(mendel.MENDEL_TRIO_DTYPE).tobytes() == want[0].tobytes()
    assert mask.view(np.uint64).tobytes() == want[1].tobytes()
    assert ctx.lib.cuking_mendel_trios(None, None, 0, 2, 0, None, 0, None, None, None) == \
        _lib.ERR_INVALID_ARGUMENT
    assert ctx.lib.cuking_mendel_site_counts(None, None, 0, 1, None, None) == \
        _lib.ERR_INVALID_ARGUMENT
    st, out, mask = raw_trios(ctx, inp, num_trios=0, trios=None, out=None, bits=None,
                              error_bits=None)
    assert st == _lib.OK and (out == 0x2B2B2B2B).all()
    with pytest.raises(ValueError, match="error_bits"):
        ctx.mendel_errors_raw(to_device(inp.bits()), inp.wps, 180, inp.trios,
                              error_bits=to_device(np.zeros((1, 1), dtype=np.uint64)))


# ---- end to end ----------------------------------------------------------------------------------
def test_from_king_records_to_confirmed_trios(ctx):
    """60 samples x 5000 sites, six families of two founders and three children:
    compute_king at the third-degree threshold -> ibd_segments(...).relationship() ->
    candidate_trios -> mendel_errors.  The candidates are exactly the 18 true trios and show no
    error; with one parent swapped for an unrelated sample a trio shows errors that need both
    parents (codes 1, 2, 5, 8)."""
    import torch
    from site_qc_cases import pack
    geno, true_trios = mc.e2e_cohort()
    n, m = geno.shape
    host_bits = pack(geno)
    bits, wps = to_device(host_bits), host_bits.shape[1]
    results = torch.zeros((4096, 6), dtype=torch.int32, device="cuda:0")
    index_flag = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    ctx.compute_king(cuking_amd.Submatrix(n), wps, bits, 0.0442, 4096, results, index_flag[0:1],
                     index_flag[1:2])
    count = int(index_flag[0])
    assert 0 < count < 4096 and int(index_flag[1]) == 0
    recs = ctx.ibd_segments(bits, wps, m, results, num_records=count)
    codes = recs.relationship()
    candidates = cuking_amd.candidate_trios(recs.pairs(), codes)
    print("records", count, "parent-child", int((codes == pcrelate.PARENT_CHILD).sum()),
          "candidates", len(candidates))
    assert candidates.tolist() == true_trios.tolist()
    got = ctx.mendel_errors(bits, wps, m, candidates, site_counts=True)
    assert not got.errors.any() and not got.site_errors.any()
    assert (got.called > 0.9 * m).all() and (got.rate() == 0).all()
    assert not got.per_sample(n).any()
    # one parent swapped for an unrelated sample
    swapped = candidates.copy()
    swapped[:, 2] = 30 + np.arange(len(swapped))
    bad = ctx.mendel_errors(bits, wps, m, swapped, site_counts=True)
    both = bad.errors[:, [0, 1, 4, 7]].sum(axis=1)
    print("errors that need both parents", both.tolist(), "rate", bad.rate().round(4).tolist())
    assert (both > 0).all() and (bad.rate() > 0.01).all()
    assert not bad.errors[:, [2, 5]].any()      # the true parent in the father column
    per = bad.per_sample(n)
    assert (per[30:30 + len(swapped)] > 0).all() and per[48:].sum() == 0
    host = cuking_amd.mendel_errors_host(host_bits, wps, m, swapped, site_counts=True)
    assert bad.rows.tobytes() == host.rows.tobytes()
    assert bad.site_errors.tobytes() == host.site_errors.tobytes()
