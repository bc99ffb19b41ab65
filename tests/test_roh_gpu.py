"""Runs of homozygosity on the GPU: the device rows and sorted segments against the host twin's
bytes for every case and fuzz seed of roh_cases.py and with ones-padding, a second stream and a
second call, the call without a list, split launches, the cross-check through the IBD kernel, the
overflow and retry path, the refusals through the raw ABI, and the end-to-end cohort."""
import ctypes as C

import numpy as np
import pytest

import roh_cases as rc
from test_roh_host import bridges_of, check_ibd_twin, ibd_twin_inputs

import cuking_amd
from cuking_amd import _lib, ibd, roh

pytestmark = pytest.mark.gpu


def to_device(host):
    import torch
    return torch.from_numpy(np.ascontiguousarray(host).view(np.int64)).to("cuda:0")


def run_device(ctx, case, ones_padding=False, stream=None, bridge=None, listed=True, **kw):
    """``(rows, segments)`` of the device call, on the host."""
    inp = rc.inputs(case)
    kw.setdefault("segments", True)
    rows, segments, found = ctx.roh_segments_raw(
        to_device(inp.bits(ones_padding)), inp.wps, case.sites, inp.listed if listed else None,
        group=inp.group, pos=inp.pos, min_sites=case.min_sites, min_length=case.min_length,
        bridge_sites=case.bridge if bridge is None else bridge, stream=stream, **kw)
    if stream is not None:
        stream.synchronize()
    return roh.rows_to_host(rows), \
        None if segments is None else ibd.segments_to_host(segments, found)


def same(got, want):
    return got[0].tobytes() == want[0].tobytes() and \
        rc.sort_rows(got[1]).tobytes() == rc.sort_rows(want[1]).tobytes()


@pytest.mark.parametrize("case", rc.CASES, ids=lambda c: c.name)
def test_device_equals_the_host_twin(ctx, case):
    for bridge in bridges_of(case):
        want = rc.run_host(case, bridge=bridge)
        got = run_device(ctx, case, bridge=bridge)
        assert got[0].dtype == roh.ROH_SAMPLE_DTYPE and same(got, want), (case.name, bridge)
        rc.check_against(case, *got, "device", bridge)
        # all-ones padding beyond num_sites: the same bytes
        assert same(run_device(ctx, case, ones_padding=True, bridge=bridge), want)


@pytest.mark.parametrize("seed", rc.FUZZ_SEEDS)
def test_device_fuzz(ctx, seed):
    case = rc.fuzz_case(seed)
    want = rc.run_host(case)
    assert same(run_device(ctx, case), want), case.name
    assert same(run_device(ctx, case, ones_padding=True), want), case.name


def test_a_second_stream_a_second_call_and_no_list(ctx):
    import torch
    case = next(c for c in rc.CASES if c.name.startswith("hets at bit 63"))
    first = run_device(ctx, case)
    assert first[0]["bridged"].any() and same(first, rc.run_host(case))
    side = torch.cuda.Stream()
    for stream in (side, None, side):
        assert same(run_device(ctx, case, stream=stream), first)
    # without the segment list: the same rows, no count, and no wait for the device
    inp = rc.inputs(case)
    before = ctx.get_option("host_syncs")
    rows, segments, found = ctx.roh_segments_raw(
        to_device(inp.bits()), inp.wps, case.sites, inp.listed, min_sites=case.min_sites,
        bridge_sites=case.bridge)
    assert ctx.get_option("host_syncs") == before
    assert segments is None and found == 0
    assert roh.rows_to_host(rows).tobytes() == first[0].tobytes()
    # the null list against the explicit list of every sample, and a device tensor as the list
    null = run_device(ctx, case, listed=False)
    everyone = torch.arange(case.samples, dtype=torch.int32, device="cuda:0")
    rows, segments, found = ctx.roh_segments_raw(
        to_device(inp.bits()), inp.wps, case.sites, everyone, min_sites=case.min_sites,
        bridge_sites=case.bridge, segments=True)
    assert same((roh.rows_to_host(rows), ibd.segments_to_host(segments, found)), null)
    assert same(null, rc.run_host(case, listed=False))
    # the wrapper
    got = ctx.roh_segments(to_device(inp.bits()), inp.wps, case.sites, inp.listed,
                           min_sites=case.min_sites, bridge_sites=case.bridge, segments=True)
    assert got.bridge_sites == case.bridge and got.rows.tobytes() == first[0].tobytes()
    assert got.total_length == case.sites - 1
    assert got.sorted().tobytes() == rc.sort_rows(first[1]).tobytes()


def test_launches_are_split(ctx):
    """A cap of one workgroup per launch: the bytes of the one launch."""
    case = next(c for c in rc.CASES if c.samples > 8)
    assert len(rc.inputs(case).listed) > 2 * 4
    for listed in (True, False):
        want = run_device(ctx, case, listed=listed)
        ctx.set_option("max_launch_blocks", 1)
        try:
            got = run_device(ctx, case, listed=listed)
        finally:
            ctx.set_option("max_launch_blocks", 0)
        assert same(got, want) and len(want[1]) > 0 and want[0]["bridged"].sum() >= 3
        assert same(want, rc.run_host(case, listed=listed))


def test_kind_2_of_the_ibd_kernel_on_a_shadow_row_is_the_roh_row(ctx):
    """The cross-check of test_roh_host.py through the IBD kernel, on the device, for one case."""
    case = next(c for c in rc.CASES if c.name.startswith("two steps and 37 sites"))
    inp, bits, pairs = ibd_twin_inputs(case)
    kw = dict(group=inp.group, pos=inp.pos, min_sites=case.min_sites, min_length=case.min_length)
    for bridge in (0, 64):
        mine = roh.rows_to_host(ctx.roh_segments_raw(to_device(inp.bits()), inp.wps, case.sites,
                                                     bridge_sites=bridge, **kw)[0])
        theirs = ctx.ibd_segments(to_device(bits), inp.wps, case.sites, pairs,
                                  bridge_sites=bridge, **kw)
        bridged = theirs.bridged if bridge else np.zeros((case.samples, 2), dtype=np.uint32)
        check_ibd_twin(case, mine, theirs.rows, bridged)
        assert mine["segments"].sum() >= 6 and (bridge == 0 or mine["bridged"].sum() == 3)


def test_overflow_and_retry(ctx):
    case = next(c for c in rc.CASES if c.name == "every word a group")
    want = rc.run_host(case)
    total = len(want[1])
    assert total > 16
    assert same(run_device(ctx, case, max_segments=total), want)
    for room in (total - 1, 0):
        with pytest.raises(cuking_amd.ResourceExhaustedError) as e:
            run_device(ctx, case, max_segments=room)
        assert e.value.num_segments == total
    # the wrapper grows its default buffer once: ten segments of one sample, four fit
    inp = rc.inputs(case)
    before = ctx.get_option("host_syncs")
    got = ctx.roh_segments(to_device(inp.bits()), inp.wps, case.sites, [0], group=inp.group,
                           min_sites=case.min_sites, segments=True)
    assert ctx.get_option("host_syncs") - before == 2   # (two calls, each reads its count)
    assert len(got.segment_list) == got.segments[0] == 10 > 4


def raw_device(ctx, inp, **over):
    """cuking_roh_samples with single arguments replaced: (status, out, found)."""
    import torch
    count = inp.case.samples if inp.listed is None else len(inp.listed)
    out = torch.full((count, 6), 0x2B2B2B2B, dtype=torch.int32, device="cuda:0")
    segments = torch.zeros((16, 4), dtype=torch.int32, device="cuda:0")
    bits = to_device(inp.bits())
    samples = torch.from_numpy(inp.listed.view(np.int32)).to("cuda:0")
    found = C.c_uint64(77)
    keep = []
    if over.get("pos") == "decreasing":
        pos = np.arange(inp.case.sites, dtype=np.int32)
        pos[100] = 5
        keep.append(torch.from_numpy(pos).to("cuda:0"))
        over = dict(over, pos=keep[0].data_ptr())
    pointers = dict(bits=bits.data_ptr(), group=None, pos=None, samples=samples.data_ptr(),
                    out=out.data_ptr(), segments=segments.data_ptr(), found=C.byref(found))
    st = ctx.lib.cuking_roh_samples(ctx.handle, *rc.raw_arguments(inp, pointers, **over), None)
    torch.cuda.synchronize()
    return st, out.cpu().numpy(), found.value


@pytest.mark.parametrize("name", rc.REFUSALS)
def test_device_refusals_leave_the_outputs_untouched(ctx, name):
    over, status, word = rc.REFUSALS[name]
    inp = rc.inputs(rc.REFUSAL_CASE)
    st, out, _ = raw_device(ctx, inp, **over)
    want = _lib.ERR_INVALID_ARGUMENT if status == "INVALID" else _lib.ERR_FAILED_PRECONDITION
    assert st == want, name
    assert word in ctx.lib.cuking_last_error().decode()
    assert (out == 0x2B2B2B2B).all()


def test_the_raw_call_and_a_null_context(ctx):
    inp = rc.inputs(rc.REFUSAL_CASE)
    want_rows, want_segments = rc.reference(rc.REFUSAL_CASE)
    st, out, found = raw_device(ctx, inp)
    assert st == _lib.OK and found == len(want_segments) > 0
    assert np.ascontiguousarray(out).view(roh.ROH_SAMPLE_DTYPE).tobytes() == want_rows.tobytes()
    st = ctx.lib.cuking_roh_samples(None, None, 0, 0, 0, None, None, 0, 0, 0, None, 0, None, None,
                                    0, None, None)
    assert st == _lib.ERR_INVALID_ARGUMENT
    st, out, found = raw_device(ctx, inp, num_samples=0, samples=None, out=None, bits=None)
    assert st == _lib.OK and found == 0 and (out == 0x2B2B2B2B).all()


def test_the_end_to_end_cohort(ctx):
    """The cohort of test_roh_host.py through KingContext.roh_segments: the three conditions, and
    the host twin's bytes."""
    code, group, stretches = rc.e2e_cohort()
    m = rc.E2E_SITES
    host_bits = rc.pack_codes(code, -(-m // 64), ones_padding=True)
    bits, wps = to_device(host_bits), host_bits.shape[1]
    kw = dict(group=group, min_sites=rc.E2E_MIN_SITES, segments=True)
    strict = ctx.roh_segments(bits, wps, m, **kw)
    bridged = ctx.roh_segments(bits, wps, m, bridge_sites=rc.E2E_BRIDGE, **kw)
    rc.check_e2e(strict, bridged, stretches)
    for got, bridge in ((strict, 0), (bridged, rc.E2E_BRIDGE)):
        host = cuking_amd.roh_segments_host(host_bits, wps, m, bridge_sites=bridge, **kw)
        assert got.rows.tobytes() == host.rows.tobytes()
        assert got.sorted().tobytes() == host.sorted().tobytes()
        assert got.total_length == host.total_length and \
            got.froh().tobytes() == host.froh().tobytes()
