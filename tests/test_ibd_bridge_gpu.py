"""IBD segments with bridged breaks on the GPU: the device rows, bridged counts and sorted
segments against the host twin's bytes for every case and fuzz seed of ibd_bridge_cases.py,
bridge_sites = 0 against the strict call, a second stream and a second call, a reordered part of
the list, split launches, the refusals, the overflow and retry path, and the synthetic cohort
with genotyping errors."""
import ctypes as C

import numpy as np
import pytest

import ibd_bridge_cases as bc
import ibd_cases as ic
from test_ibd_bridge_host import E2E_BRIDGE, check_e2e_errors, decode, naive_pairs, with_errors
from test_ibd_host import E2E, e2e_cohort

import cuking_amd
from cuking_amd import _lib, ibd

pytestmark = pytest.mark.gpu


def _device_bits(inp, ones_padding=False):
    import torch
    return torch.from_numpy(inp.bits(ones_padding).view(np.int64)).to("cuda:0")


def run_device(ctx, case, ones_padding=False, stream=None, index=None, **kw):
    """``(rows, segments, bridged)`` of the device call, on the host."""
    inp = bc.inputs(case)
    rows, segments, found, bridged = ctx.ibd_segments_raw(
        _device_bits(inp, ones_padding), inp.wps, case.sites,
        inp.pairs if index is None else index, group=inp.group, pos=inp.pos,
        min_sites=case.min_sites, min_length=case.min_length, segments=True, stream=stream,
        bridge_sites=case.bridge, **kw)
    if stream is not None:
        stream.synchronize()
    return (ibd.rows_to_host(rows), ibd.segments_to_host(segments, found),
            ibd.bridged_to_host(bridged))


def same(got, want):
    return got[0].tobytes() == want[0].tobytes() and got[2].tobytes() == want[2].tobytes() and \
        ibd.sort_segments(got[1]).tobytes() == ibd.sort_segments(want[1]).tobytes()


def check_device(ctx, case):
    want = bc.run_host(case)
    got = run_device(ctx, case)
    assert got[2].dtype == np.uint32 and got[2].shape == want[2].shape
    assert same(got, want), case.name
    return got


@pytest.mark.parametrize("case", bc.CASES, ids=lambda c: c.name)
def test_device_equals_the_host_twin(ctx, case):
    rows, segments, bridged = check_device(ctx, case)
    bc.check_against(case, rows, segments, bridged, "device")
    # all-ones padding beyond num_sites: the same bytes
    assert same(run_device(ctx, case, ones_padding=True), (rows, segments, bridged))


@pytest.mark.parametrize("seed", bc.FUZZ_SEEDS)
def test_device_fuzz(ctx, seed):
    check_device(ctx, bc.fuzz_case(seed))


@pytest.mark.parametrize("case", ic.CASES, ids=lambda c: c.name)
def test_bridge_sites_zero_is_the_strict_call(ctx, case):
    """cuking_ibd_pairs_bridged at bridge_sites = 0: the bytes of cuking_ibd_pairs."""
    import torch
    inp = ic.inputs(case)
    bits = _device_bits(inp)
    want_rows, want_segments, want_found = ctx.ibd_segments_raw(
        bits, inp.wps, case.sites, inp.pairs, group=inp.group, pos=inp.pos,
        min_sites=case.min_sites, min_length=case.min_length, segments=True)
    dev = lambda a: None if a is None else \
        torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to("cuda:0")  # noqa: E731
    pairs, group, pos = dev(inp.pairs), dev(inp.group), dev(inp.pos)
    out = torch.zeros((len(inp.index), 10), dtype=torch.int32, device="cuda:0")
    bridged = torch.full((len(inp.index), 2), 7, dtype=torch.int32, device="cuda:0")
    segments = torch.zeros((max(1, want_found), 4), dtype=torch.int32, device="cuda:0")
    found = C.c_uint64(0)
    st = ctx.lib.cuking_ibd_pairs_bridged(
        ctx.handle, bits.data_ptr(), case.samples, inp.wps, case.sites,
        None if group is None else group.data_ptr(), None if pos is None else pos.data_ptr(),
        case.min_sites, case.min_length, 0, pairs.data_ptr(), len(inp.index), case.stride,
        out.data_ptr(), bridged.data_ptr(), segments.data_ptr(), segments.shape[0],
        C.byref(found), None)
    torch.cuda.synchronize()
    assert st == _lib.OK and found.value == want_found
    assert ibd.rows_to_host(out).tobytes() == ibd.rows_to_host(want_rows).tobytes()
    assert not bridged.cpu().numpy().any()
    assert ibd.sort_segments(ibd.segments_to_host(segments, want_found)).tobytes() == \
        ibd.sort_segments(ibd.segments_to_host(want_segments, want_found)).tobytes()


def test_a_second_stream_a_second_call_and_a_reordered_part(ctx):
    import torch
    case = next(c for c in bc.CASES if c.name.startswith("breaks at bit 63"))
    first = run_device(ctx, case)
    assert first[2].any()
    side = torch.cuda.Stream()
    for stream in (side, None, side):
        assert same(run_device(ctx, case, stream=stream), first)
    # without the list: the same rows and bridged counts, no count
    inp = bc.inputs(case)
    rows, segments, found, bridged = ctx.ibd_segments_raw(
        _device_bits(inp), inp.wps, case.sites, inp.pairs, min_sites=case.min_sites,
        bridge_sites=case.bridge)
    assert segments is None and found == 0
    assert ibd.rows_to_host(rows).tobytes() == first[0].tobytes()
    assert ibd.bridged_to_host(bridged).tobytes() == first[2].tobytes()
    # a row depends on its own pair only: a part of the list, reordered
    order = np.random.default_rng(4).permutation(len(inp.index))[:15]
    rows, _, moved = run_device(ctx, case, index=np.ascontiguousarray(inp.index[order]))
    assert rows.tobytes() == first[0][order].tobytes()
    assert moved.tobytes() == first[2][order].tobytes()
    # the wrapper
    got = ctx.ibd_segments(_device_bits(inp), inp.wps, case.sites, inp.pairs,
                           min_sites=case.min_sites, bridge_sites=case.bridge)
    assert got.bridge_sites == case.bridge and got.bridged.tobytes() == first[2].tobytes()
    assert got.rows.tobytes() == first[0].tobytes()


def test_launches_are_split(ctx):
    """A cap of one workgroup per launch: the bytes of the one launch."""
    case = next(c for c in bc.CASES if c.name.startswith("five breaks 70 sites apart, 64"))
    assert len(bc.inputs(case).index) > 2 * 4
    want = run_device(ctx, case)
    ctx.set_option("max_launch_blocks", 1)
    try:
        got = run_device(ctx, case)
    finally:
        ctx.set_option("max_launch_blocks", 0)
    assert same(got, want) and len(want[1]) > 0 and want[2].sum() >= 10


def _raw_device(ctx, inp, bridge_sites, null_bridged=False, **over):
    """cuking_ibd_pairs_bridged with single arguments replaced; returns (status, out, bridged,
    found)."""
    import torch
    out = torch.full((len(inp.index), 10), 0x2B2B2B2B, dtype=torch.int32, device="cuda:0")
    bridged = torch.full((len(inp.index), 2), 0x2B2B2B2B, dtype=torch.int32, device="cuda:0")
    segments = torch.zeros((16, 4), dtype=torch.int32, device="cuda:0")
    bits = _device_bits(inp)
    pairs = torch.from_numpy(np.ascontiguousarray(inp.pairs).view(np.int32)).to("cuda:0")
    found = C.c_uint64(77)
    pointers = dict(bits=bits.data_ptr(), group=None, pos=None, pairs=pairs.data_ptr(),
                    out=out.data_ptr(), segments=segments.data_ptr(), found=C.byref(found),
                    bridged=None if null_bridged else bridged.data_ptr())
    st = ctx.lib.cuking_ibd_pairs_bridged(
        ctx.handle, *bc.bridged_arguments(inp, pointers, bridge_sites, **over), None)
    torch.cuda.synchronize()
    return st, out.cpu().numpy(), bridged.cpu().numpy(), found.value


@pytest.mark.parametrize("name", list(ic.REFUSALS) + ["bridge_sites 1", "bridge_sites 63"])
def test_device_refusals_leave_the_outputs_untouched(ctx, name):
    inp = ic.inputs(ic.REFUSAL_CASE)
    if name.startswith("bridge_sites"):
        st, out, bridged, _ = _raw_device(ctx, inp, int(name.split()[1]))
        assert "bridge_sites" in ctx.lib.cuking_last_error().decode()
    else:
        st, out, bridged, _ = _raw_device(ctx, inp, 64, **ic.REFUSALS[name])
    assert st == _lib.ERR_INVALID_ARGUMENT, name
    assert (out == 0x2B2B2B2B).all() and (bridged == 0x2B2B2B2B).all()


def test_a_null_bridged_is_accepted(ctx):
    case = bc.CASES[0]
    inp = bc.inputs(case)
    want_rows, want_bridged, want_segments = bc.reference(case)
    over = dict(min_sites=case.min_sites)
    st, out, bridged, found = _raw_device(ctx, inp, case.bridge, **over)
    assert st == _lib.OK and found == len(want_segments)
    assert np.ascontiguousarray(out).view(ibd.IBD_PAIR_DTYPE).tobytes() == want_rows.tobytes()
    assert bridged.view(np.uint32).tobytes() == want_bridged.tobytes()
    st, again, bridged, found = _raw_device(ctx, inp, case.bridge, null_bridged=True, **over)
    assert st == _lib.OK and found == len(want_segments)
    assert again.tobytes() == out.tobytes() and (bridged == 0x2B2B2B2B).all()


def test_overflow_and_retry(ctx):
    case = next(c for c in bc.CASES if c.name.startswith("sixteen samples"))
    want = bc.run_host(case)
    total = len(want[1])
    assert total > 8
    assert same(run_device(ctx, case, max_segments=total), want)
    for room in (total - 1, 0):
        with pytest.raises(cuking_amd.ResourceExhaustedError) as e:
            run_device(ctx, case, max_segments=room)
        assert e.value.num_segments == total
    # the wrapper grows its default buffer once: more than four segments per pair
    inp = bc.inputs(case)
    selfs = np.array([[0, 0]] * 2, dtype=np.uint32)
    group = (np.arange(case.sites) // 300).astype(np.int32)
    before = ctx.get_option("host_syncs")
    got = ctx.ibd_segments(_device_bits(inp), inp.wps, case.sites, selfs, group=group,
                           min_sites=case.min_sites, segments=True, bridge_sites=case.bridge)
    assert ctx.get_option("host_syncs") - before == 2   # (two calls, each reads its count)
    assert len(got.segments) == 40 > 4 * 2 and not got.bridged.any()


def test_the_cohort_with_genotyping_errors(ctx):
    """The cohort of smoke() with errors in its related pairs (test_ibd_bridge_host.py has the
    rate and how it was chosen): the strict call loses relationships, the bridged call gives
    every error-free one, and the device gives the host twin's bytes."""
    import torch
    from cuking_amd.synth import cohort_to_device
    n, m, seed = E2E
    cohort, index, labels = e2e_cohort()
    kind, pa, pb = cohort_to_device(cohort)
    clean_bits = ctx.synth_bitset(seed, kind, pa, pb, 0, n, m)
    wps = clean_bits.shape[1]
    clean = decode(clean_bits.cpu().numpy().view(np.uint64), m)
    noisy = with_errors(clean, index, labels)
    host_bits = ic.pack_codes(noisy, wps // 2, ones_padding=True)
    bits = torch.from_numpy(host_bits.view(np.int64)).to("cuda:0")
    strict = ctx.ibd_segments(bits, wps, m, index)
    bridged = ctx.ibd_segments(bits, wps, m, index, segments=True, bridge_sites=E2E_BRIDGE)
    check_e2e_errors(naive_pairs(clean, index, 0), strict, bridged, labels)
    host = cuking_amd.ibd_segments_host(host_bits, wps, m, index, segments=True,
                                        bridge_sites=E2E_BRIDGE)
    assert bridged.rows.tobytes() == host.rows.tobytes()
    assert bridged.bridged.tobytes() == host.bridged.tobytes()
    assert bridged.sorted().tobytes() == host.sorted().tobytes()
