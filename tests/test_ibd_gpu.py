"""IBD segments for listed pairs on the GPU: the device rows and sorted segments against the host
twin's bytes for every case and fuzz seed of ibd_cases.py, a second stream and a second call, a
compute_king record buffer on the device, the refusals through the raw ABI, the overflow and
retry path of the wrapper, and the relationships of the synthetic cohort's records."""
import ctypes as C

import numpy as np
import pytest

import ibd_cases as ic
from test_ibd_host import E2E, check_e2e, e2e_cohort

import cuking_amd
from cuking_amd import _lib, ibd
from cuking_amd import pcrelate as pcr

pytestmark = pytest.mark.gpu


def _device_bits(inp, ones_padding=False):
    import torch
    return torch.from_numpy(inp.bits(ones_padding).view(np.int64)).to("cuda:0")


def run_device(ctx, case, ones_padding=False, stream=None, **kw):
    inp = ic.inputs(case)
    rows, segments, found = ctx.ibd_segments_raw(
        _device_bits(inp, ones_padding), inp.wps, case.sites, inp.pairs, group=inp.group,
        pos=inp.pos, min_sites=case.min_sites, min_length=case.min_length, segments=True,
        stream=stream, **kw)
    if stream is not None:
        stream.synchronize()
    return ibd.rows_to_host(rows), ibd.segments_to_host(segments, found)


def check_device(ctx, case):
    want_rows, want_segments = ic.run_host(case)
    rows, segments = run_device(ctx, case)
    assert rows.tobytes() == want_rows.tobytes(), case.name
    assert ibd.sort_segments(segments).tobytes() == ibd.sort_segments(want_segments).tobytes()
    return rows, segments


@pytest.mark.parametrize("case", ic.CASES, ids=lambda c: c.name)
def test_device_equals_the_host_twin(ctx, case):
    rows, segments = check_device(ctx, case)
    ic.check_against(case, rows, segments, "device")
    # all-ones padding beyond num_sites: the same bytes
    padded_rows, padded_segments = run_device(ctx, case, ones_padding=True)
    assert padded_rows.tobytes() == rows.tobytes()
    assert ibd.sort_segments(padded_segments).tobytes() == ibd.sort_segments(segments).tobytes()


@pytest.mark.parametrize("seed", ic.FUZZ_SEEDS)
def test_device_fuzz(ctx, seed):
    check_device(ctx, ic.fuzz_case(seed))


def test_a_second_stream_and_a_second_call_give_the_same_bytes(ctx):
    import torch
    case = next(c for c in ic.CASES if c.name.startswith("two steps"))
    first_rows, first_segments = run_device(ctx, case)
    side = torch.cuda.Stream()
    for stream in (side, None, side):
        rows, segments = run_device(ctx, case, stream=stream)
        assert rows.tobytes() == first_rows.tobytes()
        assert ibd.sort_segments(segments).tobytes() == ibd.sort_segments(first_segments).tobytes()
    # without the list: the same rows, no count
    inp = ic.inputs(case)
    rows, segments, found = ctx.ibd_segments_raw(
        _device_bits(inp), inp.wps, case.sites, inp.pairs, group=inp.group, pos=inp.pos,
        min_sites=case.min_sites, min_length=case.min_length)
    assert segments is None and found == 0
    assert ibd.rows_to_host(rows).tobytes() == first_rows.tobytes()
    # a row depends on its own pair only: a part of the list, reordered
    order = np.random.default_rng(4).permutation(len(inp.index))[:15]
    rows, _, _ = ctx.ibd_segments_raw(
        _device_bits(inp), inp.wps, case.sites, np.ascontiguousarray(inp.index[order]),
        group=inp.group, pos=inp.pos, min_sites=case.min_sites, min_length=case.min_length)
    assert ibd.rows_to_host(rows).tobytes() == first_rows[order].tobytes()


def test_the_waits_of_one_call(ctx):
    """One raw call waits once, for its count, and without a list not at all (no positions: no
    check of them to wait for)."""
    case = next(c for c in ic.CASES if c.name.startswith("two steps"))
    inp = ic.inputs(case)
    bits = _device_bits(inp)
    for kw, want in ((dict(max_segments=1 << 16), 1), (dict(), 0)):
        before = ctx.get_option("host_syncs")
        _, segments, found = ctx.ibd_segments_raw(bits, inp.wps, case.sites, inp.index,
                                                  min_sites=case.min_sites, **kw)
        assert ctx.get_option("host_syncs") - before == want
        assert (segments is not None) == bool(want) and (want or found == 0)


def test_launches_are_split(ctx):
    """A cap of one workgroup per launch sends the 15 pairs (four to a workgroup) out in four
    launches, three of them with a pair base above 0: the bytes of the one launch."""
    case = next(c for c in ic.CASES if c.name.startswith("every word a group"))
    assert len(ic.inputs(case).index) > 2 * 4
    want_rows, want_segments = run_device(ctx, case)
    ctx.set_option("max_launch_blocks", 1)
    try:
        rows, segments = run_device(ctx, case)
    finally:
        ctx.set_option("max_launch_blocks", 0)
    assert np.array_equal(rows.view(np.uint8), want_rows.view(np.uint8))
    assert np.array_equal(ibd.sort_segments(segments).view(np.uint8),
                          ibd.sort_segments(want_segments).view(np.uint8))
    assert len(want_segments) > 0


def test_zero_sites_and_an_empty_list(ctx):
    import torch
    inp = ic.inputs(ic.REFUSAL_CASE)
    rows, segments, found = ctx.ibd_segments_raw(_device_bits(inp), inp.wps, 0, inp.index,
                                                 segments=True)
    rows = ibd.rows_to_host(rows)
    assert found == 0 and np.array_equal(rows["sample_j"], inp.index[:, 1])
    for name in ibd.IBD_PAIR_DTYPE.names[2:]:
        assert not rows[name].any()
    rows, _, found = ctx.ibd_segments_raw(_device_bits(inp), inp.wps, ic.REFUSAL_CASE.sites,
                                          torch.zeros((0, 2), dtype=torch.int32, device="cuda:0"),
                                          segments=True)
    assert tuple(rows.shape) == (0, 10) and found == 0


def _raw_device(ctx, inp, **over):
    """cuking_ibd_pairs with single arguments replaced; returns (status, out, found)."""
    import torch
    out = torch.full((len(inp.index), 10), 0x2B2B2B2B, dtype=torch.int32, device="cuda:0")
    segments = torch.zeros((16, 4), dtype=torch.int32, device="cuda:0")
    bits = _device_bits(inp)
    pairs = torch.from_numpy(np.ascontiguousarray(inp.pairs).view(np.int32)).to("cuda:0")
    found = C.c_uint64(77)
    pointers = dict(bits=bits.data_ptr(), group=None, pos=None, pairs=pairs.data_ptr(),
                    out=out.data_ptr(), segments=segments.data_ptr(), found=C.byref(found))
    st = ctx.lib.cuking_ibd_pairs(ctx.handle, *ic.raw_arguments(inp, pointers, **over), None)
    torch.cuda.synchronize()
    return st, out.cpu().numpy(), found.value


@pytest.mark.parametrize("name", ic.REFUSALS)
def test_device_refusals_leave_out_untouched(ctx, name):
    inp = ic.inputs(ic.REFUSAL_CASE)
    st, out, _ = _raw_device(ctx, inp, **ic.REFUSALS[name])
    assert st == _lib.ERR_INVALID_ARGUMENT, name
    assert (out == 0x2B2B2B2B).all()
    st, out, found = _raw_device(ctx, inp)
    want_rows, want_segments = ic.reference(ic.REFUSAL_CASE)
    assert st == _lib.OK and found == len(want_segments)
    assert np.ascontiguousarray(out).view(ibd.IBD_PAIR_DTYPE).tobytes() == want_rows.tobytes()


def test_device_positions_must_not_decrease(ctx):
    case = ic.REFUSAL_CASE
    inp = ic.inputs(case)
    pos = np.arange(case.sites, dtype=np.uint32) * 3
    pos[100] = 7
    with pytest.raises(cuking_amd.CukingError, match=r"pos\[100\] = 7 follows") as e:
        ctx.ibd_segments_raw(_device_bits(inp), inp.wps, case.sites, inp.index, pos=pos)
    assert e.value.status == _lib.ERR_FAILED_PRECONDITION
    group = (np.arange(case.sites) >= 100).astype(np.int32)
    rows, _, _ = ctx.ibd_segments_raw(_device_bits(inp), inp.wps, case.sites, inp.index, pos=pos,
                                      group=group)
    want, _ = ibd.ibd_segments_raw_host(inp.bits(), inp.wps, case.sites, inp.index, pos=pos,
                                        group=group)
    assert ibd.rows_to_host(rows).tobytes() == want.tobytes()


def test_overflow_and_retry(ctx):
    case = next(c for c in ic.CASES if c.name.startswith("group boundaries"))
    want_rows, want_segments = ic.run_host(case)
    total = len(want_segments)
    rows, segments = run_device(ctx, case, max_segments=total)
    assert ibd.sort_segments(segments).tobytes() == ibd.sort_segments(want_segments).tobytes()
    for room in (total - 1, 0):
        with pytest.raises(cuking_amd.ResourceExhaustedError) as e:
            run_device(ctx, case, max_segments=room)
        assert e.value.num_segments == total
    # the wrapper grows its default buffer once: more than four segments per pair
    inp = ic.inputs(case)
    one = np.array([inp.index[0]] * 2, dtype=np.uint32)
    before = ctx.get_option("host_syncs")
    got = ctx.ibd_segments(_device_bits(inp), inp.wps, case.sites, one, group=inp.group,
                           min_sites=case.min_sites, segments=True)
    assert ctx.get_option("host_syncs") - before == 2   # (two calls, each reads its count)
    assert len(got.segments) == 16 and got.sorted()["pair"].tolist() == [0] * 8 + [1] * 8
    assert got.rows.tobytes() == want_rows[[0, 0]].tobytes()


def test_the_records_of_compute_king_on_the_device(ctx):
    """The synthetic cohort: compute_king's record buffer, on the device, is the list."""
    import torch
    from cuking_amd.synth import cohort_to_device
    n, m, seed = E2E
    cohort, index, labels = e2e_cohort()
    kind, pa, pb = cohort_to_device(cohort)
    bits = ctx.synth_bitset(seed, kind, pa, pb, 0, n, m)
    wps = bits.shape[1]
    # the listed pairs against the host twin, and their relationships
    got = ctx.ibd_segments(bits, wps, m, index, segments=True)
    check_e2e(got, labels)
    host = cuking_amd.ibd_segments_host(bits.cpu().numpy().view(np.uint64), wps, m, index,
                                        segments=True)
    assert got.rows.tobytes() == host.rows.tobytes()
    assert got.sorted().tobytes() == host.sorted().tobytes()
    # the record buffer of compute_king as it lies on the device
    sm = cuking_amd.Submatrix(n)
    results = torch.zeros((4096, 6), dtype=torch.int32, device="cuda:0")
    index_flag = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    ctx.compute_king(sm, wps, bits, 0.177, 4096, results, index_flag[0:1], index_flag[1:2])
    count = int(index_flag[0])
    assert 0 < count < 4096 and int(index_flag[1]) == 0
    recs = ctx.ibd_segments(bits, wps, m, results, num_records=count)
    pairs = {(int(i), int(j)): k for k, (i, j) in enumerate(zip(recs.sample_i, recs.sample_j))}
    codes = recs.relationship()
    for (a, b), what in zip(index, labels):
        if what == "none":
            continue
        k = pairs[(min(a, b), max(a, b))]
        assert codes[k] == (pcr.DUPLICATE if what == "dup" else pcr.PARENT_CHILD)
    host = cuking_amd.ibd_segments_host(bits.cpu().numpy().view(np.uint64), wps, m,
                                        results[:count].cpu().numpy())
    assert recs.rows.tobytes() == host.rows.tobytes()
