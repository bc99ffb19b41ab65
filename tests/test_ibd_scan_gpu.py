"""IBD scan of a block on the GPU: the device records, sorted by (i, j), against the host twin's
bytes for every case and fuzz seed of ibd_cases.py and for every block of the 70-sample cohort
of ibd_scan_cases.py (diagonal, off-diagonal and partial tiles in one launch, up to four LDS
chunks and 37 sites), with all-ones padding, on a second stream and in a second call, with one
workgroup per launch; the scan against ``ctx.ibd_segments`` on its own pairs; overflow, retry,
the counting call and the number of waits; the refusals through the raw ABI; the end-to-end
cohort."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import ibd_cases as ic
import ibd_scan_cases as sc
from test_ibd_host import E2E, e2e_cohort

import cuking_amd
from cuking_amd import _lib, ibd
from cuking_amd import pcrelate as pcr

pytestmark = pytest.mark.gpu


def _device(bits):
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int64)).to("cuda:0")


def scan_device(ctx, bits, wps, sites, group, pos, min_sites, min_length, stream=None, **kw):
    """The device records of one call, sorted by (i, j)."""
    recs, count = ctx.ibd_scan_raw(_device(bits), wps, sites, group=group, pos=pos,
                                   min_sites=min_sites, min_length=min_length, stream=stream, **kw)
    if stream is not None:
        stream.synchronize()
    return ibd.records_to_host(recs, count)


def scan_case_device(ctx, case, ones_padding=False, **kw):
    inp = ic.inputs(case)
    return scan_device(ctx, inp.bits(ones_padding), inp.wps, case.sites, inp.group, inp.pos,
                       case.min_sites, case.min_length, **kw)


@lru_cache(maxsize=None)
def host_case(case):
    return sc.scan_case(case)[0]


def check_case(ctx, case):
    want = host_case(case)
    got = scan_case_device(ctx, case)
    assert got.tobytes() == want.tobytes(), case.name
    # all-ones padding beyond num_sites: the same bytes
    assert scan_case_device(ctx, case, ones_padding=True).tobytes() == want.tobytes(), case.name
    return got


@pytest.mark.parametrize("case", ic.CASES, ids=lambda c: c.name)
def test_device_equals_the_host_twin(ctx, case):
    sc.check_reference(case, check_case(ctx, case))


@pytest.mark.parametrize("seed", ic.FUZZ_SEEDS)
def test_device_fuzz(ctx, seed):
    check_case(ctx, ic.fuzz_case(seed))


@pytest.mark.parametrize("sites,grouped", sc.COHORTS)
def test_blocks_of_the_cohort(ctx, sites, grouped):
    """Diagonal, off-diagonal and partial tiles in one launch; a pair's record is the same bytes
    in every block that holds it, with clear and with all-ones padding."""
    c = sc.cohort(sites, grouped)
    whole = sc.by_pair(sc.cohort_records(sites, grouped, "diagonal"))
    for name, block in sc.BLOCKS.items():
        want = sc.cohort_records(sites, grouped, name)
        assert len(want) > 0 or (sites == 64 and grouped)
        for ones in (False, True):
            got = scan_device(ctx, c.bits(ones), *c.args(), block=block)
            assert got.tobytes() == want.tobytes(), (sites, name, ones)
        for key, row in sc.by_pair(want).items():
            assert whole[key] == row


def test_a_second_stream_a_second_call_and_one_workgroup_per_launch(ctx):
    import torch
    sites, grouped = sc.COHORTS[-1]
    c = sc.cohort(sites, grouped)
    side = torch.cuda.Stream()
    for name in ("diagonal", "off-diagonal"):
        want = sc.cohort_records(sites, grouped, name)
        for stream in (side, None, side):
            got = scan_device(ctx, c.bits(), *c.args(), block=sc.BLOCKS[name], stream=stream)
            assert got.tobytes() == want.tobytes()
        # six and four tiles, one launch each, all but the first with a tile base above 0
        ctx.set_option("max_launch_blocks", 1)
        try:
            got = scan_device(ctx, c.bits(), *c.args(), block=sc.BLOCKS[name])
        finally:
            ctx.set_option("max_launch_blocks", 0)
        assert got.tobytes() == want.tobytes()


def test_the_scan_equals_the_listed_call_on_its_own_pairs(ctx):
    sites, grouped = sc.COHORTS[-1]
    c = sc.cohort(sites, grouped)
    bits = _device(c.bits())
    found = ctx.ibd_scan(bits, c.wps, sites, group=c.group, pos=c.pos, min_sites=c.min_sites,
                         min_length=c.min_length)
    assert found.num_records == len(sc.cohort_records(sites, grouped, "diagonal")) > 20
    assert found.pairs().dtype == np.uint32 and found.pairs().shape == (found.num_records, 2)
    listed = ctx.ibd_segments(bits, c.wps, sites, found.pairs(), group=c.group, pos=c.pos,
                              min_sites=c.min_sites, min_length=c.min_length)
    assert found.rows.tobytes() == listed.rows.tobytes()
    assert found.total_length == listed.total_length
    assert np.array_equal(found.relationship(), listed.relationship())


def test_min_total(ctx):
    sites, grouped = sc.COHORTS[2]
    c = sc.cohort(sites, grouped)
    want = sc.cohort_records(sites, grouped, "diagonal")
    length = int(np.sort(want["length1"])[len(want) // 2])
    for min_total in (0, length, length + 1):
        got = scan_device(ctx, c.bits(), *c.args(), min_total=min_total)
        assert got.tobytes() == sc.filtered(want, min_total).tobytes()


def test_overflow_retry_the_counting_call_and_the_waits(ctx):
    import torch
    sites, grouped = sc.COHORTS[2]
    c = sc.cohort(sites, grouped)
    bits = _device(c.bits())
    kw = dict(group=c.group, min_sites=c.min_sites)   # (no pos: no check of positions to wait for)
    want_nopos = sc.listed_records(c.bits(), c.wps, sites, c.group, None, c.min_sites, 0,
                                   sc.BLOCKS["diagonal"])
    total = len(want_nopos)
    before = ctx.get_option("host_syncs")
    recs, count = ctx.ibd_scan_raw(bits, c.wps, sites, max_records=total, **kw)
    assert ctx.get_option("host_syncs") - before == 1   # (the count, and nothing else)
    assert count == total and tuple(recs.shape) == (total, 10)
    assert ibd.records_to_host(recs, count).tobytes() == want_nopos.tobytes()
    # with positions the check of the listed call waits once more
    before = ctx.get_option("host_syncs")
    ctx.ibd_scan_raw(bits, c.wps, sites, pos=c.pos, **kw)
    assert ctx.get_option("host_syncs") - before == 2
    # one less, and the counting call: the exact count, nothing past the buffer
    for room in (total - 1, 0):
        out = torch.full((total + 4, 10), sc.FILL, dtype=torch.int32, device="cuda:0")
        before = ctx.get_option("host_syncs")
        with pytest.raises(cuking_amd.ResourceExhaustedError, match=f"{total} records") as e:
            ctx.ibd_scan_raw(bits, c.wps, sites, max_records=room, out=out, **kw)
        assert e.value.num_records == total
        assert ctx.get_option("host_syncs") - before == 1
        out = out.cpu().numpy()
        assert (out[room:] == sc.FILL).all()
        stored = np.ascontiguousarray(out[:room]).view(ibd.IBD_PAIR_DTYPE).reshape(-1)
        have = sc.by_pair(want_nopos)
        assert len(sc.by_pair(stored)) == room
        assert all(have[key] == row for key, row in sc.by_pair(stored).items())
    # the raw counting call: null records
    found = C.c_uint64(77)
    block = cuking_amd.Submatrix.from_ranges(0, sc.COHORT_SAMPLES, 0, sc.COHORT_SAMPLES)
    st = ctx.lib.cuking_ibd_scan(ctx.handle, bits.data_ptr(), sc.COHORT_SAMPLES, c.wps, sites,
                                 None, None, c.min_sites, 0, C.byref(block.c), 0, None, 0,
                                 C.byref(found), None)
    one_group = sc.listed_records(c.bits(), c.wps, sites, None, None, c.min_sites, 0,
                                  sc.BLOCKS["diagonal"])
    assert st == _lib.ERR_RESOURCE_EXHAUSTED and found.value == len(one_group) > 0
    # the wrapper's one retry: 2415 pairs of duplicates against a default buffer of 2240
    d = sc.duplicates()
    before = ctx.get_option("host_syncs")
    got = ctx.ibd_scan(_device(d.bits()), d.wps, d.sites, min_sites=d.min_sites)
    assert ctx.get_option("host_syncs") - before == 2   # (two calls, each reads its count)
    assert got.num_records == 2415 and got.rows.tobytes() == sc.listed_records(
        d.bits(), *d.args(), (0, 70, 0, 70)).tobytes()
    assert (got.relationship() == pcr.DUPLICATE).all()


def _raw_device(ctx, inp, **over):
    """cuking_ibd_scan with single arguments replaced; returns (status, records, found)."""
    import torch
    records = torch.full((16, 10), sc.FILL, dtype=torch.int32, device="cuda:0")
    bits = _device(inp.bits())
    found = C.c_uint64(77)
    n = inp.case.samples
    block = over.pop("block", (0, n, 0, n))
    sm = None if block is None else cuking_amd.Submatrix.from_ranges(*block)
    pos = over.pop("pos", None)
    d_pos = None
    if pos is not None:
        d_pos = torch.from_numpy(sc.decreasing_pos(inp.case.sites).view(np.int32)).to("cuda:0")
    pointers = dict(bits=bits.data_ptr(), group=None,
                    pos=None if d_pos is None else d_pos.data_ptr(),
                    block=None if sm is None else C.byref(sm.c), records=records.data_ptr(),
                    found=C.byref(found))
    st = ctx.lib.cuking_ibd_scan(ctx.handle, *sc.raw_arguments(inp, pointers, **over), None)
    torch.cuda.synchronize()
    return st, records.cpu().numpy(), found.value


@pytest.mark.parametrize("name", sc.REFUSALS)
def test_device_refusals_leave_the_buffer_untouched(ctx, name):
    inp = ic.inputs(sc.REFUSAL_CASE)
    over, status, text = sc.REFUSALS[name]
    st, records, found = _raw_device(ctx, inp, **dict(over))
    assert st == (_lib.ERR_INVALID_ARGUMENT if status == "INVALID"
                  else _lib.ERR_FAILED_PRECONDITION), name
    assert text in ctx.lib.cuking_last_error().decode()
    # (the count starts at zero on every call that has somewhere to write it)
    assert (records == sc.FILL).all() and found == (77 if "found" in over else 0)


@pytest.mark.parametrize("name", sc.NO_WORK)
def test_device_calls_without_work(ctx, name):
    inp = ic.inputs(sc.REFUSAL_CASE)
    st, records, found = _raw_device(ctx, inp, **dict(sc.NO_WORK[name]))
    assert st == _lib.OK and found == 0 and (records == sc.FILL).all()
    # ... and the call with work, through the same helper
    st, records, found = _raw_device(ctx, inp)
    want = sc.listed_case(sc.REFUSAL_CASE)
    assert st == _lib.OK and 1 <= found == len(want) <= 16
    got = np.ascontiguousarray(records[:found]).view(ibd.IBD_PAIR_DTYPE).reshape(-1)
    assert got.tobytes() == want.tobytes() and (records[found:] == sc.FILL).all()


def test_the_synthetic_cohort_end_to_end(ctx):
    """Scan at min_sites = 512, then relationship(): every planted relationship the listed call
    recovers from the KING records is recovered from the scan's records, with the same bytes."""
    import torch
    from cuking_amd.synth import cohort_to_device
    n, m, seed = E2E
    cohort, index, labels = e2e_cohort()
    kind, pa, pb = cohort_to_device(cohort)
    bits = ctx.synth_bitset(seed, kind, pa, pb, 0, n, m)
    wps = bits.shape[1]
    found = ctx.ibd_scan(bits, wps, m)
    host = cuking_amd.ibd_scan_host(bits.cpu().numpy().view(np.uint64), wps, m)
    assert found.rows.tobytes() == host.rows.tobytes() and found.total_length == m - 1
    # the listed call on the record buffer of compute_king
    sm = cuking_amd.Submatrix(n)
    results = torch.zeros((4096, 6), dtype=torch.int32, device="cuda:0")
    index_flag = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    ctx.compute_king(sm, wps, bits, 0.177, 4096, results, index_flag[0:1], index_flag[1:2])
    count = int(index_flag[0])
    listed = ctx.ibd_segments(bits, wps, m, results, num_records=count)
    scan_rows, scan_codes = sc.by_pair(found.rows), found.relationship()
    at = {key: k for k, key in enumerate(scan_rows)}
    codes = listed.relationship()
    recovered = 0
    for k, r in enumerate(listed.rows):
        key = (int(r["sample_i"]), int(r["sample_j"]))
        if codes[k] != pcr.UNRELATED:
            assert scan_rows[key] == r.tobytes()[8:] and scan_codes[at[key]] == codes[k]
            recovered += 1
    planted = {(min(a, b), max(a, b)) for (a, b), what in zip(index, labels) if what != "none"}
    assert recovered >= len(planted) and planted <= set(scan_rows)
