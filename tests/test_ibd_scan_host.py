"""IBD scan of a block, host side (no GPU): the host twin against the listed call over the
explicit list of all pairs and against the per-site numpy walk of ibd_cases.py, the blocks of the
70-sample cohort, min_total, the buffer rule, the refusals, the superset guarantee for the bridged
call, the stand-alone sanitizer driver and the end-to-end check on the synthetic cohort."""
import ctypes as C

import numpy as np
import pytest

import ibd_cases as ic
import ibd_scan_cases as sc
from host_driver import run_sanitized_driver
from test_ibd_bridge_host import e2e_codes
from test_ibd_host import E2E, e2e_cohort

import cuking_amd
from cuking_amd import _lib, ibd
from cuking_amd import pcrelate as pcr


def check_case(case):
    records, count = sc.scan_case(case)
    want = sc.listed_case(case)
    assert count == len(records) == len(want)
    assert records.dtype == ibd.IBD_PAIR_DTYPE and records.tobytes() == want.tobytes(), case.name
    sc.check_sorted(records)
    # all-ones padding beyond num_sites: the same bytes
    assert sc.scan_case(case, ones_padding=True)[0].tobytes() == want.tobytes(), case.name
    return records


@pytest.mark.parametrize("case", ic.CASES, ids=lambda c: c.name)
def test_host_twin_equals_the_listed_call_and_the_naive_walk(case):
    sc.check_reference(case, check_case(case))


@pytest.mark.parametrize("seed", ic.FUZZ_SEEDS)
def test_host_twin_fuzz(seed):
    case = ic.fuzz_case(seed)
    sc.check_reference(case, check_case(case))


def test_the_cases_have_records_and_the_walk_sees_them():
    seen = sum(sc.check_reference(case, sc.scan_case(case)[0]) for case in ic.CASES)
    assert seen > 40


@pytest.mark.parametrize("sites,grouped", sc.COHORTS)
def test_blocks_of_the_cohort(sites, grouped):
    """The diagonal block, a sub-block and two off-diagonal blocks: the listed call's records,
    and a pair's record is the same bytes in every block that holds it."""
    c = sc.cohort(sites, grouped)
    whole = sc.by_pair(sc.cohort_records(sites, grouped, "diagonal"))
    if sites == 64 and grouped:   # two groups leave no room for 64 sites
        assert not whole
    else:
        assert len(whole) >= len(sc.PLANTED)
    for name, block in sc.BLOCKS.items():
        want = sc.cohort_records(sites, grouped, name)
        records, count = ibd.ibd_scan_raw_host(c.bits(), *c.args(), block=block)
        assert count == len(want) and records.tobytes() == want.tobytes(), (sites, name)
        sc.check_sorted(records)
        i0, i1, j0, j1 = block
        inside = {key: row for key, row in whole.items()
                  if i0 <= key[0] < i1 and j0 <= key[1] < j1}
        assert sc.by_pair(records) == inside, (sites, name)
        if whole:
            assert len(inside) >= 2   # (every block holds planted pairs)
        padded, _ = ibd.ibd_scan_raw_host(c.bits(True), *c.args(), block=block)
        assert padded.tobytes() == want.tobytes()


def test_min_total():
    sites, grouped = sc.COHORTS[2]
    c = sc.cohort(sites, grouped)
    want = sc.cohort_records(sites, grouped, "diagonal")
    length = int(np.sort(want["length1"])[len(want) // 2])
    counts = []
    for min_total in (0, length, length + 1, 1 << 63):
        records, count = ibd.ibd_scan_raw_host(c.bits(), *c.args(), min_total=min_total)
        assert records.tobytes() == sc.filtered(want, min_total).tobytes()
        counts.append(count)
    assert counts[0] == len(want) and counts[1] > counts[2] and counts[3] == 0
    at = [int(x) for x in want["length1"]].index(length)
    key = (int(want[at]["sample_i"]), int(want[at]["sample_j"]))
    assert key in sc.by_pair(ibd.ibd_scan_raw_host(c.bits(), *c.args(), min_total=length)[0])
    assert key not in sc.by_pair(ibd.ibd_scan_raw_host(c.bits(), *c.args(),
                                                       min_total=length + 1)[0])
    with pytest.raises(ValueError):
        ibd.ibd_scan_raw_host(c.bits(), *c.args(), min_total=-1)


def test_the_buffer_rule():
    sites, grouped = sc.COHORTS[2]
    c = sc.cohort(sites, grouped)
    want = sc.cohort_records(sites, grouped, "diagonal")
    total = len(want)
    records, count = ibd.ibd_scan_raw_host(c.bits(), *c.args(), max_records=total)
    assert count == total and records.tobytes() == want.tobytes()
    for room in (total - 1, 0):
        with pytest.raises(cuking_amd.ResourceExhaustedError, match=f"{total} records") as e:
            ibd.ibd_scan_raw_host(c.bits(), *c.args(), max_records=room)
        assert e.value.num_records == total
    # the raw call: the first max_records in ascending (i, j), nothing past the buffer
    bits = c.bits()
    block = cuking_amd.Submatrix.from_ranges(0, 70, 0, 70)

    def raw(records, room, found):
        return _lib.load().cuking_ibd_scan_host(
            bits.ctypes.data, 70, c.wps, sites, c.group.ctypes.data, c.pos.ctypes.data,
            c.min_sites, c.min_length, C.byref(block.c), 0,
            None if records is None else records.ctypes.data, room,
            None if found is None else C.byref(found))

    out = np.full(10 * (total + 2), sc.FILL, dtype=np.uint32)
    found = C.c_uint64(77)
    assert raw(out, 3, found) == _lib.ERR_RESOURCE_EXHAUSTED and found.value == total
    assert out[:30].tobytes() == want[:3].tobytes() and (out[30:] == sc.FILL).all()
    found = C.c_uint64(77)   # the counting call
    assert raw(None, 0, found) == _lib.ERR_RESOURCE_EXHAUSTED and found.value == total
    found = C.c_uint64(77)
    assert raw(out, total, found) == _lib.OK and found.value == total
    assert out[:10 * total].tobytes() == want.tobytes() and (out[10 * total:] == sc.FILL).all()
    # the wrapper's one retry: 2415 pairs of duplicates against a default buffer of 2240
    d = sc.duplicates()
    assert pcr._default_records(cuking_amd.Submatrix.from_ranges(0, 70, 0, 70)) == 2240
    got = cuking_amd.ibd_scan_host(d.bits(), *d.args())
    assert got.num_records == 2415 and got.min_total == 0
    assert got.pairs().tobytes() == sc.block_pairs((0, 70, 0, 70)).tobytes()
    assert (got.segments2 == 1).all() and (got.relationship() == pcr.DUPLICATE).all()
    assert got.total_length == 199 and got.segments is None


def _raw_host(inp, **over):
    """cuking_ibd_scan_host with single arguments replaced; returns (status, records, found)."""
    records = np.full(16 * 10, sc.FILL, dtype=np.uint32)
    found = C.c_uint64(77)
    bits = inp.bits()
    n = inp.case.samples
    block = over.pop("block", (0, n, 0, n))
    sm = None if block is None else cuking_amd.Submatrix.from_ranges(*block)
    pos = sc.decreasing_pos(inp.case.sites) if over.pop("pos", None) else None
    pointers = dict(bits=bits.ctypes.data, group=None,
                    pos=None if pos is None else pos.ctypes.data,
                    block=None if sm is None else C.byref(sm.c), records=records.ctypes.data,
                    found=C.byref(found))
    st = _lib.load().cuking_ibd_scan_host(*sc.raw_arguments(inp, pointers, **over))
    return st, records, found.value


@pytest.mark.parametrize("name", sc.REFUSALS)
def test_host_refusals(name):
    inp = ic.inputs(sc.REFUSAL_CASE)
    over, status, text = sc.REFUSALS[name]
    st, records, found = _raw_host(inp, **dict(over))
    assert st == (_lib.ERR_INVALID_ARGUMENT if status == "INVALID"
                  else _lib.ERR_FAILED_PRECONDITION), name
    assert text in _lib.load().cuking_last_error().decode()
    # (the count starts at zero on every call that has somewhere to write it)
    assert (records == sc.FILL).all() and found == (77 if "found" in over else 0)


@pytest.mark.parametrize("name", sc.NO_WORK)
def test_calls_without_work(name):
    inp = ic.inputs(sc.REFUSAL_CASE)
    st, records, found = _raw_host(inp, **dict(sc.NO_WORK[name]))
    assert st == _lib.OK and found == 0 and (records == sc.FILL).all()
    # ... and the call with work, through the same helper
    st, records, found = _raw_host(inp)
    want = sc.listed_case(sc.REFUSAL_CASE)
    assert st == _lib.OK and 1 <= found == len(want) <= 16
    assert records[:10 * found].tobytes() == want.tobytes()
    assert (records[10 * found:] == sc.FILL).all()


def test_the_wrapper_takes_a_block_and_gives_an_ibdpairs():
    sites, grouped = sc.COHORTS[3]
    c = sc.cohort(sites, grouped)
    got = cuking_amd.ibd_scan_host(c.bits(), c.wps, sites, group=c.group, pos=c.pos,
                                   min_sites=c.min_sites, min_length=c.min_length,
                                   block=sc.BLOCKS["off-diagonal"])
    want = sc.cohort_records(sites, grouped, "off-diagonal")
    assert isinstance(got, ibd.IBDPairs) and got.rows.tobytes() == want.tobytes()
    assert got.num_records == len(want) and got.block.i_end == 33 and got.block.j_begin == 33
    assert got.total_length == ibd.genome_length(c.group, c.pos, sites)
    listed = cuking_amd.ibd_segments_host(c.bits(), c.wps, sites, got.pairs(), group=c.group,
                                          pos=c.pos, min_sites=c.min_sites,
                                          min_length=c.min_length)
    assert listed.rows.tobytes() == got.rows.tobytes()
    assert np.array_equal(listed.relationship(), got.relationship())
    empty = cuking_amd.ibd_scan_host(c.bits(), c.wps, sites, block=(4, 4, 4, 4))
    assert empty.num_records == 0 and empty.pairs().shape == (0, 2)


@pytest.mark.parametrize("bridge", [64, 128])
def test_the_scan_is_a_superset_of_the_bridged_call(oracle, bridge):
    """On the synthetic cohort with one genotype in 400 replaced: every pair for which the bridged
    call at min_sites = 512 reports a kind-1 segment is a record of the scan at min_sites = B."""
    n, m, _ = E2E
    _, noisy, wps = e2e_codes(oracle)
    bits = ic.pack_codes(noisy, wps // 2, ones_padding=True)
    every = sc.block_pairs((0, n, 0, n))
    bridged = cuking_amd.ibd_segments_host(bits, wps, m, every, min_sites=512, bridge_sites=bridge)
    need = {(int(i), int(j)) for i, j in every[bridged.segments1 > 0]}
    found = cuking_amd.ibd_scan_host(bits, wps, m, min_sites=bridge)
    have = {(int(i), int(j)) for i, j in found.pairs()}
    assert need and need <= have


def test_host_side_under_asan_ubsan(tmp_path):
    """csrc/king_host.cc and a stand-alone driver (tests/ibd_scan_host_driver.cc) built with
    AddressSanitizer + UBSan.  A program of its own on the CPU: nothing is loaded into Python."""
    run_sanitized_driver(tmp_path, "ibd_scan_host_driver")


def test_end_to_end_on_the_host(oracle):
    """The synthetic cohort with its planted relatives: scan at min_sites = 512, then
    relationship().  The scan's records are the filtered listed call over all pairs; every
    planted relationship the listed call recovers is recovered from the scan, with the same row
    bytes.  (The README's count of unrelated pairs the scan also records is `others` below.)"""
    n, m, seed = E2E
    cohort, index, labels = e2e_cohort()
    bits = oracle.synth_bitset(seed, cohort.kind, cohort.pa, cohort.pb, 0, n, m)
    wps = bits.shape[1]
    found = cuking_amd.ibd_scan_host(bits, wps, m)
    every = sc.block_pairs((0, n, 0, n))
    want = sc.filtered(cuking_amd.ibd_segments_host(bits, wps, m, every).rows)
    assert found.rows.tobytes() == want.tobytes() and found.total_length == m - 1
    listed = cuking_amd.ibd_segments_host(bits, wps, m, index)
    rows, codes = sc.by_pair(found.rows), found.relationship()
    at = {key: k for k, key in enumerate(rows)}
    related = labels != "none"
    assert related.sum() >= 7
    for r, code in zip(listed.rows[related], listed.relationship()[related]):
        key = (int(min(r["sample_i"], r["sample_j"])), int(max(r["sample_i"], r["sample_j"])))
        assert code in (pcr.PARENT_CHILD, pcr.DUPLICATE)
        assert rows[key] == r.tobytes()[8:] and codes[at[key]] == code
    others = int((codes == pcr.UNRELATED).sum())
    print(f"scan of {n} samples x {m} sites at min_sites = 512: {found.num_records} records, "
          f"{others} of them unrelated by relationship()")
