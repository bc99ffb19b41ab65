"""Runs of homozygosity without a GPU: the host twin against the naive walk of roh_cases.py (rows
and sorted segments, bytewise), the independent cross-check through the IBD code, the refusals
with their messages, the overflow rule, froh(), the stand-alone sanitizer driver and the
end-to-end cohort with genotyping errors."""
import ctypes as C

import numpy as np
import pytest

import roh_cases as rc
from host_driver import run_sanitized_driver

import cuking_amd
from cuking_amd import _lib, ibd, roh


def bridges_of(case):
    return (case.bridge,) if case.bridge == 0 else (case.bridge, 0)


@pytest.mark.parametrize("case", rc.CASES, ids=lambda c: c.name)
def test_host_twin_equals_the_naive_walk(case):
    rc.check_case(case)
    for bridge in bridges_of(case):
        rows, segments = rc.run_host(case, bridge=bridge)
        rc.check_against(case, rows, segments, "host twin", bridge)
        # all-ones padding beyond num_sites: the same bytes
        padded = rc.run_host(case, ones_padding=True, bridge=bridge)
        assert padded[0].tobytes() == rows.tobytes()
        assert rc.sort_rows(padded[1]).tobytes() == rc.sort_rows(segments).tobytes()


@pytest.mark.parametrize("seed", rc.FUZZ_SEEDS)
def test_host_twin_fuzz(seed):
    case = rc.fuzz_case(seed)
    rc.check_fuzz_case(case)
    rc.check_against(case, *rc.run_host(case), "host twin")
    padded = rc.run_host(case, ones_padding=True)
    rc.check_against(case, *padded, "host twin, ones padding")


def test_the_case_list_covers_the_scan():
    """The minimum counts below were fixed after running the naive reference on the CPU: the
    cases hold 108 segments at their own bridge_sites and 29 bridged hets (rows of repeated
    samples included), the 40 fuzz seeds 87 segments and 49 bridged hets over 25 values of
    bridge_sites, and 13 seeds give another segment list strictly."""
    assert rc.S == 64 * 64 and _lib.IBD_MIN_SITES == 64
    assert rc.SITE_COUNTS <= {c.sites for c in rc.CASES}
    assert max(c.samples for c in rc.CASES) <= 20 and any(c.samples > 8 for c in rc.CASES)
    assert {c.tight for c in rc.CASES} == {0, 1} and {c.listed for c in rc.CASES} == {0, 1}
    assert {c.bridge for c in rc.CASES} >= {0, 64, 80, 100}
    assert any(c.bounds for c in rc.CASES) and any(c.pos and c.min_length for c in rc.CASES)
    assert any(c.all_missing for c in rc.CASES) and any(c.all_het for c in rc.CASES)
    assert sum(len(rc.reference(c)[1]) for c in rc.CASES) >= 50
    assert sum(int(rc.reference(c)[0]["bridged"].sum()) for c in rc.CASES) >= 10
    fuzz = [rc.fuzz_case(s) for s in rc.FUZZ_SEEDS]
    assert max(c.samples for c in fuzz) <= 20 and len({c.bridge for c in fuzz}) > 15
    assert sum(len(rc.reference(c)[1]) for c in fuzz) >= 60
    assert sum(int(rc.reference(c)[0]["bridged"].sum()) for c in fuzz) >= 30
    assert sum(rc.reference(c)[1].tobytes() != rc.reference(c, 0)[1].tobytes()
               for c in fuzz) >= 10


def test_one_case_in_full():
    """700 sites, a plant 100 .. 300 of sample 0 with a het at 200, min_sites 150."""
    case = next(c for c in rc.CASES if c.name.startswith("100 + het + 100"))
    inp = rc.inputs(case)
    bits = inp.bits()
    got = cuking_amd.roh_segments_host(bits, inp.wps, case.sites, [0], min_sites=150,
                                       bridge_sites=64, segments=True)
    assert isinstance(got, cuking_amd.ROHSamples) and got.rows.dtype == cuking_amd.ROH_SAMPLE_DTYPE
    assert [tuple(int(x) for x in s) for s in got.sorted()] == [(0, roh.ROH_KIND, 100, 300)]
    assert (got.sample[0], got.segments[0], got.length[0], got.longest[0], got.bridged[0]) == \
        (0, 1, 200, 200, 1)
    assert got.total_length == 699 and got.froh()[0] == 200 / 699
    assert (got.min_sites, got.min_length, got.bridge_sites) == (150, 0, 64)
    strict = cuking_amd.roh_segments_host(bits, inp.wps, case.sites, [0], min_sites=150)
    assert strict.segments[0] == 0 and strict.segment_list is None and strict.froh()[0] == 0
    with pytest.raises(ValueError, match="segments=True"):
        strict.sorted()
    # at min_sites = 64 the strict call sees the two runs
    loose = cuking_amd.roh_segments_host(bits, inp.wps, case.sites, [0], min_sites=64,
                                         segments=True)
    assert [tuple(int(x) for x in s)[2:] for s in loose.sorted()] == [(100, 199), (201, 300)]


@pytest.mark.parametrize("case", rc.CASES, ids=lambda c: c.name)
def test_an_explicit_list_equals_the_null_list(case):
    everyone = np.arange(case.samples, dtype=np.uint32)
    inp = rc.inputs(case)
    null_rows, null_segs = rc.run_host(case, listed=False)
    rows, segs = roh.roh_segments_raw_host(inp.bits(), inp.wps, case.sites, everyone, inp.group,
                                           inp.pos, case.min_sites, case.min_length, case.bridge,
                                           segments=True)
    assert rows.tobytes() == null_rows.tobytes() and null_rows["sample"].tolist() == \
        everyone.tolist()
    assert rc.sort_rows(segs).tobytes() == rc.sort_rows(null_segs).tobytes()
    # a row depends on its own sample only: the case's shuffled list with repeats
    if inp.listed is not None:
        shuffled, _ = rc.run_host(case)
        inside = inp.listed < case.samples
        assert shuffled[inside].tobytes() == null_rows[inp.listed[inside]].tobytes()


# ---- the independent cross-check through the existing IBD code ----------------------------------
def ibd_twin_inputs(case):
    """The case's bitset with one more row t per sample s -- hom-ref where s is het, missing
    everywhere else -- and the pairs (s, t): ibd_diff(s, t) is exactly the het sites of s."""
    inp = rc.inputs(case)
    shadow = np.where(inp.code == 1, 0, 3).astype(np.uint8)
    bits = rc.pack_codes(np.vstack([inp.code, shadow]), inp.wps // 2)
    n = case.samples
    pairs = np.stack([np.arange(n), n + np.arange(n)], axis=1).astype(np.uint32)
    return inp, bits, pairs


def check_ibd_twin(case, roh_rows, ibd_rows, ibd_bridged):
    assert roh_rows["segments"].tobytes() == ibd_rows["segments2"].tobytes(), case.name
    assert roh_rows["length"].tobytes() == ibd_rows["length2"].tobytes(), case.name
    assert roh_rows["longest"].tobytes() == ibd_rows["longest2"].tobytes(), case.name
    assert roh_rows["bridged"].tobytes() == \
        np.ascontiguousarray(ibd_bridged[:, 1]).tobytes(), case.name


@pytest.mark.parametrize("case", rc.CASES + [rc.fuzz_case(s) for s in range(8)],
                         ids=lambda c: c.name)
def test_kind_2_of_the_ibd_scan_of_a_shadow_row_is_the_roh_row(case):
    inp, bits, pairs = ibd_twin_inputs(case)
    args = (inp.group, inp.pos, case.min_sites, case.min_length)
    for bridge in (0, 64):
        mine, _ = roh.roh_segments_raw_host(inp.bits(), inp.wps, case.sites, None, *args, bridge)
        if bridge == 0:
            theirs, _ = ibd.ibd_segments_raw_host(bits, inp.wps, case.sites, pairs, *args)
            bridged = np.zeros((case.samples, 2), dtype=np.uint32)
        else:
            theirs, _, bridged = ibd.ibd_segments_raw_host(bits, inp.wps, case.sites, pairs,
                                                           *args, bridge_sites=bridge)
        check_ibd_twin(case, mine, theirs, bridged)


# ---- refusals ------------------------------------------------------------------------------------
def raw_host(inp, **over):
    """cuking_roh_samples_host with single arguments replaced: (status, out, segments, found)."""
    count = inp.case.samples if inp.listed is None else len(inp.listed)
    out = np.full(count * 6, 0xABABABAB, dtype=np.uint32)
    segments = np.zeros(16, dtype=ibd.IBD_SEGMENT_DTYPE)
    found = C.c_uint64(77)
    bits = inp.bits()
    keep = []
    if over.get("pos") == "decreasing":
        pos = np.arange(inp.case.sites, dtype=np.uint32)
        pos[100] = 5
        keep.append(pos)
        over = dict(over, pos=pos.ctypes.data)
    pointers = dict(bits=bits.ctypes.data, group=None, pos=None,
                    samples=None if inp.listed is None else inp.listed.ctypes.data,
                    out=out.ctypes.data, segments=segments.ctypes.data, found=C.byref(found))
    st = _lib.load().cuking_roh_samples_host(*rc.raw_arguments(inp, pointers, **over))
    return st, out, segments, found.value


@pytest.mark.parametrize("name", rc.REFUSALS)
def test_every_refusal_with_its_message(name):
    over, status, word = rc.REFUSALS[name]
    inp = rc.inputs(rc.REFUSAL_CASE)
    st, out, _, _ = raw_host(inp, **over)
    want = _lib.ERR_INVALID_ARGUMENT if status == "INVALID" else _lib.ERR_FAILED_PRECONDITION
    assert st == want, name
    assert (out == 0xABABABAB).all()
    message = _lib.load().cuking_last_error().decode()
    assert word in message, message


def test_the_refusals_are_those_of_the_bridged_ibd_call():
    """Message for message: the same refusal of cuking_ibd_pairs_bridged_host."""
    inp = rc.inputs(rc.REFUSAL_CASE)
    bits = inp.bits()
    pairs = np.array([[0, 1]], dtype=np.uint32)
    out, bridged = np.zeros(10, dtype=np.uint32), np.zeros(2, dtype=np.uint32)
    for over in (dict(wps=3), dict(min_sites=63), dict(bridge=63), dict(num_sites=193)):
        st, _, _, _ = raw_host(inp, **over)
        mine = _lib.load().cuking_last_error().decode()
        a = dict(wps=inp.wps, num_sites=180, min_sites=64, bridge=0)
        a.update(over)
        st2 = _lib.load().cuking_ibd_pairs_bridged_host(
            bits.ctypes.data, 6, a["wps"], a["num_sites"], None, None, a["min_sites"], 0,
            a["bridge"], pairs.ctypes.data, 1, 8, out.ctypes.data, bridged.ctypes.data, None, 0,
            None)
        assert st == st2 == _lib.ERR_INVALID_ARGUMENT
        assert mine == _lib.load().cuking_last_error().decode()


def test_the_wrappers_refuse_too():
    inp = rc.inputs(rc.REFUSAL_CASE)
    args = (inp.bits(), inp.wps, rc.REFUSAL_CASE.sites)
    with pytest.raises(cuking_amd.CukingError, match="bridge_sites"):
        roh.roh_segments_raw_host(*args, bridge_sites=63)
    with pytest.raises(cuking_amd.CukingError, match="min_sites"):
        roh.roh_segments_raw_host(*args, min_sites=10)
    with pytest.raises(ValueError, match="samples"):
        roh.roh_segments_raw_host(*args, samples=np.zeros((2, 2), dtype=np.uint32))
    with pytest.raises(ValueError, match="uint32"):
        roh.roh_segments_raw_host(*args, samples=[-1])
    with pytest.raises(ValueError, match="pos"):
        roh.roh_segments_raw_host(*args, pos=np.zeros(3, dtype=np.uint32))


def test_the_calls_without_work():
    inp = rc.inputs(rc.REFUSAL_CASE)
    st, out, _, found = raw_host(inp, num_samples=0, samples=None, out=None, bits=None)
    assert st == _lib.OK and (out == 0xABABABAB).all() and found == 0
    rows, segs = roh.roh_segments_raw_host(inp.bits(), inp.wps, 180, samples=[], segments=True)
    assert len(rows) == 0 and len(segs) == 0
    # num_sites == 0 writes zero rows
    rows, _ = roh.roh_segments_raw_host(inp.bits(), inp.wps, 0, samples=[3, 1])
    assert rows["sample"].tolist() == [3, 1] and not rows["segments"].any()
    assert np.isnan(roh.roh_segments_host(inp.bits(), inp.wps, 0).froh()).all()


# ---- the overflow rule ---------------------------------------------------------------------------
def test_the_overflow_rule():
    """Exact count, one retry, max_segments = 0 counts."""
    case = next(c for c in rc.CASES if c.name == "every word a group")
    inp = rc.inputs(case)
    want_rows, want_segments = rc.reference(case)
    total = len(want_segments)
    assert total > 16    # (more than the raw call's buffer below)
    # the default buffer of a list of ONE sample is four segments: one retry with the count
    rows, segs = roh.roh_segments_raw_host(inp.bits(), inp.wps, case.sites, [0], inp.group,
                                           min_sites=case.min_sites, segments=True)
    assert rows["segments"][0] == len(segs) == 10 > 4
    for room in (total - 1, 1, 0):
        with pytest.raises(cuking_amd.ResourceExhaustedError) as e:
            rc.run_host(case, max_segments=room)
        assert e.value.num_segments == total
    rows, segs = rc.run_host(case, max_segments=total)
    rc.check_against(case, rows, segs, "exactly the count")
    # the raw call: every row written, nothing past the buffer, the exact count
    st, out, segments, found = raw_host(inp, group=inp.group.ctypes.data)
    assert st == _lib.ERR_RESOURCE_EXHAUSTED and found == total
    assert out.view(roh.ROH_SAMPLE_DTYPE).tobytes() == want_rows.tobytes()
    assert all(tuple(s) in set(map(tuple, want_segments.tolist())) for s in segments.tolist())
    st, out, _, found = raw_host(inp, group=inp.group.ctypes.data, segments=None, max_segments=0)
    assert st == _lib.ERR_RESOURCE_EXHAUSTED and found == total
    assert out.view(roh.ROH_SAMPLE_DTYPE).tobytes() == want_rows.tobytes()


def test_froh_on_hand_made_values():
    rows = np.zeros(4, dtype=roh.ROH_SAMPLE_DTYPE)
    rows["length"] = [0, 250, 1000, 2 ** 40]
    got = roh.ROHSamples(rows, 1000, None, 512, 0)
    assert got.froh().dtype == np.float64
    assert got.froh().tolist() == [0.0, 0.25, 1.0, 2 ** 40 / 1000]
    empty = roh.ROHSamples(rows, 0, None, 512, 0)
    assert np.isnan(empty.froh()).all() and empty.froh().shape == (4,)
    assert ibd.genome_length([0, 0, 1, 1, 1], [5, 9, 2, 3, 10], 5) == 4 + 8


def test_host_side_under_asan_ubsan(tmp_path):
    """csrc/king_host.cc and a stand-alone driver (tests/roh_host_driver.cc) built with
    AddressSanitizer + UBSan.  A program of its own on the CPU: nothing is loaded into Python."""
    run_sanitized_driver(tmp_path, "roh_host_driver")


# ---- end to end ----------------------------------------------------------------------------------
def test_end_to_end_on_the_host():
    """24 samples x 6000 sites in 3 groups, six planted stretches, one planted genotype in 400
    flipped to het, min_sites = 256.  Found on the CPU at E2E_SEED: the strict call finds 1 of
    the 6 stretches, bridge_sites = 64 all 6, and no unplanted sample has a segment."""
    code, group, stretches = rc.e2e_cohort()
    m = rc.E2E_SITES
    bits = rc.pack_codes(code, -(-m // 64), ones_padding=True)
    kw = dict(group=group, min_sites=rc.E2E_MIN_SITES, segments=True)
    strict = cuking_amd.roh_segments_host(bits, bits.shape[1], m, **kw)
    bridged = cuking_amd.roh_segments_host(bits, bits.shape[1], m, bridge_sites=rc.E2E_BRIDGE,
                                           **kw)
    print("found strictly:", rc.e2e_found(strict, stretches), "bridged:",
          rc.e2e_found(bridged, stretches), "of", len(stretches))
    rc.check_e2e(strict, bridged, stretches)
    assert strict.total_length == bridged.total_length == 3 * 1999
    # ... and the host twin gives the naive walk's bytes here too
    for got, bridge in ((strict, 0), (bridged, rc.E2E_BRIDGE)):
        rows, segments = rc.naive(code, m, None, group, None, rc.E2E_MIN_SITES, 0, bridge)
        assert got.rows.tobytes() == rows.tobytes()
        assert got.sorted().tobytes() == segments.tobytes()
