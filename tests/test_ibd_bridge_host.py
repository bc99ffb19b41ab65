"""IBD segments with bridged breaks without a GPU: the host twin against the naive walk of
ibd_bridge_cases.py (rows, bridged counts and sorted segments, bytewise), bridge_sites = 0 against
the strict call, the refusals, the stand-alone sanitizer driver, and the end-to-end check on the
synthetic cohort with genotyping errors."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import ibd_bridge_cases as bc
import ibd_cases as ic
from host_driver import run_sanitized_driver
from test_ibd_host import E2E, e2e_cohort

import cuking_amd
from cuking_amd import _lib, ibd
from cuking_amd import pcrelate as pcr


@pytest.mark.parametrize("case", bc.CASES, ids=lambda c: c.name)
def test_host_twin_equals_the_naive_walk(case):
    bc.check_case(case)
    rows, segments, bridged = bc.run_host(case)
    bc.check_against(case, rows, segments, bridged, "host twin")
    # all-ones padding beyond num_sites: the same bytes
    padded = bc.run_host(case, ones_padding=True)
    assert padded[0].tobytes() == rows.tobytes() and padded[2].tobytes() == bridged.tobytes()
    assert ibd.sort_segments(padded[1]).tobytes() == ibd.sort_segments(segments).tobytes()


@pytest.mark.parametrize("seed", bc.FUZZ_SEEDS)
def test_host_twin_fuzz(seed):
    case = bc.fuzz_case(seed)
    bc.check_fuzz_case(case)
    bc.check_against(case, *bc.run_host(case), "host twin")


def test_the_case_list_covers_the_scan():
    assert bc.S == 64 * 64 and _lib.IBD_MIN_SITES == 64
    assert {640, bc.S, bc.S + 1, bc.TWO_STEPS} <= {c.sites for c in bc.CASES}
    assert {c.bridge for c in bc.CASES} >= {64, 80, 100}
    assert {c.stride for c in bc.CASES} == {8, 24} and {c.tight for c in bc.CASES} == {0, 1}
    assert any(c.bounds for c in bc.CASES) and any(c.pos and c.min_length for c in bc.CASES)
    assert sum(c.bridges for c in bc.CASES) >= 12 and sum(not c.bridges for c in bc.CASES) >= 6
    fuzz = [bc.fuzz_case(s) for s in bc.FUZZ_SEEDS]
    assert {c.bridge for c in fuzz} <= set(range(64, 151)) and len({c.bridge for c in fuzz}) > 20
    # the fuzz bridges something, and some of its breaks stay
    assert sum(int(bc.reference(c)[1].sum()) for c in fuzz) > 100
    assert sum(len(bc.reference(c)[2]) != len(bc.reference(c, 0)[2]) for c in fuzz) > 10


def test_the_first_case_in_full():
    """700 sites, a kind-2 plant 100 .. 600, one opp at 300, min_sites 150."""
    case = bc.CASES[0]
    _, _, plain = bc.reference(case, 0)
    rows, segments, bridged = bc.run_host(case)
    mine = lambda segs: [tuple(int(x) for x in s) for s in segs if s["pair"] == 0]  # noqa: E731
    assert mine(plain) == [(0, 1, 100, 299), (0, 1, 301, 600), (0, 2, 100, 299), (0, 2, 301, 600)]
    assert mine(ibd.sort_segments(segments)) == [(0, 1, 100, 600), (0, 2, 100, 600)]
    assert bridged[0].tolist() == [1, 1] and int(rows[0]["length1"]) == 500
    # the wrapper: IBDPairs carries bridge_sites and bridged; 0 leaves them out
    inp = bc.inputs(case)
    got = cuking_amd.ibd_segments_host(inp.bits(), inp.wps, case.sites, inp.pairs, min_sites=150,
                                       bridge_sites=64)
    assert got.bridge_sites == 64 and got.bridged.tobytes() == bridged.tobytes()
    assert got.rows.tobytes() == rows.tobytes()
    got = cuking_amd.ibd_segments_host(inp.bits(), inp.wps, case.sites, inp.pairs, min_sites=150)
    assert got.bridge_sites == 0 and got.bridged is None and got.segments1[0] == 2


def _raw_host(inp, bridge_sites, null_bridged=False, **over):
    """cuking_ibd_pairs_bridged_host with single arguments replaced; returns (status, out,
    bridged, segments, found)."""
    out = np.full(len(inp.index) * 10, 0xABABABAB, dtype=np.uint32)
    bridged = np.full((len(inp.index), 2), 0xABABABAB, dtype=np.uint32)
    segments = np.zeros(16, dtype=ibd.IBD_SEGMENT_DTYPE)
    found = C.c_uint64(77)
    bits, pairs = inp.bits(), np.ascontiguousarray(inp.pairs)
    pointers = dict(bits=bits.ctypes.data, group=None, pos=None, pairs=pairs.ctypes.data,
                    out=out.ctypes.data, segments=segments.ctypes.data, found=C.byref(found),
                    bridged=None if null_bridged else bridged.ctypes.data)
    st = _lib.load().cuking_ibd_pairs_bridged_host(
        *bc.bridged_arguments(inp, pointers, bridge_sites, **over))
    return st, out, bridged, segments, found.value


@pytest.mark.parametrize("case", ic.CASES, ids=lambda c: c.name)
def test_bridge_sites_zero_is_the_strict_call(case):
    inp = ic.inputs(case)
    want_rows, want_segments = ic.run_host(case)
    out = np.zeros(len(inp.index), dtype=ibd.IBD_PAIR_DTYPE)
    bridged = np.full((len(inp.index), 2), 7, dtype=np.uint32)
    segments = np.zeros(max(1, len(want_segments)), dtype=ibd.IBD_SEGMENT_DTYPE)
    found = C.c_uint64(0)
    bits, pairs = inp.bits(), np.ascontiguousarray(inp.pairs)
    st = _lib.load().cuking_ibd_pairs_bridged_host(
        bits.ctypes.data, case.samples, inp.wps, case.sites,
        None if inp.group is None else inp.group.ctypes.data,
        None if inp.pos is None else inp.pos.ctypes.data, case.min_sites, case.min_length, 0,
        pairs.ctypes.data, len(inp.index), case.stride, out.ctypes.data, bridged.ctypes.data,
        segments.ctypes.data, len(segments), C.byref(found))
    assert st == _lib.OK and found.value == len(want_segments)
    assert out.tobytes() == want_rows.tobytes() and not bridged.any()
    assert ibd.sort_segments(segments[:found.value]).tobytes() == \
        ibd.sort_segments(want_segments).tobytes()


@pytest.mark.parametrize("name", ic.REFUSALS)
def test_the_refusals_of_the_strict_call(name):
    inp = ic.inputs(ic.REFUSAL_CASE)
    st, out, bridged, _, _ = _raw_host(inp, 64, **ic.REFUSALS[name])
    assert st == _lib.ERR_INVALID_ARGUMENT, name
    assert (out == 0xABABABAB).all() and (bridged == 0xABABABAB).all()
    assert _lib.load().cuking_last_error().decode()


@pytest.mark.parametrize("bridge_sites", (1, 63))
def test_bridge_sites_below_64_are_refused(bridge_sites):
    inp = ic.inputs(ic.REFUSAL_CASE)
    st, out, bridged, _, _ = _raw_host(inp, bridge_sites)
    assert st == _lib.ERR_INVALID_ARGUMENT
    assert (out == 0xABABABAB).all() and (bridged == 0xABABABAB).all()
    message = _lib.load().cuking_last_error().decode()
    assert "bridge_sites" in message and str(bridge_sites) in message and "64" in message
    with pytest.raises(cuking_amd.CukingError, match="bridge_sites"):
        ibd.ibd_segments_raw_host(inp.bits(), inp.wps, ic.REFUSAL_CASE.sites, inp.index,
                                  bridge_sites=bridge_sites)


def test_a_null_bridged_is_accepted_and_the_list_overflows_as_before():
    case = next(c for c in bc.CASES if c.name.startswith("sixteen samples"))
    inp = bc.inputs(case)
    want_rows, want_bridged, want_segments = bc.reference(case)
    kw = {}
    for null in (False, True):
        st, out, bridged, segments, found = _raw_host(inp, case.bridge, null_bridged=null, **kw)
        assert st == _lib.OK and found == len(want_segments) <= 16
        assert out.view(ibd.IBD_PAIR_DTYPE).tobytes() == want_rows.tobytes()
        assert ibd.sort_segments(segments[:found]).tobytes() == want_segments.tobytes()
        if not null:
            assert bridged.tobytes() == want_bridged.tobytes()
    total = len(want_segments)
    for room in (total - 1, 0):
        with pytest.raises(cuking_amd.ResourceExhaustedError) as e:
            bc.run_host(case, max_segments=room)
        assert e.value.num_segments == total
    st, out, bridged, _, found = _raw_host(inp, case.bridge, max_segments=2, **kw)
    assert st == _lib.ERR_RESOURCE_EXHAUSTED and found == total
    assert out.view(ibd.IBD_PAIR_DTYPE).tobytes() == want_rows.tobytes()
    assert bridged.tobytes() == want_bridged.tobytes()
    # the calls without work
    st, out, bridged, _, found = _raw_host(inp, 64, num_pairs=0, pairs=None, out=None, bits=None)
    assert st == _lib.OK and (out == 0xABABABAB).all() and found == 0


def test_a_row_depends_on_its_own_pair_only():
    case = next(c for c in bc.CASES if c.name.startswith("breaks at bit 63"))
    inp = bc.inputs(case)
    whole, _, bridged = bc.run_host(case)
    args = (inp.bits(), inp.wps, case.sites)
    kw = dict(min_sites=case.min_sites, bridge_sites=case.bridge)
    order = np.random.default_rng(3).permutation(len(inp.index))[:20]
    moved, _, moved_bridged = ibd.ibd_segments_raw_host(
        *args, np.ascontiguousarray(inp.index[order]), **kw)
    assert moved.tobytes() == whole[order].tobytes()
    assert moved_bridged.tobytes() == bridged[order].tobytes() and moved_bridged.any()
    swapped, _, swapped_bridged = ibd.ibd_segments_raw_host(
        *args, np.ascontiguousarray(inp.index[:, ::-1]), **kw)
    assert swapped_bridged.tobytes() == bridged.tobytes()
    for name in ibd.IBD_PAIR_DTYPE.names[2:]:
        assert swapped[name].tobytes() == whole[name].tobytes(), name
    # out of range: zeros
    outside = (whole["sample_i"] >= case.samples) | (whole["sample_j"] >= case.samples)
    assert outside.sum() == 2 and not bridged[outside].any()


def test_host_side_under_asan_ubsan(tmp_path):
    """csrc/king_host.cc and a stand-alone driver (tests/ibd_bridge_host_driver.cc) built with
    AddressSanitizer + UBSan.  A program of its own on the CPU: nothing is loaded into Python."""
    run_sanitized_driver(tmp_path, "ibd_bridge_host_driver")


# ---- the end-to-end check on the synthetic cohort with genotyping errors ------------------------
# One genotype in E2E_RATE of the second sample of every parent-child and duplicate pair is
# replaced by another called genotype (seed E2E_SEED).  Chosen on the CPU from the naive walk
# alone, the first of the rates 1/800, 1/400, 1/200 at which the strict call loses a relationship
# code while bridge_sites = 64, the smallest legal value, gives every error-free code back.
E2E_RATE, E2E_SEED, E2E_BRIDGE = 1 / 400, 11, 64


def decode(bits, num_sites):
    """Codes uint8 [samples, num_sites] of a sample-major bitset."""
    planes = np.unpackbits(np.ascontiguousarray(bits).view(np.uint8).reshape(len(bits), 2, -1),
                           axis=2, bitorder="little")
    return (planes[:, 0, :num_sites] | planes[:, 1, :num_sites] << 1).astype(np.uint8)


def with_errors(clean, index, labels):
    """The codes with E2E_RATE of the called genotypes of the second sample of every related
    pair replaced by another called genotype."""
    noisy = clean.copy()
    rng = np.random.default_rng(E2E_SEED)
    for (_, b), label in zip(index, labels):
        if label == "none":
            continue
        sites = np.flatnonzero((rng.random(clean.shape[1]) < E2E_RATE) & (noisy[b] != 3))
        noisy[b, sites] = (noisy[b, sites] + rng.integers(1, 3, size=len(sites))) % 3
    return noisy


@lru_cache(maxsize=None)
def e2e_codes(oracle):
    """(error-free codes, codes with errors, words_per_sample) of the cohort of smoke()."""
    n, m, seed = E2E
    cohort, index, labels = e2e_cohort()
    bits = oracle.synth_bitset(seed, cohort.kind, cohort.pa, cohort.pb, 0, n, m)
    clean = decode(bits, m)
    return clean, with_errors(clean, index, labels), bits.shape[1]


def naive_pairs(code, index, bridge_sites):
    n, m, _ = E2E
    rows, bridged, _ = bc.naive(code, m, index, None, None, 512, 0, bridge_sites)
    return ibd.IBDPairs(rows, m - 1, None, 512, 0, bridge_sites, bridged)


def check_e2e_errors(clean, strict, bridged, labels):
    """IBDPairs of the error-free cohort and of the cohort with errors, strict and bridged."""
    related = labels != "none"
    want = clean.relationship()
    assert set(want[related].tolist()) == {pcr.PARENT_CHILD, pcr.DUPLICATE}
    assert (strict.relationship() != want).any()
    assert (bridged.relationship() == want).all()
    assert bridged.bridged[related].sum() > 20 and not bridged.bridged[~related].any()
    # no unrelated pair gains a segment
    for got in (strict, bridged):
        assert not got.segments1[~related].any() and not got.segments2[~related].any()


def test_end_to_end_on_the_host(oracle):
    n, m, _ = E2E
    _, index, labels = e2e_cohort()
    clean, noisy, wps = e2e_codes(oracle)
    # the choice of the rate and of bridge_sites holds on the naive walk alone
    naive_clean = naive_pairs(clean, index, 0)
    naive_bridged = naive_pairs(noisy, index, E2E_BRIDGE)
    check_e2e_errors(naive_clean, naive_pairs(noisy, index, 0), naive_bridged, labels)
    # ... and the host twin gives the naive walk's bytes
    bits = ic.pack_codes(noisy, wps // 2, ones_padding=True)
    strict = cuking_amd.ibd_segments_host(bits, wps, m, index)
    bridged = cuking_amd.ibd_segments_host(bits, wps, m, index, bridge_sites=E2E_BRIDGE)
    assert bridged.rows.tobytes() == naive_bridged.rows.tobytes()
    assert bridged.bridged.tobytes() == naive_bridged.bridged.tobytes()
    check_e2e_errors(naive_clean, strict, bridged, labels)
