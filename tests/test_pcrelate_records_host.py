"""PC-Relate records without a GPU: the host twin against pcrelate_matrix_host thresholded and
against the float64 reference at the gap thresholds of pcrelate_records_cases.py, the counts at
-inf and +inf, the refusals, the overflow rule, the tile map of a diagonal block, the
stand-alone sanitizer driver, and the end-to-end fixture through pca_host ->
pcrelate_records_host."""
import ctypes as C
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

import pcrelate_cases as pc
import pcrelate_records_cases as rc
from host_driver import run_sanitized_driver

import cuking_amd
from cuking_amd import KING_RESULT_DTYPE, _lib
from cuking_amd.pcrelate import pcrelate_matrix_host, pcrelate_records_raw_host

ROOT = Path(__file__).resolve().parent.parent


@lru_cache(maxsize=None)
def host_matrix(case):
    inp = pc.inputs(case)
    return pcrelate_matrix_host(inp.bits, inp.wps, case.sites, inp.x, inp.beta, inp.lo, inp.hi,
                                block=case.block)


def host_records(case, min_kin, **kw):
    inp = pc.inputs(case)
    return pcrelate_records_raw_host(inp.bits, inp.wps, case.sites, inp.x, inp.beta, inp.lo,
                                     inp.hi, min_kin, block=case.block, **kw)


@pytest.mark.parametrize("case", rc.CASES, ids=lambda c: c.name)
def test_host_records_equal_the_host_matrix_thresholded(case):
    """The (i, j) set, the kin bytes and the ascending order, at every threshold."""
    for t in rc.thresholds(case):
        got, count = host_records(case, t)
        want = rc.threshold_matrix(host_matrix(case), case.block, t)
        assert count == got.shape[0] == want.shape[0], (t, count, want.shape)
        rc.check_records(got, case.block)
        rc.same_records(got, want)      # (no sort: the host twin's order IS ascending (i, j))


@pytest.mark.parametrize("d", range(1, 33))
def test_ladder_host_records_against_float64_reference(d):
    """Every d from 1 to 32 at 130 samples x 97 sites, the whole block and (5, 70, 97, 130):
    at -inf the records are the reference's pairs of defined kinship, each within tolerance,
    and the host matrix thresholded; the rungs the GPU test climbs."""
    for block in pc.LADDER_BLOCKS:
        case = pc.ladder_case(d, block)
        got, count = host_records(case, -rc.INF)
        assert count == got.shape[0]
        rc.check_records_reference(pc.reference(case), block, got, case.name, "host twin")
        rc.same_records(got, rc.threshold_matrix(host_matrix(case), block, -rc.INF))


@pytest.mark.parametrize("case", rc.CASES, ids=lambda c: c.name)
def test_gap_thresholds_equal_the_float64_reference(case):
    ref = pc.reference(case)
    for gap in rc.gap_thresholds(case):
        print(f"{case.name}: threshold {gap.threshold:.6g} at rank {gap.rank} (target "
              f"{gap.target_rank}), nearest pair {gap.margin:.3g} tolerances away")
        got, _ = host_records(case, gap.threshold)
        want = rc.threshold_matrix(ref.kin, case.block, gap.threshold)
        assert 0 < want.shape[0] < rc.num_pairs(case.block)
        assert np.array_equal(got["sample_i"], want["sample_i"])
        assert np.array_equal(got["sample_j"], want["sample_j"])


@pytest.mark.parametrize("case", rc.CASES, ids=lambda c: c.name)
def test_counts_at_the_infinities(case):
    ref = pc.reference(case)
    nan_pairs = int((rc.pair_mask(case.block) & np.isnan(ref.kin)).sum())
    if case.exact and rc.is_diagonal(case.block):
        assert nan_pairs >= 1           # the planted pair (0, 1) and the all-missing sample
    _, count = host_records(case, -rc.INF)
    assert count == rc.num_pairs(case.block) - nan_pairs
    _, count = host_records(case, rc.INF)
    assert count == 0


def test_no_work_cases():
    inp = pc.inputs(pc.CASES[4])
    args = (inp.bits, inp.wps)
    tail = (inp.x, inp.beta, inp.lo, inp.hi, -rc.INF)
    assert pcrelate_records_raw_host(*args, 63, *tail, block=(4, 4, 9, 20))[1] == 0
    assert pcrelate_records_raw_host(*args, 63, *tail, block=(7, 8, 7, 8))[1] == 0
    assert pcrelate_records_raw_host(*args, 0, *tail)[1] == 0


def _raw_host(inp, slots=None, sentinel=3, **over):
    """cuking_pcrelate_records_host with single arguments replaced; returns (status, buffer,
    count): the buffer holds `slots` records and `sentinel` rows of 0xAB bytes behind them."""
    case = inp.case
    pairs = case.n * (case.n - 1) // 2
    slots = pairs if slots is None else slots
    buf = np.frombuffer(bytes([0xAB]) * (24 * (slots + sentinel)), dtype=KING_RESULT_DTYPE).copy()
    count = C.c_uint64(12345)
    a = dict(bits=inp.bits.ctypes.data, num_stored=case.n, wps=inp.wps, sites=case.sites,
             x=inp.x.ctypes.data, ldx=inp.x.strides[0] // 4, beta=inp.beta.ctypes.data,
             ldbeta=inp.beta.strides[0] // 4, d=case.d, lo=inp.lo, hi=inp.hi,
             block=(0, case.n, 0, case.n), min_kin=-rc.INF, records=buf.ctypes.data,
             max_records=slots, num_records=C.byref(count))
    a.update(over)
    block = _lib.CSubmatrix(*a["block"])
    st = _lib.load().cuking_pcrelate_records_host(
        a["bits"], a["num_stored"], a["wps"], a["sites"], a["x"], a["ldx"], a["beta"],
        a["ldbeta"], a["d"], a["lo"], a["hi"], C.byref(block), a["min_kin"], a["records"],
        a["max_records"], a["num_records"])
    return st, buf, int(count.value)


# the matrix call's refusals that concern the model and the block (not its `out` and `ldo`),
# and the records' own
REFUSALS = {k: {n: v for n, v in over.items() if n != "ldo"} for k, over in pc.REFUSALS.items()
            if k not in ("pitch below the columns", "null out")}
REFUSALS.update({
    "min_kin NaN": dict(min_kin=float("nan")),
    "null num_records": dict(num_records=None),
    "null records with room": dict(records=None),
})


@pytest.mark.parametrize("name", REFUSALS)
def test_host_refusals(name):
    inp = pc.inputs(pc.CASES[4])    # 33 samples x 63 sites, d = 3, two plane words
    st, buf, count = _raw_host(inp, **REFUSALS[name])
    assert st == _lib.ERR_INVALID_ARGUMENT, name
    assert (buf.view(np.uint8) == 0xAB).all()
    assert count == (12345 if name == "null num_records" else 0)
    assert _lib.load().cuking_last_error().decode()
    st, buf, count = _raw_host(inp)
    assert st == _lib.OK and count > 0


def test_wrapper_refusals():
    inp = pc.inputs(pc.CASES[4])
    args = (inp.bits, inp.wps, 63, inp.x, inp.beta, inp.lo, inp.hi)
    with pytest.raises(ValueError, match="NaN"):
        pcrelate_records_raw_host(*args, float("nan"))
    with pytest.raises(cuking_amd.CukingError):
        pcrelate_records_raw_host(*args, 0.0, block=(0, 40, 0, 40))
    with pytest.raises(ValueError, match="either scores or model"):
        cuking_amd.pcrelate_records_host(inp.bits, inp.wps, 63)


def test_overflow_counts_exactly_and_writes_nothing_behind_the_buffer():
    case = pc.CASES[4]
    inp = pc.inputs(case)
    t = rc.gap_thresholds(case)[0].threshold
    full, total = host_records(case, t)
    assert total > 1
    st, buf, count = _raw_host(inp, slots=total - 1, min_kin=t)
    assert st == _lib.ERR_RESOURCE_EXHAUSTED and count == total
    assert buf[:total - 1].tobytes() == full[:total - 1].tobytes()    # the first ones, in order
    assert (buf[total - 1:].view(np.uint8) == 0xAB).all()
    st, buf, count = _raw_host(inp, slots=0, min_kin=t, records=None)  # the counting call
    assert st == _lib.ERR_RESOURCE_EXHAUSTED and count == total
    assert (buf.view(np.uint8) == 0xAB).all()
    st, buf, count = _raw_host(inp, slots=total, min_kin=t)
    assert st == _lib.OK and count == total and buf[:total].tobytes() == full.tobytes()
    assert (buf[total:].view(np.uint8) == 0xAB).all()
    with pytest.raises(cuking_amd.ResourceExhaustedError) as e:
        host_records(case, t, max_records=total - 1)
    assert e.value.num_records == total
    # without max_records the wrapper retries: 257 samples have more pairs of defined kinship
    # than the default buffer's 16 records per sample
    big = next(c for c in rc.CASES if c.name == "exact 257x64")
    got, count = host_records(big, -rc.INF)
    assert count == got.shape[0] > 16 * 2 * big.n
    rc.same_records(got, rc.threshold_matrix(host_matrix(big), big.block, -rc.INF))


def _tile(lib, side, index):
    i, j = C.c_uint32(0), C.c_uint32(0)
    assert lib.cuking_pcrelate_triangle_tile(side, index, C.byref(i), C.byref(j)) == 1
    return i.value, j.value


def test_tile_map_is_the_row_major_triangle():
    lib = _lib.load()
    for side in range(1, 65):
        want = [(i, j) for i in range(side) for j in range(i, side)]
        assert lib.cuking_pcrelate_triangle_tiles(side) == len(want)
        for index, (i, j) in enumerate(want):
            assert _tile(lib, side, index) == (i, j)
            assert lib.cuking_pcrelate_triangle_index(side, i, j) == index
        i, j = C.c_uint32(0), C.c_uint32(0)
        assert lib.cuking_pcrelate_triangle_tile(side, len(want), C.byref(i), C.byref(j)) == 0


def test_tile_map_at_the_largest_side():
    """33554432 = ceil((2^32 - 1) / 128) tiles per side: the first and the last 1000 indices."""
    lib = _lib.load()
    side = _lib.PCRELATE_TRIANGLE_SIDE_MAX
    assert side == -(-(2 ** 32 - 1) // 128)
    total = side * (side + 1) // 2
    assert lib.cuking_pcrelate_triangle_tiles(side) == total
    for index in range(1000):           # row 0: (0, index)
        assert _tile(lib, side, index) == (0, index)
        assert lib.cuking_pcrelate_triangle_index(side, 0, index) == index
    # the last rows hold 1, 2, 3, ... tiles
    want, row = [], side - 1
    while len(want) < 1000:
        want = [(row, j) for j in range(row, side)] + want
        row -= 1
    for k, (i, j) in enumerate(want[-1000:]):
        index = total - 1000 + k
        assert _tile(lib, side, index) == (i, j), index
        assert lib.cuking_pcrelate_triangle_index(side, i, j) == index
    assert lib.cuking_pcrelate_triangle_tiles(side + 1) == 0
    assert lib.cuking_pcrelate_triangle_index(side, 5, 4) == 2 ** 64 - 1


def test_constants_agree():
    text = (ROOT / "include" / "cuking_amd.h").read_text()
    assert "#define CUKING_PCRELATE_TRIANGLE_SIDE_MAX (1ull << 25)\n" in text
    shared = (ROOT / "cuking_amd" / "csrc" / "king_pcrelate.h").read_text()
    assert "constexpr uint64_t kPcrelateTriangleSideMax = 1ull << 25;" in shared
    assert _lib.PCRELATE_TRIANGLE_SIDE_MAX == 1 << 25


def test_host_side_under_asan_ubsan(tmp_path):
    """csrc/king_host.cc and a stand-alone driver (tests/pcrelate_records_host_driver.cc) built
    with AddressSanitizer + UBSan and without contraction.  A program of its own on the CPU:
    nothing is loaded into Python."""
    run_sanitized_driver(tmp_path, "pcrelate_records_host_driver")


def test_end_to_end_on_the_host():
    """At min_kinship = 0.125 the records are exactly the 30 planted first-degree pairs: the
    fixture's own conditions (first degree in (0.177, 0.354), every other pair below 0.0884;
    pcrelate_cases.check_e2e asserts them on the reference) put every pair further from 0.125
    than any tolerance."""
    from site_qc_cases import pack
    geno, population, fit, related = pc.e2e_cohort()
    assert len(related) == 30
    bits = pack(np.asarray(geno))
    wps = bits.shape[1]
    pca = cuking_amd.pca_host(bits, wps, pc.E2E_SITES, k=pc.E2E_K, fit=fit)
    got = cuking_amd.pcrelate_records_host(bits, wps, pc.E2E_SITES,
                                           scores=pca.scores[:, :pc.E2E_K], fit=pca.fit,
                                           min_kinship=0.125)
    assert got.num_records == 30
    rows = got.sorted()
    rc.check_records(rows, (0, 132, 0, 132))
    assert rc.pair_set(rows) == {(min(i, j), max(i, j)) for i, j in related}
    assert (rows["kin"] > 0.177).all() and (rows["kin"] < 0.354).all()
    # the records feed pcrelate_pairs with the same model, and the unrelated set
    pairs = cuking_amd.pcrelate_pairs_host(bits, wps, pc.E2E_SITES, rows, model=got)
    assert np.array_equal(pairs.sample_i, rows["sample_i"])
    assert (pairs.relationship() >= cuking_amd.pcrelate.FULL_SIBLING).all()
    keep, _family = cuking_amd.unrelated_set_host(rows, 132)
    kept = keep == 1
    assert not any(kept[i] and kept[j] for i, j in related)
