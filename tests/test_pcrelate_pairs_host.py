"""PC-Relate for listed pairs without a GPU: the host twin against the integer formula and the
float64 reference of pcrelate_pairs_cases.py, the teeth of the tolerances, the refusals through
the raw ABI, the wrapper's errors, relationship() on hand-made values, the stand-alone sanitizer
driver, and the end-to-end fixture through pca_host -> pcrelate_pairs_host."""
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

import pcrelate_cases as pc
import pcrelate_pairs_cases as pp
from host_driver import run_sanitized_driver

import cuking_amd
from cuking_amd import _lib
from cuking_amd import pcrelate as pcr

ROOT = Path(__file__).resolve().parent.parent


@lru_cache(maxsize=None)
def host_backend(case):
    inp = pp.inputs(case)
    return pcr.pcrelate_pairs_raw_host(inp.bits, inp.wps, case.sites, inp.x, inp.beta, inp.lo,
                                       inp.hi, inp.pairs, inp.f)


@pytest.mark.parametrize("case", pp.EXACT_CASES, ids=lambda c: c.name)
def test_host_twin_exact(case):
    pp.check_exact(case, host_backend)


@pytest.mark.parametrize("case", pp.REAL_CASES, ids=lambda c: c.name)
def test_host_twin_against_float64_reference(case):
    pp.check_reference(case, host_backend, "host twin")


@pytest.mark.parametrize("d", range(1, 33))
def test_ladder_host_twin_against_float64_reference(d):
    """Every d from 1 to 32 at 130 samples x 97 sites, 513 pairs, both strides, with and
    without f: the rungs the GPU test climbs."""
    for case in pp.ladder(d):
        assert pp.reference(case).margin_violations() == 0
        pp.check_reference(case, host_backend, "host twin")


def test_the_case_list_covers_the_kernel_constants():
    text = (ROOT / "cuking_amd" / "csrc" / "king_pcrelate_pairs.hip").read_text()
    assert f"constexpr uint32_t kPairThreads = {pp.WORKGROUP_PAIRS};" in text
    assert f"constexpr uint32_t kPairStep = {pp.STEP};" in text
    pairs = {c.pairs for c in pp.CASES}
    assert {1, 63, 64, 65, 257, pp.WORKGROUP_PAIRS, pp.WORKGROUP_PAIRS + 1} <= pairs
    sites = {c.sites for c in pp.CASES}
    assert {1, 63, 64, 65, 700, 2 * pp.STEP, 2 * pp.STEP + 1} <= sites
    assert {c.d for c in pp.REAL_CASES} == {1, 3, 11, 32}
    assert {c.stride for c in pp.CASES} == {8, 24} and {c.f for c in pp.REAL_CASES} == {0, 1}
    header = (ROOT / "include" / "cuking_amd.h").read_text()
    assert "#define CUKING_PCRELATE_K0_SWITCH 0.17677669529663689f" in header
    assert np.float32(_lib.PCRELATE_K0_SWITCH) == pp.SWITCH
    assert pp.SWITCH.view(np.uint32) == 0x3E3504F3
    assert pcr.PCRELATE_PAIR_DTYPE.itemsize == 32


def test_the_tolerances_have_teeth():
    """Each defect moves some value of each real-valued case by at least 10 of that value's
    tolerances, and does nothing at all where the case is immune to it by construction."""
    smallest = (float("inf"), "", "")
    for case in pp.REAL_CASES:
        for defect in pp.DEFECTS:
            ratio = pp.defect_ratio(case, defect)
            print(f"{case.name}: {defect} moves a value by {ratio:.3g} tolerances")
            if defect in case.immune:
                assert ratio == 0.0, (case.name, defect, ratio)
                continue
            assert ratio >= 10.0, (case.name, defect, ratio)
            smallest = min(smallest, (ratio, defect, case.name))
    print(f"smallest defect: {smallest[0]:.3g} tolerances ({smallest[1]} on {smallest[2]})")


def test_a_row_depends_on_its_own_pair_only():
    case = next(c for c in pp.CASES if c.name == "P257 S700 d3")
    inp, whole = pp.inputs(case), host_backend(case)
    args = (inp.bits, inp.wps, case.sites, inp.x, inp.beta, inp.lo, inp.hi)
    order = np.random.default_rng(3).permutation(case.pairs)[:100]
    moved = pcr.pcrelate_pairs_raw_host(*args, np.ascontiguousarray(inp.index[order]), inp.f)
    assert moved.tobytes() == whole[order].tobytes()
    # the indices swapped: everything but sample_i and sample_j is the same bytes
    swapped = pcr.pcrelate_pairs_raw_host(*args, np.ascontiguousarray(inp.index[:, ::-1]), inp.f)
    assert np.array_equal(swapped["sample_i"], whole["sample_j"])
    for name in pp.FLOATS + ("ibs0", "sites"):
        assert swapped[name].tobytes() == whole[name].tobytes(), name
    # the other stride
    recs = np.zeros(case.pairs, dtype=cuking_amd.KING_RESULT_DTYPE)
    recs["sample_i"], recs["sample_j"] = inp.index[:, 0], inp.index[:, 1]
    assert pcr.pcrelate_pairs_raw_host(*args, recs, inp.f).tobytes() == whole.tobytes()
    words = recs.view(np.uint32).reshape(-1, 6)
    part = pcr.pcrelate_pairs_raw_host(*args, words, inp.f, num_records=50)
    assert part.tobytes() == whole[:50].tobytes()


def test_zero_sites_write_the_nan_rows_and_an_empty_list_is_ok():
    case = pp.REFUSAL_CASE
    inp = pp.inputs(case)
    rows = pcr.pcrelate_pairs_raw_host(inp.bits, inp.wps, 0, inp.x, inp.beta, inp.lo, inp.hi,
                                       inp.pairs, inp.f)
    pp.check_rows(case, rows)
    for name in pp.FLOATS:
        assert np.isnan(rows[name]).all()
    assert not rows["ibs0"].any() and not rows["sites"].any()
    rows = pcr.pcrelate_pairs_raw_host(inp.bits, inp.wps, case.sites, inp.x, inp.beta, inp.lo,
                                       inp.hi, np.zeros((0, 2), dtype=np.uint32))
    assert rows.shape == (0,)


def _raw_host(inp, **over):
    """cuking_pcrelate_pairs_host with single arguments replaced; returns (status, out)."""
    case = inp.case
    out = np.full(case.pairs * 8, 0xABABABAB, dtype=np.uint32)
    pairs = np.ascontiguousarray(inp.pairs)
    pointers = dict(bits=inp.bits.ctypes.data, x=inp.x.ctypes.data, ldx=inp.x.strides[0] // 4,
                    beta=inp.beta.ctypes.data, ldbeta=inp.beta.strides[0] // 4, f=None,
                    pairs=pairs.ctypes.data, out=out.ctypes.data)
    st = _lib.load().cuking_pcrelate_pairs_host(*pp.raw_arguments(inp, pointers, **over))
    return st, out


@pytest.mark.parametrize("name", pp.REFUSALS)
def test_host_refusals(name):
    inp = pp.inputs(pp.REFUSAL_CASE)
    st, out = _raw_host(inp, **pp.REFUSALS[name])
    assert st == _lib.ERR_INVALID_ARGUMENT, name
    assert (out == 0xABABABAB).all()
    message = _lib.load().cuking_last_error().decode()
    assert message and any(ch.isdigit() for ch in message) or "null" in message, message
    st, out = _raw_host(inp)
    assert st == _lib.OK
    assert out.view(pcr.PCRELATE_PAIR_DTYPE).tobytes() == host_backend(pp.REFUSAL_CASE).tobytes()
    st, out = _raw_host(inp, num_pairs=0, pairs=None, out=None, bits=None, x=None, beta=None)
    assert st == _lib.OK and (out == 0xABABABAB).all()


def test_wrapper_errors():
    case = pp.REFUSAL_CASE
    inp = pp.inputs(case)
    args = (inp.bits, inp.wps, case.sites, inp.x, inp.beta)
    with pytest.raises(cuking_amd.CukingError):
        pcr.pcrelate_pairs_raw_host(*args, 0.5, 0.5, inp.pairs)
    with pytest.raises(ValueError):
        pcr.pcrelate_pairs_raw_host(*args, inp.lo, inp.hi, inp.index.astype(np.float32))
    with pytest.raises(ValueError):
        pcr.pcrelate_pairs_raw_host(*args, inp.lo, inp.hi, inp.index[:, :1])
    with pytest.raises(ValueError, match="num_records"):
        pcr.pcrelate_pairs_raw_host(*args, inp.lo, inp.hi, inp.index, num_records=3)
    with pytest.raises(ValueError, match="num_records"):
        pcr.pcrelate_pairs_raw_host(*args, inp.lo, inp.hi, inp.pairs, num_records=case.pairs + 1)
    with pytest.raises(ValueError, match="2\\^32"):
        pcr.pcrelate_pairs_raw_host(*args, inp.lo, inp.hi, np.array([[0, -1]]))
    with pytest.raises(ValueError, match="inbreeding"):
        pcr.pcrelate_pairs_raw_host(*args, inp.lo, inp.hi, inp.pairs, np.zeros(3, np.float32))
    scores = np.ascontiguousarray(inp.x[:, 1:3])
    small = (inp.bits, inp.wps, case.sites)
    with pytest.raises(ValueError, match="outside the 40 stored"):
        cuking_amd.pcrelate_pairs_host(*small, inp.pairs, scores=scores)
    good = np.array([[0, 1], [5, 5], [9, 3]], dtype=np.int64)
    with pytest.raises(ValueError, match="either scores or model"):
        cuking_amd.pcrelate_pairs_host(*small, good)
    with pytest.raises(ValueError, match="min_maf"):
        cuking_amd.pcrelate_pairs_host(*small, good, scores=scores, min_maf=0.5)
    with pytest.raises(ValueError, match="rank"):
        cuking_amd.pcrelate_pairs_host(*small, good, scores=np.zeros((40, 2), dtype=np.float32))
    with pytest.raises(ValueError, match="model must be"):
        cuking_amd.pcrelate_pairs_host(*small, good, model=object())
    first = cuking_amd.pcrelate_pairs_host(*small, good, scores=scores)
    again = cuking_amd.pcrelate_pairs_host(*small, good, model=first)
    assert again.rows.tobytes() == first.rows.tobytes()
    assert again.inbreeding.tobytes() == first.inbreeding.tobytes()
    assert np.isnan(first.inbreeding[2])          # the all-missing sample: a NaN stays NaN
    given = cuking_amd.pcrelate_pairs_host(*small, good, model=first,
                                           inbreeding=np.zeros(40, dtype=np.float32))
    assert given.kin.tobytes() == first.kin.tobytes() and not given.inbreeding.any()


def test_relationship_on_hand_made_values():
    f32 = np.float32
    thr = [f32(t) for t in cuking_amd.KING_CUTOFFS]
    up = lambda t: np.nextafter(t, f32(1.0))   # noqa: E731
    kin = [f32(-0.2), thr[0], up(thr[0]), thr[1], up(thr[1]), thr[2], up(thr[2]), f32(0.25),
           f32(0.25), f32(0.25), f32(0.25), thr[3], up(thr[3]), f32(np.nan), f32(0.6)]
    k0 = [f32(0.9)] * 7 + [f32(0.0), f32(0.1), np.nextafter(f32(0.1), f32(0.0)), f32(np.nan),
                           f32(0.0), f32(0.0), f32(0.0), f32(np.nan)]
    rows = np.zeros(len(kin), dtype=pcr.PCRELATE_PAIR_DTYPE)
    rows["kin"], rows["k0"] = kin, k0
    got = pcr.PCRelatePairs(rows, None, None, None, None, None)
    u, t3, t2, fs, po, dup = (pcr.UNRELATED, pcr.THIRD_DEGREE, pcr.SECOND_DEGREE,
                              pcr.FULL_SIBLING, pcr.PARENT_CHILD, pcr.DUPLICATE)
    want = [u, u, t3, t3, t2, t2, fs, po, fs, po, fs, po, dup, u, dup]
    assert got.relationship().tolist() == want
    assert got.relationship().dtype == np.uint8
    assert [pcr.RELATIONSHIP_NAMES[c] for c in (u, po)] == ["unrelated", "parent-child"]
    # the arguments: other cut-offs, another k0 bound
    assert got.relationship(parent_child_k0=0.05).tolist()[7:10] == [po, fs, fs]
    assert got.relationship(thresholds=(0.0, 0.1, 0.2, 0.7)).tolist()[-1] == fs
    with pytest.raises(ValueError):
        got.relationship(thresholds=(0.1, 0.05, 0.2, 0.3))


def test_host_side_under_asan_ubsan(tmp_path):
    """csrc/king_host.cc and a stand-alone driver (tests/pcrelate_pairs_host_driver.cc) built
    with AddressSanitizer + UBSan and without contraction.  A program of its own on the CPU:
    nothing is loaded into Python."""
    run_sanitized_driver(tmp_path, "pcrelate_pairs_host_driver")


# ---- the end-to-end fixture -------------------------------------------------------------------
def e2e_pairs():
    """(uint32 [P, 2], parent_child bool [P], sibling bool [P]): the planted first-degree pairs
    of pcrelate_pairs_cases.e2e_cohort() -- the fixture of pcrelate_cases.py at 8000 sites; the
    reason is beside it --, then unrelated founder pairs."""
    _, _, parent_child, siblings = pp.e2e_cohort()
    first = parent_child + siblings
    others = [(i, i + 7) for i in range(0, 30)] + [(i, 119 - i) for i in range(4, 30)]
    index = np.array(first + others, dtype=np.uint32)
    at = np.arange(len(index))
    return index, at < len(parent_child), (at >= len(parent_child)) & (at < len(first))


def check_e2e(result, code):
    """A PCRelatePairs of the end-to-end fixture: the conditions on the fixture on the float64
    reference fed with the backend's own x, beta and f, then the backend against it."""
    index, parent_child, sibling = e2e_pairs()
    lo, hi = float(np.float32(0.01)), float(np.float32(1.0) - np.float32(0.01))
    case = pp.Case("e2e", len(index), code.shape[1], result.x.shape[1])
    inp = pp.Inputs(case, code, None, result.x, result.beta, result.inbreeding, lo, hi, index,
                    index, 0)
    ref = pp.Reference(inp)
    kin, k0 = ref.value["kin"], ref.value["k0"]
    first = parent_child | sibling
    # -- conditions on the fixture
    assert parent_child.sum() == 24 and sibling.sum() == 6
    assert (k0[parent_child] < 0.1).all(), k0[parent_child].max()
    assert (k0[sibling] > 0.1).all(), k0[sibling].min()
    assert kin[first].min() > 0.177 and kin[first].max() < 0.354, (kin[first].min(),
                                                                   kin[first].max())
    assert kin[~first].max() < 0.0442, kin[~first].max()
    print(f"parent-child k0 <= {k0[parent_child].max():.3f}, sibling k0 >= "
          f"{k0[sibling].min():.3f}, first-degree kin {kin[first].min():.3f} .. "
          f"{kin[first].max():.3f}")
    # -- the backend against the reference, and its relationship codes
    assert ref.margin_violations() == 0
    assert np.array_equal(result.ibs0, ref.ibs0) and np.array_equal(result.sites, ref.sites)
    for name in pp.FLOATS:
        ratio = (np.abs(getattr(result, name) - ref.value[name]) / ref.tol[name]).max()
        print(f"{name}: largest error / tolerance {ratio:.3g}")
        assert ratio <= 1.0, name
    codes = result.relationship()
    assert (codes[parent_child] == pcr.PARENT_CHILD).all()
    assert (codes[sibling] == pcr.FULL_SIBLING).all()
    assert (codes[~first] == pcr.UNRELATED).all()
    return index, ref


def test_end_to_end_on_the_host():
    from site_qc_cases import pack
    geno, fit, _, _ = pp.e2e_cohort()
    bits = pack(np.asarray(geno))
    wps = bits.shape[1]
    code = np.where(geno < 0, 3, geno).astype(np.uint8)
    index, _, _ = e2e_pairs()
    pca = cuking_amd.pca_host(bits, wps, pp.E2E_SITES, k=pc.E2E_K, fit=fit)
    result = cuking_amd.pcrelate_pairs_host(bits, wps, pp.E2E_SITES, index,
                                            scores=pca.scores[:, :pc.E2E_K], fit=pca.fit)
    assert np.array_equal(result.fit, fit) and result.inbreeding.shape == (132,)
    check_e2e(result, code)
    # the twin's kin against the entries of the matrix twin
    n = geno.shape[0]
    lo, hi = float(np.float32(0.01)), float(np.float32(1.0) - np.float32(0.01))
    matrix = pcr.pcrelate_matrix_host(bits, wps, pp.E2E_SITES, result.x, result.beta, lo, hi)
    tol = pc.Reference(code, result.x, result.beta, lo, hi, (0, n, 0, n)).twin_tolerance()
    i, j = index[:, 0], index[:, 1]
    ratio = (np.abs(result.kin.astype(np.float64) - matrix[i, j]) / tol[i, j]).max()
    print(f"kin against the matrix twin: largest error / twin tolerance {ratio:.3g}")
    assert ratio <= 1.0
    # the self pairs behind `inbreeding`
    assert np.allclose(result.inbreeding, 2.0 * np.diagonal(matrix) - 1.0, atol=1e-4)
