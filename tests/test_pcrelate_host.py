"""PC-Relate without a GPU: the host twin against the integer formula and the float64 reference
of pcrelate_cases.py, the teeth of the tolerance, the refusals, the stand-alone sanitizer
driver, and the end-to-end fixture through pca_host -> pcrelate_host."""
import ctypes as C
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

import pcrelate_cases as pc
from host_driver import run_sanitized_driver

import cuking_amd
from cuking_amd import _lib
from cuking_amd.pcrelate import pcrelate_matrix_host

ROOT = Path(__file__).resolve().parent.parent


@lru_cache(maxsize=None)
def host_backend(case):
    inp = pc.inputs(case)
    rows, cols = case.block[1] - case.block[0], case.block[3] - case.block[2]
    wide = np.full((rows, cols + case.pad), np.float32(-7.0), dtype=np.float32)
    out = pcrelate_matrix_host(inp.bits, inp.wps, case.sites, inp.x, inp.beta, inp.lo, inp.hi,
                               block=case.block, out=wide[:, :cols])
    assert (wide[:, cols:] == -7.0).all()     # nothing between the columns and the pitch
    return np.ascontiguousarray(out)


@pytest.mark.parametrize("case", pc.EXACT_CASES, ids=lambda c: c.name)
def test_host_twin_exact(case):
    pc.check_exact(case, host_backend)


@pytest.mark.parametrize("case", pc.REAL_CASES, ids=lambda c: c.name)
def test_host_twin_against_float64_reference(case):
    pc.check_reference(case, host_backend, "host twin")


@pytest.mark.parametrize("d", range(1, 33))
def test_ladder_host_twin_against_float64_reference(d):
    """Every d from 1 to 32 at 130 samples x 97 sites, the whole block and (5, 70, 97, 130):
    the rungs the GPU test climbs, so that a fault of the generator shows without a GPU."""
    for block in pc.LADDER_BLOCKS:
        case = pc.ladder_case(d, block)
        assert pc.reference(case).margin_violations() == 0
        pc.check_reference(case, host_backend, "host twin")


@pytest.mark.parametrize("case", pc.REAL_CASES, ids=lambda c: c.name)
def test_real_cases_keep_their_distance_from_the_bounds(case):
    ref = pc.reference(case)
    assert ref.margin_violations() == 0
    if case.sites >= 63:    # the case exercises both kinds of element
        assert (ref.called & ~ref.valid).any() and ref.valid.any()


def test_the_tolerance_has_teeth():
    """Each defect moves some entry of each real-valued case by at least 10 of that entry's
    tolerances, and does nothing at all where the case is immune to it by construction."""
    smallest, largest_tol = float("inf"), 0.0
    for case in pc.REAL_CASES:
        ref = pc.reference(case)
        ok = ~np.isnan(ref.kin)
        if ok.any():
            largest_tol = max(largest_tol, ref.tolerance()[ok].max())
        for defect in pc.DEFECTS:
            ratio = pc.defect_ratio(case, defect)
            print(f"{case.name}: {defect} moves an entry by {ratio:.3g} tolerances")
            if defect in case.immune:
                assert ratio == 0.0, (case.name, defect, ratio)
                continue
            assert ratio >= 10.0, (case.name, defect, ratio)
            smallest = min(smallest, ratio)
    print(f"largest tolerance {largest_tol:.3g}, smallest defect {smallest:.3g} tolerances")


def test_zero_sites_write_nan_and_empty_blocks_write_nothing():
    inp = pc.inputs(pc.CASES[4])
    out = pcrelate_matrix_host(inp.bits, inp.wps, 0, inp.x, inp.beta, inp.lo, inp.hi)
    assert out.shape == (33, 33) and np.isnan(out).all()
    out = pcrelate_matrix_host(inp.bits, inp.wps, 63, inp.x, inp.beta, inp.lo, inp.hi,
                               block=(4, 4, 9, 20))
    assert out.shape == (0, 11)


def _raw_host(inp, **over):
    """cuking_pcrelate_matrix_host with single arguments replaced; returns (status, out)."""
    case = inp.case
    a = dict(bits=inp.bits.ctypes.data, num_stored=case.n, wps=inp.wps, sites=case.sites,
             x=inp.x.ctypes.data, ldx=inp.x.strides[0] // 4, beta=inp.beta.ctypes.data,
             ldbeta=inp.beta.strides[0] // 4, d=case.d, lo=inp.lo, hi=inp.hi,
             block=(0, case.n, 0, case.n), ldo=case.n)
    a.update(over)
    out = np.full((case.n, case.n), np.float32(-7.0), dtype=np.float32)
    block = _lib.CSubmatrix(*a["block"])
    st = _lib.load().cuking_pcrelate_matrix_host(
        a["bits"], a["num_stored"], a["wps"], a["sites"], a["x"], a["ldx"], a["beta"],
        a["ldbeta"], a["d"], a["lo"], a["hi"], C.byref(block),
        a.get("out", out.ctypes.data), a["ldo"])
    return st, out


REFUSALS = pc.REFUSALS


@pytest.mark.parametrize("name", REFUSALS)
def test_host_refusals(name):
    inp = pc.inputs(pc.CASES[4])    # 33 samples x 63 sites, d = 3, two plane words
    st, out = _raw_host(inp, **REFUSALS[name])
    assert st == _lib.ERR_INVALID_ARGUMENT, name
    assert (out == -7.0).all()
    message = _lib.load().cuking_last_error().decode()
    assert message and any(ch.isdigit() for ch in message) or "null" in message, message
    st, out = _raw_host(inp)
    assert st == _lib.OK and not (out == -7.0).any()


def test_wrapper_refusals():
    inp = pc.inputs(pc.CASES[4])
    args = (inp.bits, inp.wps, 63, inp.x, inp.beta)
    with pytest.raises(cuking_amd.CukingError):
        pcrelate_matrix_host(*args, 0.5, 0.5)
    with pytest.raises(cuking_amd.CukingError):
        pcrelate_matrix_host(*args, inp.lo, inp.hi, block=(0, 40, 0, 40))
    with pytest.raises(ValueError):
        pcrelate_matrix_host(inp.bits, inp.wps, 63, inp.x, inp.beta[:, :2], inp.lo, inp.hi)
    with pytest.raises(ValueError):
        pcrelate_matrix_host(inp.bits, inp.wps, 63, inp.x.astype(np.float64), inp.beta, 0.1, 0.9)
    inp = pc.inputs(pc.CASES[5])    # 130 samples x 64 sites: a bitset without spare words
    assert (inp.case.n, inp.case.sites, inp.wps) == (130, 64, 2)
    scores = np.ascontiguousarray(inp.x[:, 1:])
    with pytest.raises(ValueError, match="rank"):
        cuking_amd.pcrelate_host(inp.bits, 2, 64, np.zeros((130, 2), dtype=np.float32))
    with pytest.raises(ValueError, match="fit samples"):
        cuking_amd.pcrelate_host(inp.bits, 2, 64, scores, fit=np.arange(130) < 11)
    with pytest.raises(ValueError, match="min_maf"):
        cuking_amd.pcrelate_host(inp.bits, 2, 64, scores, min_maf=0.5)
    with pytest.raises(ValueError, match="no used site"):
        cuking_amd.pcrelate_host(np.zeros_like(inp.bits), 2, 64, scores)
    with pytest.raises(ValueError, match="exceeds"):
        cuking_amd.pcrelate_host(inp.bits, 2, 64, np.zeros((130, 32), dtype=np.float32))


def test_constants_agree():
    text = (ROOT / "include" / "cuking_amd.h").read_text()
    assert f"#define CUKING_PCRELATE_COLUMNS_MAX {_lib.PCRELATE_COLUMNS_MAX}\n" in text
    shared = (ROOT / "cuking_amd" / "csrc" / "king_pcrelate.h").read_text()
    assert "constexpr uint32_t kPcrelateColumnsMax = 32;" in shared


def test_host_side_under_asan_ubsan(tmp_path):
    """csrc/king_host.cc and a stand-alone driver (tests/pcrelate_host_driver.cc) built with
    AddressSanitizer + UBSan and without contraction.  A program of its own on the CPU: nothing
    is loaded into Python."""
    run_sanitized_driver(tmp_path, "pcrelate_host_driver")


def test_end_to_end_on_the_host(naive):
    from site_qc_cases import pack
    geno, population, fit, _ = pc.e2e_cohort()
    bits = pack(np.asarray(geno))
    wps = bits.shape[1]
    pca = cuking_amd.pca_host(bits, wps, pc.E2E_SITES, k=pc.E2E_K, fit=fit)
    result = cuking_amd.pcrelate_host(bits, wps, pc.E2E_SITES, pca.scores[:, :pc.E2E_K],
                                      fit=pca.fit)
    pc.check_e2e(result, bits, naive)
