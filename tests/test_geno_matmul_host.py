"""Genotype matrix products, CPU side: the host twin (the specification in executable form)
against the dense float64 reference over the shared case list -- exact for integer operands,
within the accumulation bound for real ones --, its output rules, the refusals of both entry
points, the header, and the host code under AddressSanitizer + UBSan.  No GPU."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from geno_cases import CASES, check_both_layouts, check_bound, check_exact, refusals
from host_driver import compile_c99, run_sanitized_driver

import cuking_amd
from cuking_amd import _lib

ROOT = Path(__file__).resolve().parent.parent


def run_host(bits, words_per_row, num_cols, table, per_row, b_full, num_rhs, out_full):
    cuking_amd.geno_matmul_host(bits, words_per_row, num_cols, table, b_full[:, :num_rhs],
                                per_row=per_row, out=out_full[:, :num_rhs])
    return out_full


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_exact_for_integer_operands(case):
    check_exact(run_host, case)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_within_the_accumulation_bound(case):
    check_bound(run_host, case)


def test_both_layouts_against_one_reference():
    check_both_layouts(
        run_host, lambda bits, wps, m: cuking_amd.transpose_sites_host(bits, wps, m).reshape(m, -1))


def test_known_answer_from_the_definition():
    """2 rows x 3 columns: codes (0, 1, 3) and (2, 2, 1), a per-column table and B = [1, 10,
    100]^T written out by hand."""
    bits = np.zeros((2, cuking_amd.words_per_sample(3)), dtype=np.uint64)
    plane = bits.shape[1] // 2
    bits[0, 0], bits[0, plane] = 0b110, 0b100         # het bits, hom_var bits
    bits[1, 0], bits[1, plane] = 0b100, 0b011
    table = np.float32([[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12]])
    b = np.float32([[1], [10], [100]])
    got = cuking_amd.geno_matmul_host(bits, bits.shape[1], 3, table, b)
    assert got.tolist() == [[1 * 1 + 6 * 10 + 12 * 100], [3 * 1 + 7 * 10 + 10 * 100]]
    rows = np.float32([[1, 2, 3, 4], [5, 6, 7, 8]])
    got = cuking_amd.geno_matmul_host(bits, bits.shape[1], 3, rows, b, per_row=True)
    assert got.tolist() == [[1 * 1 + 2 * 10 + 4 * 100], [7 * 1 + 7 * 10 + 6 * 100]]
    # no columns: zeros
    out = np.full((2, 1), np.nan, dtype=np.float32)
    cuking_amd.geno_matmul_host(bits, bits.shape[1], 0, table[:0], b[:0], out=out)
    assert out.tolist() == [[0.0], [0.0]]


def abi_arguments(kw):
    bits = np.zeros((5, 4), dtype=np.uint64)
    table = np.ones((70, 4), dtype=np.float32)
    b = np.ones((70, 3), dtype=np.float32)
    out = np.zeros((5, 3), dtype=np.float32)
    a = dict(bits=bits.ctypes.data, num_rows=5, words_per_row=4, num_cols=70,
             table=table.ctypes.data, axis=_lib.GENO_TABLE_PER_COLUMN, b=b.ctypes.data, ldb=3,
             num_rhs=3, out=out.ctypes.data, ldo=3)
    a.update(kw)
    keep = (bits, table, b, out)
    return a, keep


def test_refused_arguments():
    lib = _lib.load()

    def host(**kw):
        a, _keep = abi_arguments(kw)
        status = lib.cuking_geno_matmul_host(a["bits"], a["num_rows"], a["words_per_row"],
                                             a["num_cols"], a["table"], a["axis"], a["b"],
                                             a["ldb"], a["num_rhs"], a["out"], a["ldo"])
        return status, lib.cuking_last_error().decode()
    refusals(host)
    # the device entry point checks its arguments before it touches a device: no context
    a, _keep = abi_arguments({})
    assert lib.cuking_geno_matmul(None, a["bits"], 5, 4, 70, a["table"], 0, a["b"], 3, 3,
                                  a["out"], 3, None) == _lib.ERR_INVALID_ARGUMENT
    # ... and the Python function
    bits = np.zeros((5, 4), dtype=np.uint64)
    with pytest.raises(ValueError, match="table"):
        cuking_amd.geno_matmul_host(bits, 4, 70, np.ones((69, 4), np.float32),
                                    np.ones((70, 3), np.float32))
    with pytest.raises(ValueError, match="rhs"):
        cuking_amd.geno_matmul_host(bits, 4, 70, np.ones((70, 4), np.float32),
                                    np.ones((70, 3), np.float64))
    with pytest.raises(ValueError, match="out"):
        cuking_amd.geno_matmul_host(bits, 4, 70, np.ones((70, 4), np.float32),
                                    np.ones((70, 3), np.float32), out=np.zeros((5, 2), np.float32))
    with pytest.raises(cuking_amd.CukingError, match="num_rhs"):
        cuking_amd.geno_matmul_host(bits, 4, 70, np.ones((70, 4), np.float32),
                                    np.ones((70, 65), np.float32))


def test_shared_constants():
    text = (ROOT / "include" / "cuking_amd.h").read_text()
    for name, value in (("CUKING_GENO_RHS_MAX", _lib.GENO_RHS_MAX),
                        ("CUKING_GENO_TABLE_PER_COLUMN", _lib.GENO_TABLE_PER_COLUMN),
                        ("CUKING_GENO_TABLE_PER_ROW", _lib.GENO_TABLE_PER_ROW)):
        assert f"#define {name} {value}\n" in text, name
    geno_h = (ROOT / "cuking_amd" / "csrc" / "king_geno.h").read_text()
    assert "constexpr uint32_t kGenoRhsMax = 64;" in geno_h


def test_header_is_still_plain_c(tmp_path):
    compile_c99(tmp_path, """
#include "cuking_amd.h"
int use(const uint64_t *bits, const float *table, const float *b, float *out) {
  cuking_status (*device)(cuking_ctx *, const uint64_t *, uint32_t, uint32_t, uint32_t,
                          const float *, int, const float *, uint32_t, uint32_t, float *, uint32_t,
                          void *) = cuking_geno_matmul;
  (void)device;
  return (int)cuking_geno_matmul_host(bits, 5, 4, 70, table, CUKING_GENO_TABLE_PER_ROW, b, 3, 3,
                                      out, CUKING_GENO_RHS_MAX);
}
""")


def test_host_side_under_asan_ubsan(tmp_path):
    """csrc/king_host.cc and a stand-alone driver (tests/geno_matmul_host_driver.cc: exact-size
    heap buffers, the host product against the definition on plain code arrays, the refusals)
    built with AddressSanitizer + UBSan.  A program of its own on the CPU: nothing is loaded
    into Python."""
    run_sanitized_driver(tmp_path, "geno_matmul_host_driver")
