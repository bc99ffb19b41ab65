"""The Hardy-Weinberg exact test without a GPU: the host twin against the Python restatement of
hwe_cases.py bit for bit on every case, the restatement against exact rational arithmetic, the
tie constant's margin, the paper's known answers, what the case lists cover, the mask arithmetic
of filter_sites, the refusals, the ABI symbols and the stand-alone sanitizer driver."""
import ctypes as C
import math
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import cuking_amd
from cuking_amd import _lib
from cuking_amd._lib import CukingError, check

import hwe_cases as hc
from host_driver import run_sanitized_driver

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("midp", [False, True])
def test_host_twin_equals_restatement_bitwise(midp):
    rows = hc.all_tables()
    counts = hc.counts_array(rows)
    got = cuking_amd.hwe_sites_host(counts, len(rows), midp=midp)
    assert got.dtype == np.float64 and got.shape == (len(rows),)
    want = hc.expected(midp)
    differ = np.flatnonzero(hc.bits(got) != hc.bits(want))
    assert differ.size == 0, [(rows[k], got[k].hex(), want[k].hex()) for k in differ[:5]]
    # int32 counts are the same bytes; fewer sites read fewer rows
    again = cuking_amd.hwe_sites_host(counts.view(np.int32), 100, midp=midp)
    assert hc.bits(again).tolist() == hc.bits(want[:100]).tolist()


def test_case_lists_cover_what_they_claim():
    rows = hc.all_tables()
    assert len(hc.small_tables()) == 2925 and len(hc.fuzz_tables()) == 2000
    assert 5000 <= len(rows) <= 5500
    p = hc.expected(False)
    assert np.isnan(p).sum() == 2 and (p == 0.0).sum() > 100 and (p == 1.0).sum() > 100
    assert ((p > 0) & (p < 1)).sum() > 2500
    fuzz = np.array(hc.fuzz_tables(), dtype=np.int64).sum(axis=1)
    assert fuzz.min() < 8 and fuzz.max() > (1 << 23) and fuzz.max() <= hc.MAX_PEOPLE
    edge = {why: hc.hwe_walk(*row) for row, why in hc.EDGE_ROWS}
    assert edge["n = 0"][0] == 1.0
    assert math.isnan(edge["n = 2^24 + 1: NaN"][0])
    assert edge["0.0 through the inf rule"][0] == 0.0
    assert edge["n = 2^24, r0 = 0: the down-walk overflows"][0] == 0.0
    assert edge["r0 = 0: no up-walk"][1] == 0 and edge["all hom"][2] == 0
    assert edge["down-walk ends in subnormals"][3]           # a subnormal term was summed
    assert edge["down-walk ends in subnormals"][2] < 45000 // 2  # ... and the walk ended at 0.0
    assert math.isclose(edge["down-walk ends in subnormals"][0], 1.54e-36, rel_tol=5e-3)
    assert edge["n = 2^24 at equilibrium"][0] == 1.0
    # mirrored rows are the same table
    assert edge["the same, mirrored"][0] == edge["down-walk ends in subnormals"][0]
    # mid-p only moves the last two operations
    assert hc.hwe_p(83, 13, 4, True) < hc.hwe_p(83, 13, 4, False)
    assert hc.hwe_p(0, 0, 0, True) == 1.0


def test_known_answers_of_the_paper():
    for row, printed in hc.WIGGINTON:
        assert abs(hc.hwe_p(*row) - printed) <= 1e-6, (row, hc.hwe_p(*row))
    got = cuking_amd.hwe_sites_host(hc.counts_array([r for r, _ in hc.WIGGINTON]), 3)
    assert np.abs(got - np.array([p for _, p in hc.WIGGINTON])).max() <= 1e-6


def test_restatement_against_rational_arithmetic():
    """n <= 24: at most 24 steps of two roundings plus the sums, below 200 * 2^-53 ~ 2e-14; 1e-12
    leaves a factor of 50 for the final division and the oracle's own conversion to float.  The
    tie constant decides nothing here: no term that is not an exact tie lies within 2^-20 of the
    observed one, so `t <= 1 + 2^-27` and the exact `t <= 1` select the same tables."""
    worst = 0.0
    margin = Fraction(1, 1 << 20)
    for row in hc.small_tables():
        if sum(row) == 0:
            continue
        for ratio in hc.table_terms(*row).values():
            assert ratio == 1 or abs(ratio - 1) > margin, (row, ratio)
        for midp in (False, True):
            exact = hc.hwe_p_exact(*row, midp)
            got = hc.hwe_p(*row, midp)
            # (mid-p of a one-table site is 1/2; nothing here is 0)
            assert exact > 0
            rel = abs(Fraction(got) - exact) / exact
            worst = max(worst, float(rel))
            assert rel <= Fraction(1, 10 ** 12), (row, midp, got, float(exact))
    print(f"worst relative error vs exact arithmetic: {worst:.3g}")


def test_p_is_a_probability_and_symmetric():
    rows = hc.all_tables()
    for midp in (False, True):
        p = hc.expected(midp)
        ok = ~np.isnan(p)
        assert (p[ok] >= 0).all() and (p[ok] <= 1).all()
    swapped = cuking_amd.hwe_sites_host(hc.counts_array([(c, b, a) for a, b, c in rows]), len(rows))
    assert hc.bits(swapped).tolist() == hc.bits(hc.expected(False)).tolist()


def test_filter_mask_arithmetic():
    p = np.array([1.0, 1e-6, 9.99e-7, 0.0, np.nan, 0.5, np.nextafter(1e-6, 0), 1e-6])
    keep = cuking_amd.hwe_site_mask(p, 1e-6)
    assert keep.tolist() == [True, True, False, False, False, True, False, True]
    also = np.array([1, 1, 1, 1, 1, 0, 1, 0], dtype=np.uint8)
    assert cuking_amd.hwe_site_mask(p, 1e-6, also).tolist() == \
        [True, True, False, False, False, False, False, False]
    assert also.tolist() == [1, 1, 1, 1, 1, 0, 1, 0]     # (the caller's array is left alone)
    # threshold 0 keeps everything but NaN, threshold 1 only p = 1
    assert cuking_amd.hwe_site_mask(p, 0.0).tolist() == [True] * 4 + [False] + [True] * 3
    assert cuking_amd.hwe_site_mask(p, 1.0).tolist() == [True] + [False] * 7
    # ... and the mask goes through the site rule as `also`: the rule on counts, ANDed
    rows = [(50, 40, 10), (90, 0, 10), (0, 0, 0), (30, 60, 10)] + [(10, 0, 0)] * 60
    counts = hc.counts_array(rows)
    counts[:, 3] = 0
    p = cuking_amd.hwe_sites_host(counts, 64)
    hwe = cuking_amd.hwe_site_mask(p, 1e-3)
    assert hwe[:4].tolist() == [True, False, True, True]  # (n = 0: p = 1, the RULE drops it)
    words, kept = cuking_amd.site_mask_host(counts, 64, also=hwe)
    want = hwe & (counts[:, :3].sum(axis=1) > 0)
    assert cuking_amd.site_mask_bool(words, 64).tolist() == want.tolist() and kept == want.sum()


def test_refusals():
    counts = hc.counts_array([(1, 2, 3)] * 4)
    with pytest.raises(ValueError, match="counts"):
        cuking_amd.hwe_sites_host(counts, 5)                      # too few rows
    with pytest.raises(ValueError, match="counts"):
        cuking_amd.hwe_sites_host(counts.astype(np.int64), 4)
    with pytest.raises(ValueError, match="counts"):
        cuking_amd.hwe_sites_host(counts[:, :3], 4)
    with pytest.raises(ValueError):
        cuking_amd.hwe_sites_host(counts, -1)
    assert cuking_amd.hwe_sites_host(counts, 0).shape == (0,)
    for bad in (-1e-9, 1.0000001, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="min_hwe_p"):
            cuking_amd.hwe_site_mask(np.ones(3), bad)
    with pytest.raises(ValueError, match="also"):
        cuking_amd.hwe_site_mask(np.ones(3), 0.5, also=np.ones(4, dtype=bool))
    # the C ABI: unknown flag bits and null pointers, with their messages
    lib = _lib.load()
    p = np.empty(4, dtype=np.float64)
    for flags in (2, 3, 0x80000000):
        assert lib.cuking_hwe_sites_host(counts.ctypes.data, 4, flags, p.ctypes.data) == 1
        assert b"unknown flags" in lib.cuking_last_error()
    assert lib.cuking_hwe_sites_host(None, 4, 0, p.ctypes.data) == 1
    assert b"null pointer" in lib.cuking_last_error()
    assert lib.cuking_hwe_sites_host(counts.ctypes.data, 4, 0, None) == 1
    assert lib.cuking_hwe_sites_host(None, 0, 0, None) == 0
    # the device form refuses a null context before anything else
    assert lib.cuking_hwe_sites(None, None, 0, 0, None, None) == 1
    assert b"null context" in lib.cuking_last_error()
    with pytest.raises(CukingError):
        check(lib.cuking_hwe_sites_host(None, 1, 0, None))


def test_abi_symbols_and_exports():
    lib = _lib.load()
    raw = C.CDLL(lib._name)     # (the symbols themselves, not the wrapper's table)
    for name in ("cuking_hwe_sites", "cuking_hwe_sites_host"):
        assert getattr(raw, name) is not None and name in _lib.SIGNATURES
    assert cuking_amd.HWE_MIDP == 1
    header = (ROOT / "include" / "cuking_amd.h").read_text()
    assert "#define CUKING_HWE_MIDP 1u" in header
    assert "cuking_hwe_sites_host(" in header and "cuking_hwe_sites(cuking_ctx" in header
    import inspect
    sig = inspect.signature(cuking_amd.KingContext.filter_sites)
    names = list(sig.parameters)
    assert names[-3:] == ["min_hwe_p", "hwe_midp", "hwe_counts"]
    assert sig.parameters["min_hwe_p"].default == 0.0
    assert sig.parameters["hwe_midp"].default is False
    assert sig.parameters["hwe_counts"].default is None
    assert callable(cuking_amd.KingContext.hwe_sites) and callable(cuking_amd.SiteQC.hwe_p)


def test_host_side_under_asan_ubsan(tmp_path):
    """csrc/king_host.cc and a stand-alone driver (tests/hwe_host_driver.cc) built with
    AddressSanitizer + UBSan, contraction off.  A program of its own on the CPU: nothing is loaded
    into Python.  It recomputes the fixed edge rows and the paper's; the test compares the bits."""
    rows = [r for r, _ in hc.EDGE_ROWS] + [r for r, _ in hc.WIGGINTON]
    text = "".join(f"{a} {b} {c}\n" for a, b, c in rows)
    done = run_sanitized_driver(tmp_path, "hwe_host_driver", stdin=text)
    lines = [l for l in done.stdout.splitlines() if l.startswith("row ")]
    assert len(lines) == len(rows)
    for row, line in zip(rows, lines):
        head, _, words = line.partition(": ")
        assert head == "row %d %d %d" % row
        direct, direct_mid, twin, twin_mid = (int(w, 16) for w in words.split())
        want = int(np.float64(hc.hwe_p(*row, False)).view(np.uint64))
        want_mid = int(np.float64(hc.hwe_p(*row, True)).view(np.uint64))
        assert (direct, twin) == (want, want), (row, hex(direct), hex(twin), hex(want))
        assert (direct_mid, twin_mid) == (want_mid, want_mid), (row, hex(direct_mid), hex(want_mid))
