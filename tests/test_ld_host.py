"""LD pruning, CPU side: the host transpose and the host edge list (the specifications in
executable form) against a known answer written out by hand and against the numpy restatement,
bit for bit; the kept set against the sequential greedy; the refusals; the driver's usage
errors.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from host_driver import compile_c99, run_sanitized_driver
from ld_cases import (GUARD, check_guarantees, greedy_numpy, ld_cohort, ld_edges_numpy,
                      priority_numpy, same_records, site_bits_numpy,
                      test_the_restatement_is_the_squared_correlation)  # noqa: F401 (collected)
from site_qc_cases import pack, site_counts_numpy

import cuking_amd
from cuking_amd import _lib


def host_edges(geno, window, r2, group=None):
    bits = pack(geno)
    n, m = geno.shape
    site_bits = cuking_amd.transpose_sites_host(bits, bits.shape[1], m)
    return cuking_amd.ld_edges_host(site_bits, m, n, window, r2, group=group)


def host_prune(geno, window, r2, group=None):
    """ld_prune put together from the host pieces: (keep bool [m], edges)."""
    n, m = geno.shape
    edges, _ = host_edges(geno, window, r2, group)
    counts = site_counts_numpy(geno, cuking_amd.words_per_sample(m) // 2)
    priority = cuking_amd.ld_priority_host(counts, m)
    keep, _ = cuking_amd.unrelated_set_host(edges, m, priority=priority, families=False)
    return keep == 1, edges


def test_known_answer_from_the_definition():
    """6 samples x 4 sites.  Sites 0 and 1 are identical where both are called; site 2 is
    their mirror image (2 - g); site 3 is monomorphic."""
    geno = np.array([[0, 1, 2, 0, 1, -1],
                     [0, 1, 2, 0, -1, 2],
                     [2, 1, 0, 2, 1, 0],
                     [0, 0, 0, 0, -1, 0]], dtype=np.int8).T      # [samples, sites]
    bits = pack(geno)
    site_bits = cuking_amd.transpose_sites_host(bits, bits.shape[1], 4)
    tail = 0xFFFFFFFFFFFFFFC0
    # (het, hom_var) words: bit s of het = het or missing, of hom_var = hom-var or missing
    want = np.array([[tail | 0b110010, tail | 0b100100],
                     [tail | 0b010010, tail | 0b110100],
                     [tail | 0b010010, tail | 0b001001],
                     [tail | 0b010000, tail | 0b010000]], dtype=np.uint64).reshape(4, 2, 1)
    assert np.array_equal(site_bits, want)
    # pair (0, 1): called at both = samples 0 .. 3, g = (0, 1, 2, 0) twice: n = 4, Sx = Sy = 3,
    # Sxx = Syy = Sxy = 5: cov = vx = vy = 20 - 9 = 11, r^2 = 1
    # pair (0, 2): samples 0 .. 4, x = (0, 1, 2, 0, 1), y = (2, 1, 0, 2, 1): n = 5, Sx = 4,
    # Sy = 6, Sxx = 6, Syy = 10, Sxy = 2: cov = 10 - 24 = -14, vx = 30 - 16 = 14, vy = 50 - 36 = 14
    # pair (1, 2): samples 0 .. 3 and 5, x = (0, 1, 2, 0, 2), y = (2, 1, 0, 2, 0): n = 5, Sx = 5,
    # Sy = 5, Sxx = 9, Syy = 9, Sxy = 1: cov = 5 - 25 = -20, vx = vy = 45 - 25 = 20
    recs, count = cuking_amd.ld_edges_host(site_bits, 4, 6, window=4, r2=0.5)
    assert count == 3
    assert [tuple(r) for r in recs] == [(0, 1, 1.0, 4, 0, 0), (0, 2, 1.0, 5, 0, 0),
                                        (1, 2, 1.0, 5, 0, 0)]
    assert cuking_amd.ld_edges_host(site_bits, 4, 6, window=2, r2=0.5)[0]["sample_j"].tolist() == [1, 2]
    assert cuking_amd.ld_edges_host(site_bits, 4, 6, window=4, r2=1.0)[1] == 0
    # priorities: minor / (2 called) = 4/10, 5/10, 6/12 -> 0.5, 0/10; NaN for no call
    counts = site_counts_numpy(geno, 1)
    prio = cuking_amd.ld_priority_host(counts, 4)
    assert prio.tolist() == [np.float32(0.4), 0.5, 0.5, 0.0]
    assert np.isnan(_lib.load().cuking_ld_priority((C.c_uint32 * 4)(0, 0, 0, 9)))
    # sites 1 and 2 tie at 0.5: the lower index stays, 0 and 2 go, the monomorphic site stays
    keep, _ = host_prune(geno, 4, 0.5)
    assert keep.tolist() == [False, True, False, True]


@pytest.mark.parametrize("n", (1, 63, 64, 65, 130))
def test_transpose_against_numpy(n):
    rng = np.random.default_rng(6000 + n)
    for m in (1, 64, 65, 700):
        geno = ld_cohort(int(rng.integers(1 << 30)), n, m)
        bits = pack(geno)
        q = cuking_amd.ld_site_words(n)
        assert q == (n + 63) // 64
        whole = np.full((m + 2, 2, q), GUARD, dtype=np.uint64)
        out = cuking_amd.transpose_sites_host(bits, bits.shape[1], m, out=whole[1:m + 1])
        assert np.array_equal(out, site_bits_numpy(geno)), (n, m)
        assert (whole[0] == GUARD).all() and (whole[-1] == GUARD).all()
        if n % 64:  # the tail of the last word reads as missing
            assert (out[:, :, -1] >> np.uint64(n % 64) == np.uint64((1 << (64 - n % 64)) - 1)).all()


@pytest.fixture(scope="module")
def cohort():
    geno = ld_cohort(5, 130, 333)
    group = (np.arange(333) >= 100).astype(np.int32) + (np.arange(333) >= 131)   # cuts inside windows
    return geno, group


@pytest.mark.parametrize("window", (2, 7, 64, 65, 343))
def test_edges_bit_equal_to_the_restatement(cohort, window):
    geno, group = cohort
    for r2 in (0.0, 0.2, 0.999, 1.0):
        for g in (None, group):
            got, count = host_edges(geno, window, r2, g)
            want = ld_edges_numpy(geno, window, r2, g)
            assert count == len(want) and same_records(got, want), (window, r2, g is None)
            if g is not None and len(got):
                assert (group[got["sample_i"]] == group[got["sample_j"]]).all()
            if r2 == 1.0:
                assert count == 0           # although sites 7 and 9 are identical
            if r2 == 0.999 and window >= 3 and g is None:
                assert (7, 9) in set(zip(got["sample_i"].tolist(), got["sample_j"].tolist()))
    assert len(host_edges(geno, 50, 0.2)[0]) > 300


def test_kept_set_is_the_greedy_and_keeps_its_promises(cohort):
    geno, group = cohort
    for window, r2, g in ((50, 0.2, None), (50, 0.2, group), (7, 0.0, None), (343, 0.5, None)):
        keep, edges = host_prune(geno, window, r2, g)
        want_edges = ld_edges_numpy(geno, window, r2, g)
        assert np.array_equal(keep, greedy_numpy(want_edges, priority_numpy(geno)))
        check_guarantees(keep, want_edges)
        assert keep[333 // 2] and keep[333 // 3]    # monomorphic, all missing: no edges
    assert np.array_equal(cuking_amd.ld_priority_host(
        site_counts_numpy(geno, cuking_amd.words_per_sample(333) // 2), 333).view(np.uint32),
        priority_numpy(geno).view(np.uint32))


def test_allele_swap_changes_nothing(cohort):
    geno, _ = cohort
    keep, edges = host_prune(geno, 50, 0.2)
    swapped = geno.copy()
    flip = np.random.default_rng(9).random(333) < 0.5
    swapped[:, flip] = np.where(geno[:, flip] >= 0, 2 - geno[:, flip], -1)
    keep2, edges2 = host_prune(swapped, 50, 0.2)
    assert same_records(edges, edges2) and np.array_equal(keep, keep2)


def test_overflow_reports_the_exact_count(cohort):
    geno, _ = cohort
    bits = pack(geno)
    site_bits = cuking_amd.transpose_sites_host(bits, bits.shape[1], 333)
    full, count = cuking_amd.ld_edges_host(site_bits, 333, 130, 50, 0.2)
    room = 100
    assert count > room
    whole = np.zeros(room + 4, dtype=cuking_amd.KING_RESULT_DTYPE)
    whole.view(np.uint8)[:] = 0xA5
    got = C.c_uint64(0)
    status = _lib.load().cuking_ld_edges_host(site_bits.ctypes.data, 333, 130, 50, 0.2, None,
                                              whole.ctypes.data, room, C.byref(got))
    assert status == _lib.ERR_RESOURCE_EXHAUSTED == 3 and got.value == count
    assert (whole[room:].view(np.uint8) == 0xA5).all()
    assert same_records(cuking_amd.sort_results(whole[:room].copy()), full[:room])  # host order
    with pytest.raises(cuking_amd.ResourceExhaustedError) as e:
        cuking_amd.ld_edges_host(site_bits, 333, 130, 50, 0.2, max_records=room)
    assert e.value.num_records == count
    # the default buffer (4 x sites) overflows at window 343, r^2 0: the wrapper retries
    many, total = cuking_amd.ld_edges_host(site_bits, 333, 130, 343, 0.0)
    assert total == len(many) > 4 * 333


def test_refused_arguments():
    lib = _lib.load()
    n, m = 70, 129
    geno = ld_cohort(3, n, m)
    bits = pack(geno)
    wps, q = bits.shape[1], 2
    site_bits = np.zeros((m, 2, q), dtype=np.uint64)

    def transpose(in_=bits.ctypes.data, rows=n, wps_=wps, sites=m, out_=site_bits.ctypes.data, q_=q):
        return lib.cuking_transpose_sites_host(in_, rows, wps_, sites, out_, q_)
    assert transpose() == _lib.OK
    for what, kw in {"null input": dict(in_=None), "null output": dict(out_=None),
                     "words_per_sample of another site count": dict(sites=300),
                     "words_per_site_plane too small": dict(q_=1),
                     "words_per_site_plane too large": dict(q_=3),
                     "more than 2^24 samples": dict(rows=(1 << 24) + 1, q_=(1 << 18) + 1)}.items():
        assert transpose(**kw) == _lib.ERR_INVALID_ARGUMENT, what
        assert lib.cuking_last_error() != b"", what
    recs = np.zeros(8, dtype=cuking_amd.KING_RESULT_DTYPE)
    count = C.c_uint64(7)

    def edges(bits_=site_bits.ctypes.data, rows=n, window=50, r2=0.2, recs_=recs.ctypes.data,
              room=8, count_=C.byref(count)):
        return lib.cuking_ld_edges_host(bits_, m, rows, window, r2, None, recs_, room, count_)
    assert edges(r2=1.0) == _lib.OK and count.value == 0
    assert edges(recs_=None, room=0, r2=1.0) == _lib.OK
    for what, kw in {"null site bits": dict(bits_=None), "null count": dict(count_=None),
                     "null records": dict(recs_=None),
                     "more than 2^24 samples": dict(rows=(1 << 24) + 1),
                     "window 0": dict(window=0), "window 1": dict(window=1),
                     "threshold NaN": dict(r2=float("nan")), "threshold above 1": dict(r2=1.5),
                     "threshold below 0": dict(r2=-0.1)}.items():
        assert edges(**kw) == _lib.ERR_INVALID_ARGUMENT, what
        assert lib.cuking_last_error() != b"", what
    # the device entry points check their arguments before they touch a device
    assert lib.cuking_transpose_sites(None, bits.ctypes.data, n, wps, m, site_bits.ctypes.data, q,
                                      None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.cuking_ld_edges(None, site_bits.ctypes.data, m, n, 50, 0.2, None, recs.ctypes.data,
                               8, C.byref(count), None) == _lib.ERR_INVALID_ARGUMENT
    # ... and the Python functions
    with pytest.raises(ValueError, match="window"):
        cuking_amd.ld_edges_host(site_bits, m, n, window=1)
    with pytest.raises(ValueError, match="r2"):
        cuking_amd.ld_edges_host(site_bits, m, n, r2=float("nan"))
    with pytest.raises(ValueError, match="group"):
        cuking_amd.ld_edges_host(site_bits, m, n, group=np.zeros(5, dtype=np.int32))


def test_bim_chromosomes(tmp_path):
    from cuking_amd import plink
    geno = ld_cohort(1, 5, 7)
    plink.write_plink(tmp_path / "c", geno, chromosomes=["2", "2", "X", "1", "X", "2", "1"])
    group = plink.read_bim_chromosomes(tmp_path / "c")
    assert group.dtype == np.int32 and group.tolist() == [0, 0, 1, 2, 1, 0, 2]
    plink.write_plink(tmp_path / "d", geno)
    assert plink.read_bim_chromosomes(tmp_path / "d").tolist() == [0] * 7


def test_driver_usage_errors_need_no_gpu(tmp_path, capsys, monkeypatch):
    from cuking_amd import run
    base = ["--synthetic", "8,9", "--output-uri", str(tmp_path / "out")]
    flags = (["--site-ld-window", "50"], ["--site_ld_r2", "0.2"], ["--site-ld-uri", "ld.npz"])
    for flag in flags:
        assert run.main(base + flag + ["--split-factor", "2"]) == 1
        err = capsys.readouterr().err
        assert "Error: INVALID_ARGUMENT" in err and "--split_factor 1" in err, err
    monkeypatch.setenv("WORLD_SIZE", "2")
    for flag in flags:
        assert run.main(base + flag) == 1
        err = capsys.readouterr().err
        assert "Error: INVALID_ARGUMENT" in err and "one process" in err, err
    monkeypatch.delenv("WORLD_SIZE")
    for flag, name in ((["--site-ld-r2", "1.5"], "site_ld_r2"), (["--site-ld-r2=-0.1"], "site_ld_r2"),
                       (["--site-ld-r2", "nan"], "site_ld_r2"),
                       (["--site-ld-window", "1"], "site_ld_window"),
                       (["--site-ld-window=-3"], "site_ld_window")):
        assert run.main(base + flag) == 1
        err = capsys.readouterr().err
        assert "Error: INVALID_ARGUMENT" in err and name in err, err
    with pytest.raises(SystemExit):
        run.parse_args(["--help"])
    text = capsys.readouterr().out
    for name in ("site-ld-window", "site_ld_r2", "site-ld-uri"):
        assert f"--{name}" in text, name


def test_header_is_still_plain_c(tmp_path):
    compile_c99(tmp_path, """
#include "cuking_amd.h"
typedef char abi_is_2[CUKING_ABI_VERSION == 2 ? 1 : -1];
int use(const uint64_t *bits, uint64_t *site_bits, const int32_t *group, cuking_result *records) {
  uint64_t count = 0;
  const uint32_t counts[4] = {3, 2, 1, 0};
  cuking_status (*transpose)(cuking_ctx *, const uint64_t *, uint32_t, uint32_t, uint32_t,
                             uint64_t *, uint32_t, void *) = cuking_transpose_sites;
  cuking_status (*edges)(cuking_ctx *, const uint64_t *, uint32_t, uint32_t, uint32_t, float,
                         const int32_t *, cuking_result *, uint64_t, uint64_t *, void *) =
      cuking_ld_edges;
  (void)transpose; (void)edges;
  if (cuking_ld_priority(counts) < 0.0f) return 1;
  if (cuking_transpose_sites_host(bits, 70, cuking_words_per_sample(100), 100, site_bits,
                                  cuking_ld_site_words(70)) != CUKING_OK) return 1;
  return (int)cuking_ld_edges_host(site_bits, 100, 70, 50, 0.2f, group, records, 16, &count);
}
""")
    assert _lib.load().cuking_abi_version() == 2


def test_host_side_under_asan_ubsan(tmp_path):
    """csrc/king_host.cc and a stand-alone driver (tests/ld_host_driver.cc: exact-size heap
    buffers; the host transpose and edge list against the definition on plain genotype arrays,
    the helpers of csrc/king_ld.h) built with AddressSanitizer + UBSan.  A program of its own
    on the CPU: nothing is loaded into Python."""
    run_sanitized_driver(tmp_path, "ld_host_driver")
