"""Site QC, CPU side: the site rule and the host compaction (the specifications in executable
form) against the definition written out by hand, against numpy restatements and against
cuking_pack_host of the kept genotypes; the refusals; the driver's usage errors.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from conftest import random_genotypes
from host_driver import compile_c99, run_sanitized_driver
from site_qc_cases import GUARD, SAMPLES, SITES, masks, pack, rule_numpy, site_counts_numpy

import cuking_amd
from cuking_amd import _lib


def test_known_answer_from_the_definition():
    """The 6 x 3 genotypes of test_bed_host.py::test_known_answer_from_the_definition."""
    geno = np.array([[2, 0, -1, 0, 0, 0],
                     [0, -1, 1, 0, 0, 0],
                     [0, 1, 1, -1, -1, 2]], dtype=np.int8).T     # [samples, sites]
    # (hom_ref, het, hom_var, missing) of the three sites; the 61 padding sites are missing
    counts = np.zeros((64, 4), dtype=np.uint32)
    counts[:, 3] = 6
    counts[:3] = [[4, 0, 1, 1], [4, 1, 0, 1], [1, 2, 1, 2]]
    assert np.array_equal(counts, site_counts_numpy(geno, 1))
    # call rates 5/6, 5/6, 4/6; minor allele counts 2, 1, 4 (alt 4 of 8 at the last site)
    keep, kept = cuking_amd.site_mask_host(counts, 3)
    assert (keep.tolist(), kept) == ([0b111], 3)
    keep, kept = cuking_amd.site_mask_host(counts, 3, min_call_rate=0.7, min_mac=1)
    assert (keep.tolist(), kept) == ([0b011], 2)
    assert cuking_amd.site_mask_host(counts, 3, min_mac=2)[0].tolist() == [0b101]
    assert cuking_amd.site_mask_host(counts, 3, min_maf=0.15)[0].tolist() == [0b101]  # 2/10, 1/10, 4/8
    assert cuking_amd.site_mask_host(counts, 3, min_maf=0.5)[0].tolist() == [0b100]
    # sites 0 and 1 of every sample, bits 2.. missing: (het, hom_var) words
    bits = pack(geno)
    whole = np.full((8, 2), GUARD, dtype=np.uint64)
    out, wps, kept = cuking_amd.compact_sites_host(bits, 2, np.array([0b011], dtype=np.uint64), 3,
                                                   out=whole[1:7])
    base = 0xFFFFFFFFFFFFFFFC
    want = np.array([[base, base | 1],        # hom-var, hom-ref
                     [base | 2, base | 2],    # hom-ref, missing
                     [base | 3, base | 1],    # missing, het
                     [base, base], [base, base], [base, base]], dtype=np.uint64)
    assert (wps, kept) == (2, 2) and np.array_equal(out, want)
    assert np.array_equal(want, pack(geno[:, :2]))
    assert (whole[0] == GUARD).all() and (whole[-1] == GUARD).all()


def test_site_mask_against_the_rule_restated():
    rng = np.random.default_rng(42)
    m = 700
    plane = cuking_amd.words_per_sample(m) // 2
    counts = rng.integers(0, 40, size=(plane * 64, 4), dtype=np.uint32)
    counts[rng.random(plane * 64) < 0.1, :3] = 0           # called = 0
    counts[rng.random(plane * 64) < 0.1, 3] = 0            # nothing missing
    counts[rng.random(plane * 64) < 0.1, 1:3] = 0          # monomorphic
    # boundaries: minor exactly at min_maf * 2 called for 0.25 (exact) -- kept at 4 of 16, not
    # at 3 --, and for 0.1, whose float32 value is ABOVE 1/10: 1 of 10 does not pass
    counts[0] = [4, 4, 0, 0]
    counts[1] = [5, 3, 0, 0]
    counts[2] = [4, 1, 0, 7]
    counts[3] = [0, 0, 0, 9]
    also = rng.random(m) < 0.7
    for rate in (0.0, 0.5, 0.95, 1.0):
        for maf in (0.0, 0.1, 0.25, 0.5, 0.6):
            for mac in (0, 1, 5):
                for extra in (None, also):
                    keep, kept = cuking_amd.site_mask_host(counts, m, rate, maf, mac, also=extra)
                    want = rule_numpy(counts, m, rate, maf, mac, extra)
                    got = cuking_amd.site_mask_bool(keep, m)
                    assert np.array_equal(got, want), (rate, maf, mac)
                    assert kept == int(want.sum())
                    # padding sites are never kept
                    assert not cuking_amd.site_mask_bool(keep, plane * 64)[m:].any()
                    if maf == 0.6:
                        assert kept == 0
    at = lambda **kw: cuking_amd.site_mask_bool(cuking_amd.site_mask_host(counts, m, **kw)[0], m)
    assert at(min_maf=0.25)[0] and not at(min_maf=0.25)[1]
    assert at(min_maf=0.0)[2] and not at(min_maf=0.1)[2]
    assert not at()[3]
    # the defaults keep every site with one called genotype
    assert np.array_equal(at(), counts[:m, :3].sum(axis=1) > 0)


@pytest.mark.parametrize("n", SAMPLES)
def test_compaction_byte_for_byte_with_pack_host(n):
    rng = np.random.default_rng(3000 + n)
    for m in SITES:
        geno = random_genotypes(rng, n, m, missing=0.1)
        bits = pack(geno)
        for name, keep in masks(rng, m).items():
            kept = int(keep.sum())
            wps_out = cuking_amd.words_per_sample(kept)
            whole = np.full((n + 2, wps_out), GUARD, dtype=np.uint64)
            out, wps, k = cuking_amd.compact_sites_host(
                bits, bits.shape[1], cuking_amd.site_mask_words(keep), m, out=whole[1:n + 1])
            assert (wps, k) == (wps_out, kept), (n, m, name)
            assert np.array_equal(out, pack(geno[:, keep])), (n, m, name)
            assert (whole[0] == GUARD).all() and (whole[-1] == GUARD).all(), (n, m, name)


def test_refused_arguments():
    lib = _lib.load()
    m = 129
    wps = cuking_amd.words_per_sample(m)
    plane = wps // 2
    bits = pack(random_genotypes(np.random.default_rng(1), 5, m))
    keep = np.zeros(plane, dtype=np.uint64)
    keep[0] = 0xFF
    out = np.zeros((5, 2), dtype=np.uint64)

    def compact(in_=bits.ctypes.data, rows=5, wps_in=wps, keep_=keep, sites=m,
                out_=out.ctypes.data, wps_out=2):
        status = lib.cuking_compact_sites_host(
            in_, rows, wps_in, keep_.ctypes.data if keep_ is not None else None, sites, out_,
            wps_out)
        return status, lib.cuking_last_error().decode()
    assert compact()[0] == _lib.OK
    none = np.zeros(plane, dtype=np.uint64)
    status, message = compact(keep_=none)
    assert status == _lib.ERR_INVALID_ARGUMENT and "no site passes" in message
    beyond = keep.copy()
    beyond[2] = 2                                   # site 129 of 129
    padding = keep.copy()
    padding[2] = 1 << 40
    refused = {
        "null input": dict(in_=None), "null mask": dict(keep_=None), "null output": dict(out_=None),
        "wrong words_per_sample_out": dict(wps_out=4),
        "odd words_per_sample_out": dict(wps_out=3),
        "words_per_sample_in of another site count": dict(sites=300),
        "a keep bit at num_sites": dict(keep_=beyond),
        "a keep bit in the padding": dict(keep_=padding),
        "in place": dict(out_=bits.ctypes.data),
        "overlapping": dict(out_=bits.ctypes.data + 8 * wps),
    }
    for what, kw in refused.items():
        status, message = compact(**kw)
        assert status == _lib.ERR_INVALID_ARGUMENT and message, what
    assert "129" in compact(keep_=beyond)[1]
    assert compact(rows=0)[0] == _lib.OK
    # ... and through the Python function
    with pytest.raises(cuking_amd.CukingError, match="no site passes") as e:
        cuking_amd.compact_sites_host(bits, wps, none, m)
    assert e.value.status == _lib.ERR_INVALID_ARGUMENT

    counts = np.zeros((plane * 64, 4), dtype=np.uint32)

    def mask(counts_=counts.ctypes.data, sites=m, plane_=plane, rule=(0.0, 0.0, 0), rule_null=False,
             keep_=keep.ctypes.data):
        f = _lib.CSiteFilter(*rule)
        return lib.cuking_site_mask_host(counts_, sites, plane_, None if rule_null else C.byref(f),
                                         None, keep_, None)
    assert mask() == _lib.OK
    for what, kw in {"null counts": dict(counts_=None), "null rule": dict(rule_null=True),
                     "null keep": dict(keep_=None), "plane_words": dict(plane_=plane + 1),
                     "plane_words of fewer sites": dict(sites=64),
                     "call rate above 1": dict(rule=(1.5, 0.0, 0)),
                     "call rate below 0": dict(rule=(-0.1, 0.0, 0)),
                     "call rate NaN": dict(rule=(float("nan"), 0.0, 0)),
                     "maf above 1": dict(rule=(0.0, 1.01, 0)),
                     "maf below 0": dict(rule=(0.0, -1.0, 0)),
                     "maf NaN": dict(rule=(0.0, float("nan"), 0))}.items():
        assert mask(**kw) == _lib.ERR_INVALID_ARGUMENT, what
        assert lib.cuking_last_error() != b"", what
    assert mask(rule=(1.0, 0.6, 7)) == _lib.OK      # min_maf above 0.5 is legal
    # device entry points check their arguments before they touch a device
    for call in (lambda: lib.cuking_site_counts(None, 1, 1, 2, 1, None),
                 lambda: lib.cuking_sample_counts(None, 1, 1, 2, 1, 1, None),
                 lambda: lib.cuking_compact_sites(None, bits.ctypes.data, 5, wps,
                                                  keep.ctypes.data, m, out.ctypes.data, 2, None)):
        assert call() == _lib.ERR_INVALID_ARGUMENT


def test_driver_usage_errors_need_no_gpu(tmp_path, capsys, monkeypatch):
    from cuking_amd import run
    base = ["--synthetic", "8,9", "--output-uri", str(tmp_path / "out")]
    flags = (["--site-min-call-rate", "0.9"], ["--site_min_maf", "0.01"], ["--site-min-mac", "1"],
             ["--site-keep-uri", "k.npy"], ["--site_qc_uri", "q.npz"])
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
    for flag in (["--site-min-call-rate", "1.5"], ["--site-min-maf=-0.1"], ["--site-min-maf", "nan"],
                 ["--site-min-mac=-1"]):
        assert run.main(base + flag) == 1
        err = capsys.readouterr().err
        assert "Error: INVALID_ARGUMENT" in err and flag[0][2:10].replace("-", "_") in err, err
    with pytest.raises(SystemExit):
        run.parse_args(["--help"])
    text = capsys.readouterr().out
    for name in ("site-min-call-rate", "site_min_maf", "site-min-mac", "site_keep_uri",
                 "site-qc-uri"):
        assert f"--{name}" in text, name


def test_header_is_still_plain_c(tmp_path):
    compile_c99(tmp_path, """
#include "cuking_amd.h"
typedef char abi_is_2[CUKING_ABI_VERSION == 2 ? 1 : -1];
int use(const uint32_t *counts, const uint64_t *in, uint64_t *keep, uint64_t *out) {
  cuking_site_filter rule = {0.95f, 0.01f, 1};
  uint32_t kept = 0;
  cuking_status (*site)(cuking_ctx *, const uint64_t *, uint32_t, uint32_t, uint32_t *, void *) =
      cuking_site_counts;
  cuking_status (*sample)(cuking_ctx *, const uint64_t *, uint32_t, uint32_t, uint32_t,
                          uint32_t *, void *) = cuking_sample_counts;
  cuking_status (*device)(cuking_ctx *, const uint64_t *, uint32_t, uint32_t, const uint64_t *,
                          uint32_t, uint64_t *, uint32_t, void *) = cuking_compact_sites;
  (void)site; (void)sample; (void)device;
  if (cuking_site_mask_host(counts, 100, cuking_words_per_sample(100) / 2, &rule, 0, keep,
                            &kept) != CUKING_OK) return 1;
  return (int)cuking_compact_sites_host(in, 4, cuking_words_per_sample(100), keep, 100, out,
                                        cuking_words_per_sample(kept));
}
""")
    assert _lib.load().cuking_abi_version() == 2


def test_host_side_under_asan_ubsan(tmp_path):
    """csrc/king_host.cc and a stand-alone driver (tests/site_qc_host_driver.cc: exact-size heap
    buffers; the host compaction against the definition, the compaction kernel's table walk and
    the count kernel's bit-sliced counters from csrc/king_site_qc.h run on the host, the site
    rule) built with AddressSanitizer + UBSan.  A program of its own on the CPU: nothing is
    loaded into Python."""
    run_sanitized_driver(tmp_path, "site_qc_host_driver")
