"""PLINK .bed input, CPU side: the host pack (the specification in executable form) against
the format's definition and against cuking_pack_host, the file reader / writer, the argument
checks, and the driver's usage errors.  No GPU."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from conftest import random_genotypes
from host_driver import compile_c99, run_sanitized_driver

import cuking_amd
from cuking_amd import _lib, plink

ROOT = Path(__file__).resolve().parent.parent
GUARD = np.uint64(0xA5A5A5A5A5A5A5A5)

SAMPLES = (1, 3, 4, 5, 13, 37, 64, 65, 130)
SITES = (1, 31, 32, 33, 63, 64, 65, 129, 700)


def triples(geno):
    """(row_idx = site, col_idx = sample, n_alt) of every non-missing genotype, site-major."""
    site, sample = np.nonzero(geno.T >= 0)
    return site.astype(np.int64), sample.astype(np.int64), geno.T[site, sample].astype(np.int32)


def expected_bitset(sm, geno):
    bits = cuking_amd.new_host_bitset(sm, geno.shape[1])
    cuking_amd.pack_host(sm, bits, *triples(geno))
    return bits


def guarded(sm, num_sites):
    """The block's bitset prefilled with 0xA5, a guard row on either side: (whole, view)."""
    whole = np.full((sm.NumSamples() + 2, cuking_amd.words_per_sample(num_sites)), GUARD,
                    dtype=np.uint64)
    return whole, whole[1:sm.NumSamples() + 1]


def blocks(n):
    out = [cuking_amd.Submatrix(n)]
    if n == 37:  # sample ranges that start at 13 and 26, and the off-diagonal blocks
        out += [cuking_amd.Submatrix(37, 3, k) for k in range(6)]
    return out


def test_known_answer_from_the_definition(tmp_path):
    prefix = tmp_path / "six"
    Path(str(prefix) + ".bed").write_bytes(bytes.fromhex("6c1b01" "dc0f" "e70f" "6b01"))
    Path(str(prefix) + ".fam").write_text("".join(f"f{k} i{k} 0 0 0 -9\n" for k in range(6)))
    Path(str(prefix) + ".bim").write_text("".join(f"1\tv{k}\t0\t{k + 1}\tA\tC\n" for k in range(3)))
    geno = np.array([[2, 0, -1, 0, 0, 0],
                     [0, -1, 1, 0, 0, 0],
                     [0, 1, 1, -1, -1, 2]], dtype=np.int8).T     # [samples, sites]
    with plink.open_bed(prefix) as bed:
        assert (bed.num_samples, bed.num_sites, bed.row_bytes) == (6, 3, 2)
        assert bed.sample_ids == [f"i{k}" for k in range(6)]
        rows = bed.read_rows(0, 3, np.zeros(6, dtype=np.uint8))
    assert rows.tobytes() == bytes.fromhex("dc0fe70f6b01")
    sm = cuking_amd.Submatrix(6)
    whole, bits = guarded(sm, 3)
    cuking_amd.pack_bed_host(sm, bits, rows, 2, 0, 3, 3)
    assert np.array_equal(bits, expected_bitset(sm, geno))
    assert (whole[0] == GUARD).all() and (whole[-1] == GUARD).all()
    # ... and the writer produces exactly that file from those genotypes
    plink.write_plink(tmp_path / "again", geno)
    assert Path(str(tmp_path / "again") + ".bed").read_bytes() == bytes.fromhex(
        "6c1b01dc0fe70f6b01")


@pytest.mark.parametrize("n", SAMPLES)
def test_byte_for_byte_with_pack_host(tmp_path, n):
    rng = np.random.default_rng(1000 + n)
    for m in SITES:
        geno = random_genotypes(rng, n, m, missing=0.1)
        prefix = tmp_path / f"g{m}"
        plink.write_plink(prefix, geno)
        with plink.open_bed(prefix) as bed:
            assert (bed.num_samples, bed.num_sites) == (n, m)
            rows = bed.read_rows(0, m, np.empty(m * bed.row_bytes, dtype=np.uint8))
            row_bytes = bed.row_bytes
        for sm in blocks(n):
            whole, bits = guarded(sm, m)
            cuking_amd.pack_bed_host(sm, bits, rows, row_bytes, 0, m, m)
            assert np.array_equal(bits, expected_bitset(sm, geno)), (n, m, sm)
            assert (whole[0] == GUARD).all() and (whole[-1] == GUARD).all(), (n, m, sm)


def test_chunked_calls_equal_one_call():
    n, m = 37, 700
    geno = random_genotypes(np.random.default_rng(7), n, m, missing=0.1)
    rows = plink.encode_rows(geno)
    row_bytes = rows.shape[1]
    for sm in blocks(n):
        _, one = guarded(sm, m)
        cuking_amd.pack_bed_host(sm, one, rows, row_bytes, 0, m, m)
        whole, bits = guarded(sm, m)
        for begin, end in ((64, 192), (192, m), (0, 64)):   # (any order: disjoint words)
            # a copy of exactly the chunk's rows: nothing outside them is needed
            cuking_amd.pack_bed_host(sm, bits, rows[begin:end].copy(), row_bytes, begin, end, m)
        assert np.array_equal(bits, one) and np.array_equal(one, expected_bitset(sm, geno))
        assert (whole[0] == GUARD).all() and (whole[-1] == GUARD).all()
        # a chunk leaves the words outside its range alone
        _, part = guarded(sm, m)
        cuking_amd.pack_bed_host(sm, part, rows[64:192].copy(), row_bytes, 64, 192, m)
        wps = part.shape[1]
        touched = np.zeros(wps, dtype=bool)
        touched[1:3] = touched[wps // 2 + 1:wps // 2 + 3] = True
        assert (part[:, ~touched] == GUARD).all() and np.array_equal(part[:, touched],
                                                                     one[:, touched])


def test_refused_arguments():
    lib = _lib.load()
    n, m = 37, 700
    sm = cuking_amd.Submatrix(37, 3, 1)
    wps = cuking_amd.words_per_sample(m)
    bits = np.zeros((sm.NumSamples(), wps), dtype=np.uint64)
    rows = np.zeros(m * 10, dtype=np.uint8)

    def call(sm_=sm, wps_=wps, bits_=bits.ctypes.data, rows_=rows.ctypes.data, row_bytes=10,
             begin=0, end=m, sites=m):
        return lib.cuking_pack_bed_host(C.byref(sm_.c) if sm_ is not None else None, wps_, bits_,
                                        rows_, row_bytes, begin, end, sites)
    assert call() == _lib.OK
    refused = {
        "null submatrix": dict(sm_=None),
        "null bitset": dict(bits_=None),
        "null rows": dict(rows_=None),
        "site_begin not a multiple of 64": dict(begin=32),
        "site_end neither a multiple of 64 nor num_sites": dict(end=100),
        "site_begin > site_end": dict(begin=128, end=64),
        "site_end > num_sites": dict(end=704),
        "words_per_sample of another site count": dict(wps_=wps + 2),
        "rows too short for the block": dict(row_bytes=6),    # 24 samples, the block ends at 26
        "rows of no bytes": dict(row_bytes=0),
    }
    for what, kw in refused.items():
        assert call(**kw) == _lib.ERR_INVALID_ARGUMENT, what
        assert lib.cuking_last_error() != b"", what
    assert call(row_bytes=7) == _lib.OK                      # 28 samples >= 26
    # nothing to do: an empty site range, an empty block
    before = bits.copy()
    assert call(begin=64, end=64) == _lib.OK
    empty = cuking_amd.Submatrix.from_ranges(5, 5, 5, 5)
    assert call(sm_=empty) == _lib.OK
    assert np.array_equal(bits, before)


def test_bed_check_messages():
    lib = _lib.load()
    assert lib.cuking_bed_row_bytes(0) == 0 and lib.cuking_bed_row_bytes(1) == 1
    assert lib.cuking_bed_row_bytes(4) == 1 and lib.cuking_bed_row_bytes(5) == 2
    assert lib.cuking_bed_row_bytes(0xFFFFFFFF) == 1 << 30

    def check(magic, size, n=37, m=129):
        status = lib.cuking_bed_check((C.c_uint8 * 3)(*magic), size, n, m)
        return status, lib.cuking_last_error().decode()
    good = 3 + 129 * 10
    assert check((0x6C, 0x1B, 0x01), good)[0] == _lib.OK
    messages = {}
    for what, (magic, size) in {"magic": ((0x6C, 0x1A, 0x01), good),
                                "sample-major": ((0x6C, 0x1B, 0x00), good),
                                "short": ((0x6C, 0x1B, 0x01), good - 1),
                                "long": ((0x6C, 0x1B, 0x01), good + 1)}.items():
        status, messages[what] = check(magic, size)
        assert status != _lib.OK, what
    assert "not a PLINK .bed" in messages["magic"]
    assert "sample-major" in messages["sample-major"] and "not supported" in messages["sample-major"]
    for what, size in (("short", good - 1), ("long", good + 1)):
        assert str(size) in messages[what] and str(good) in messages[what], messages[what]
    assert len(set(messages.values())) == 4
    assert check((0x00, 0x1B, 0x01), good)[0] != _lib.OK
    assert lib.cuking_bed_check(None, good, 37, 129) == _lib.ERR_INVALID_ARGUMENT


def test_open_bed_reports_a_bad_file(tmp_path):
    geno = random_genotypes(np.random.default_rng(3), 9, 70)
    prefix = tmp_path / "c"
    plink.write_plink(prefix, geno, sample_ids=[f"id{k}" for k in range(9)])
    bed_path = Path(str(prefix) + ".bed")
    data = bed_path.read_bytes()
    with plink.open_bed(prefix) as bed:
        assert bed.sample_ids == [f"id{k}" for k in range(9)]
        with pytest.raises(ValueError):
            bed.read_rows(0, 71, np.zeros(71 * 3, dtype=np.uint8))
        with pytest.raises(ValueError):
            bed.read_rows(0, 70, np.zeros(70 * 3 - 1, dtype=np.uint8))
        # a chunk from the middle of the file
        assert bed.read_rows(64, 70, np.zeros(18, dtype=np.uint8)).tobytes() == \
            data[3 + 64 * 3:]
    bed_path.write_bytes(data[:-1])
    with pytest.raises(cuking_amd.CukingError, match=f"{len(data) - 1} bytes.*{len(data)}"):
        plink.open_bed(prefix)
    bed_path.write_bytes(b"\x6c\x1b\x00" + data[3:])
    with pytest.raises(cuking_amd.CukingError, match="sample-major"):
        plink.open_bed(prefix)
    bed_path.write_bytes(b"PK\x01" + data[3:])
    with pytest.raises(cuking_amd.CukingError, match="not a PLINK .bed"):
        plink.open_bed(prefix)


def test_read_fam_ids(tmp_path):
    def fam(lines):
        (tmp_path / "x.fam").write_text("".join(line + "\n" for line in lines))
        return plink.read_fam(tmp_path / "x")
    assert fam(["f a 0 0 1 -9", "f b 0 0 2 -9", "g c 0 0 0 -9"]) == ["a", "b", "c"]
    assert fam(["f\ta\t0\t0\t1\t-9", "g\ta\t0\t0\t2\t-9", "g\tb\t0\t0\t2\t-9"]) == \
        ["f_a", "g_a", "g_b"]
    with pytest.raises(ValueError, match="not distinct"):
        fam(["f a 0 0 1 -9", "f a 0 0 2 -9"])
    (tmp_path / "x.bim").write_text("1 v0 0 1 A C\n1 v1 0 2 A C\n")
    assert plink.count_sites(tmp_path / "x") == 2


def test_allele_swap_leaves_every_pair_unchanged(naive):
    """Counting A1 or A2 is a convention: g -> 2 - g at any set of sites changes none of the
    six sums, so neither the kinship nor IBS0/1/2 (the claim in include/cuking_amd.h)."""
    rng = np.random.default_rng(11)
    geno = random_genotypes(rng, 24, 300, missing=0.08)
    swapped = geno.copy()
    sites = rng.permutation(300)[:150]
    swapped[:, sites] = np.where(geno[:, sites] >= 0, 2 - geno[:, sites], -1)
    assert (swapped != geno).any()
    i0, j0, c0 = naive.all_pairs_matmul(geno)
    i1, j1, c1 = naive.all_pairs_matmul(swapped)
    assert len(i0) == 24 * 23 // 2
    assert np.array_equal(i0, i1) and np.array_equal(j0, j1) and np.array_equal(c0, c1)
    a, b = naive.king(geno, -1e30), naive.king(swapped, -1e30)
    assert len(a) > 0 and a.tobytes() == b.tobytes()
    # ... and through the file: the bitset of the swapped genotypes gives the same records
    thr = -1e30
    assert np.array_equal(naive.king(geno, thr)[["ibs0", "ibs1", "ibs2"]],
                          naive.king(swapped, thr)[["ibs0", "ibs1", "ibs2"]])


def test_driver_usage_errors_need_no_gpu(tmp_path, capsys):
    from cuking_amd import run
    out = ["--output-uri", str(tmp_path / "out")]
    for argv in (["--bed-uri", "p", "--input-uri", "d"], [], ["--bed_uri", "p", "--synthetic", "8,9"]):
        assert run.main(argv + out) == 1
        err = capsys.readouterr().err
        assert "Error: INVALID_ARGUMENT" in err, err
        for name in ("--input_uri", "--bed_uri", "--synthetic"):
            assert name in err, err
    p = subprocess.run([sys.executable, "-m", "cuking_amd.run", "--bed-uri", "p",
                        "--input-uri", "d", *out], capture_output=True, text=True, timeout=300,
                       cwd=str(ROOT))
    assert p.returncode == 1 and "Error: INVALID_ARGUMENT" in p.stderr, p.stderr


def test_header_is_still_plain_c(tmp_path):
    compile_c99(tmp_path, """
#include "cuking_amd.h"
typedef char abi_is_2[CUKING_ABI_VERSION == 2 ? 1 : -1];
int use(const cuking_submatrix *sm, uint64_t *bits, const uint8_t *rows) {
  const uint8_t magic[3] = {0x6c, 0x1b, 0x01};
  cuking_status (*device)(cuking_ctx *, const cuking_submatrix *, uint32_t, uint64_t *,
                          const uint8_t *, uint64_t, uint32_t, uint32_t, uint32_t, void *) =
      cuking_pack_bed_device;
  (void)device;
  if (cuking_bed_check(magic, 3 + 2 * cuking_bed_row_bytes(5), 5, 2) != CUKING_OK) return 1;
  return (int)cuking_pack_bed_host(sm, 2, bits, rows, cuking_bed_row_bytes(5), 0, 2, 2);
}
""")
    assert _lib.load().cuking_abi_version() == 2


def test_host_pack_under_asan_ubsan(tmp_path):
    """csrc/king_host.cc and a stand-alone driver (tests/bed_host_driver.cc: exact-size heap
    buffers, 37 x 129, shard by shard, one call and chunks) built with AddressSanitizer +
    UBSan.  A program of its own on the CPU: nothing is loaded into Python."""
    run_sanitized_driver(tmp_path, "bed_host_driver")
