"""PLINK .bed input on the GPU: the transpose kernel (csrc/king_bed.hip) against the host
function byte for byte, chunks on several streams, the chunked loader, and the way from a
file to records and to the driver's result table."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from conftest import random_genotypes

import cuking_amd
from cuking_amd import plink

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GUARD = -0x5A5A5A5A5A5A5A5B          # 0xA5A5A5A5A5A5A5A5 as int64

SAMPLES = (1, 3, 4, 5, 13, 37, 64, 65, 130)
SITES = (1, 31, 32, 33, 63, 64, 65, 129, 700)


def blocks(n):
    out = [cuking_amd.Submatrix(n)]
    if n == 37:
        out += [cuking_amd.Submatrix(37, 3, k) for k in range(6)]
    return out


def random_rows(rng, n, m):
    """Any bytes are a legal .bed: [m, ceil(n / 4)] random ones (all four codes, and the
    unused high bits of a row's last byte set at random: they must be ignored)."""
    return rng.integers(0, 256, size=(m, (n + 3) // 4), dtype=np.uint8)


def host_bitset(sm, rows, m, chunks=None):
    wps = cuking_amd.words_per_sample(m)
    bits = np.full((sm.NumSamples(), wps), np.uint64(0xA5A5A5A5A5A5A5A5), dtype=np.uint64)
    cuking_amd.pack_bed_host(sm, bits, rows, rows.shape[1], 0, m, m)
    return bits


def device_rows(rows):
    """The rows as a device tensor that starts 3 bytes into its buffer, as in the file."""
    import torch
    buf = torch.zeros(3 + rows.size, dtype=torch.uint8, device="cuda:0")
    buf[3:].copy_(torch.from_numpy(rows.reshape(-1)))
    return buf[3:]


def device_pack(ctx, sm, rows, m, chunks=None, streams=None):
    """pack_bed into a 0xA5-prefilled bitset with a guard row on either side; returns the
    block's rows as uint64 and checks the guards."""
    import torch
    wps = cuking_amd.words_per_sample(m)
    stored = sm.NumSamples()
    whole = torch.full((stored + 2, wps), GUARD, dtype=torch.int64, device="cuda:0")
    d_rows = device_rows(rows)
    row_bytes = rows.shape[1]
    torch.cuda.synchronize()
    for k, (begin, end) in enumerate(chunks or [(0, m)]):
        ctx.pack_bed(sm, wps, d_rows[begin * row_bytes:end * row_bytes], row_bytes, begin, end, m,
                     whole[1:stored + 1], stream=streams[k] if streams else None)
    torch.cuda.synchronize()
    host = whole.cpu().numpy()
    assert (host[0] == GUARD).all() and (host[-1] == GUARD).all()
    return host[1:stored + 1].view(np.uint64)


@pytest.mark.parametrize("n", SAMPLES)
def test_device_equals_host(ctx, n):
    rng = np.random.default_rng(2000 + n)
    for m in SITES:
        rows = random_rows(rng, n, m)
        for sm in blocks(n):
            assert np.array_equal(device_pack(ctx, sm, rows, m), host_bitset(sm, rows, m)), \
                (n, m, sm)


@pytest.mark.parametrize("n,m,split", [(1000, 1000, 1), (2051, 4099, 1), (2051, 4099, 3)])
def test_device_equals_host_several_tiles(ctx, n, m, split):
    """More than one tile in both directions, odd row_bytes (250 is even, 513 is odd); with a
    split factor every block of it: ranges that start inside a byte, two destination ranges."""
    rows = random_rows(np.random.default_rng(n + split), n, m)
    for shard in range(split * (split + 1) // 2):
        sm = cuking_amd.Submatrix(n, split, shard)
        assert np.array_equal(device_pack(ctx, sm, rows, m), host_bitset(sm, rows, m)), sm


def test_device_matches_pack_host_of_the_triples(ctx):
    """... and the host function's own reference once more on the device: the bitset of
    cuking_pack_host for the genotypes as triples."""
    n, m = 130, 700
    geno = random_genotypes(np.random.default_rng(5), n, m, missing=0.1)
    sm = cuking_amd.Submatrix(n)
    site, sample = np.nonzero(geno.T >= 0)
    want = cuking_amd.new_host_bitset(sm, m)
    cuking_amd.pack_host(sm, want, site, sample, geno.T[site, sample])
    assert np.array_equal(device_pack(ctx, sm, plink.encode_rows(geno), m), want)


@pytest.mark.parametrize("n,m,chunks", [
    (37, 700, [(0, 64), (64, 192), (192, 700)]),
    (300, 1100, [(0, 512), (512, 1088), (1088, 1100)]),   # a last chunk of 12 sites
    (130, 1, [(0, 1)]),
    (130, 63, [(0, 63)]),
])
def test_chunks_on_streams_equal_one_call(ctx, n, m, chunks):
    import torch
    rows = random_rows(np.random.default_rng(m), n, m)
    streams = [torch.cuda.Stream("cuda:0") for _ in chunks]
    for sm in blocks(n):
        want = host_bitset(sm, rows, m)
        assert np.array_equal(device_pack(ctx, sm, rows, m), want)
        assert np.array_equal(device_pack(ctx, sm, rows, m, chunks, streams), want)


def test_launches_are_split(ctx):
    """A cap of 3 workgroups per launch (the option the other kernels' tests use) sends the
    tiles out in many launches: same bitset."""
    n, m = 1000, 1000
    rows = random_rows(np.random.default_rng(9), n, m)
    sm = cuking_amd.Submatrix(n, 2, 1)
    ctx.set_option("max_launch_blocks", 3)
    try:
        got = device_pack(ctx, sm, rows, m)
    finally:
        ctx.set_option("max_launch_blocks", 0)
    assert np.array_equal(got, host_bitset(sm, rows, m))


def test_refused_before_the_device(ctx):
    import torch
    n, m = 37, 700
    sm = cuking_amd.Submatrix(37, 3, 1)
    wps = cuking_amd.words_per_sample(m)
    out = torch.zeros((sm.NumSamples(), wps), dtype=torch.int64, device="cuda:0")
    rows = torch.zeros(704 * 10, dtype=torch.uint8, device="cuda:0")   # (enough for every call)
    for kw in (dict(site_begin=32), dict(site_end=100), dict(site_begin=128, site_end=64),
               dict(site_end=704), dict(row_bytes=6)):
        args = dict(row_bytes=10, site_begin=0, site_end=m, num_sites=m)
        args.update(kw)
        with pytest.raises(cuking_amd.CukingError) as e:
            ctx.pack_bed(sm, wps, rows, out=out, **args)
        assert e.value.status == 1, kw
    torch.cuda.synchronize()
    assert int(out.abs().sum()) == 0


@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    """256 samples x 2048 sites with two planted duplicates and a parent-child pair, as a
    PLINK file set and as the pack_host bitset."""
    d = tmp_path_factory.mktemp("bed")
    rng = np.random.default_rng(21)
    n, m = 256, 2048
    geno = random_genotypes(rng, n, m, missing=0.02)
    geno[100] = geno[3]
    geno[200] = geno[17]
    other = random_genotypes(rng, 1, m, missing=0.0)[0]
    # child of 40 and `other`: one allele from each parent
    a = np.where(geno[40] == 1, rng.integers(0, 2, m), geno[40] // 2)
    b = np.where(other == 1, rng.integers(0, 2, m), other // 2)
    geno[41] = np.where(geno[40] < 0, -1, a + b).astype(np.int8)
    plink.write_plink(d / "cohort", geno)
    sm = cuking_amd.Submatrix(n)
    site, sample = np.nonzero(geno.T >= 0)
    bits = cuking_amd.new_host_bitset(sm, m)
    cuking_amd.pack_host(sm, bits, site, sample, geno.T[site, sample])
    return dict(prefix=d / "cohort", geno=geno, sm=sm, bits=bits, n=n, m=m)


def test_load_bed_many_chunks(ctx, cohort):
    """A tiny chunk_bytes: 64 sites per chunk, 32 chunks through the two staging tensors."""
    import torch
    sm = cohort["sm"]
    one = ctx.load_bed(cohort["prefix"], sm)
    many = ctx.load_bed(cohort["prefix"], sm, chunk_bytes=1)
    out = torch.full((cohort["n"], one.shape[1]), GUARD, dtype=torch.int64, device="cuda:0")
    assert ctx.load_bed(cohort["prefix"], sm, chunk_bytes=3 * 64 * 64, out=out) is out
    torch.cuda.synchronize()
    for got in (one, many, out):
        assert np.array_equal(got.cpu().numpy().view(np.uint64), cohort["bits"])
    # an off-diagonal block of the same file
    sm2 = cuking_amd.Submatrix(cohort["n"], 3, 1)
    got = ctx.load_bed(cohort["prefix"], sm2, chunk_bytes=5000).cpu().numpy().view(np.uint64)
    rows = plink.encode_rows(cohort["geno"])
    assert np.array_equal(got, host_bitset(sm2, rows, cohort["m"]))


def test_end_to_end_records(ctx, cohort, oracle):
    sm, thr = cohort["sm"], 0.1
    wps = cuking_amd.words_per_sample(cohort["m"])
    from_file = ctx.run(sm, wps, ctx.load_bed(cohort["prefix"], sm), thr)
    uploaded = ctx.run(sm, wps, ctx.upload_bitset(cohort["bits"]), thr)
    exp, _, _ = oracle.compute(oracle.submatrix(cohort["n"]), cohort["bits"], thr)
    assert from_file.tobytes() == uploaded.tobytes() == exp.tobytes()
    pairs = {(int(r["sample_i"]), int(r["sample_j"])) for r in from_file}
    assert {(3, 100), (17, 200), (40, 41)} <= pairs


def run_driver(*argv):
    return subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-m", "cuking_amd.run",
                           *map(str, argv)], capture_output=True, text=True, cwd=str(ROOT))


def test_driver_bed_equals_parquet(tmp_path):
    import pyarrow.parquet as pq
    from cuking_amd.inputs import write_input_tables
    n, m = 200, 1500
    geno = random_genotypes(np.random.default_rng(33), n, m, missing=0.03)
    geno[150] = geno[7]
    ids = [f"sample{k}" for k in range(n)]
    plink.write_plink(tmp_path / "plink" / "c", geno, sample_ids=ids)
    write_input_tables(tmp_path / "in", geno, sample_ids=ids, num_files=3)
    p = run_driver("--bed-uri", tmp_path / "plink" / "c", "--output-uri", tmp_path / "out_bed",
                   "--kin-threshold=0.05")
    assert p.returncode == 0, p.stderr
    q = run_driver("--input-uri", tmp_path / "in", "--output-uri", tmp_path / "out_pq",
                   "--kin-threshold=0.05", "--num_reader_threads=4")
    assert q.returncode == 0, q.stderr
    a = pq.read_table(tmp_path / "out_bed" / "part-00000.snappy.parquet")
    b = pq.read_table(tmp_path / "out_pq" / "part-00000.snappy.parquet")
    assert a.num_rows > 0 and a.equals(b)
    assert ("sample7", "sample150") in set(zip(a.column("i").to_pylist(),
                                               a.column("j").to_pylist()))


def test_driver_reports_a_truncated_bed(tmp_path):
    geno = random_genotypes(np.random.default_rng(34), 50, 300)
    plink.write_plink(tmp_path / "c", geno)
    bed = tmp_path / "c.bed"
    size = bed.stat().st_size
    bed.write_bytes(bed.read_bytes()[:-5])
    p = run_driver("--bed_uri", tmp_path / "c", "--output-uri", tmp_path / "out")
    assert p.returncode == 1, p.stderr
    assert f"{size - 5} bytes" in p.stderr and str(size) in p.stderr, p.stderr
