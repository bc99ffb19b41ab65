"""Site QC on the GPU (csrc/king_site_qc.hip): the count kernels against numpy, the
compaction byte for byte against the host function, and the way from an unfiltered cohort to
records, matrix and the driver's result table on the kept sites."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from conftest import random_genotypes
from site_qc_cases import (SAMPLES, SITES, masks, pack, qc_cohort, rule_numpy,
                           sample_counts_numpy, site_counts_numpy)

import cuking_amd
from cuking_amd import plink

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GUARD = -0x5A5A5A5A5A5A5A5B          # 0xA5A5A5A5A5A5A5A5 as int64
GUARD32 = -0x5A5A5A5B                # 0xA5A5A5A5 as int32

# csrc/king_site_qc.hip: a wavefront of the count kernel adds up at most kSiteWaveSamples = 504
# samples in its bit-sliced counters (9 planes hold 511) before it flushes them, a workgroup of
# four wavefronts kSiteBlockSamples = 2016.  The launch hands out chunks that long only when
# samples x column tiles reach kSiteTargetBlocks x 2016 = 2048 x 2016 (4.13 M); below that the
# chunks are shorter.
BLOCK_SAMPLES = 2016
FULL_CHUNKS_FROM = 2048 * 2016


def device_site_counts(ctx, bits, ranges=None):
    """site_counts of the host bitset into a zeroed tensor with guard words behind it;
    `ranges`: row ranges, one call each."""
    import torch
    wps = bits.shape[1]
    slots = wps // 2 * 64 * 4
    whole = torch.full((slots + 64,), GUARD32, dtype=torch.int32, device="cuda:0")
    whole[:slots] = 0
    out = whole[:slots].view(-1, 4)
    d_bits = ctx.upload_bitset(bits)
    for begin, end in ranges or [(0, bits.shape[0])]:
        assert ctx.site_counts(d_bits[begin:end], wps, out=out) is out
    torch.cuda.synchronize()
    host = whole.cpu().numpy()
    assert (host[slots:] == GUARD32).all()
    return host[:slots].view(np.uint32).reshape(-1, 4)


@pytest.mark.parametrize("n", (1, 3, 64, 65, 130, 300))
def test_site_and_sample_counts_match_numpy(ctx, n):
    import torch
    rng = np.random.default_rng(4000 + n)
    for m in (1, 31, 33, 64, 65, 129, 700, 4099):
        geno = random_genotypes(rng, n, m, missing=0.1)
        bits = pack(geno)
        wps = bits.shape[1]
        want = site_counts_numpy(geno, wps // 2)
        got = device_site_counts(ctx, bits)
        assert np.array_equal(got, want), (n, m)
        assert (got.sum(axis=1) == n).all()
        # accumulation: two calls on two row ranges equal one call
        if n > 1:
            cut = n // 3 + 1
            assert np.array_equal(device_site_counts(ctx, bits, [(cut, n), (0, cut)]), want), (n, m)
        # per sample, the padding excluded: the four sum to m, not to 64 P
        whole = torch.full((n + 2, 4), GUARD32, dtype=torch.int32, device="cuda:0")
        ctx.sample_counts(ctx.upload_bitset(bits), wps, m, out=whole[1:n + 1])
        torch.cuda.synchronize()
        host = whole.cpu().numpy()
        assert (host[0] == GUARD32).all() and (host[-1] == GUARD32).all()
        per_sample = host[1:n + 1].view(np.uint32)
        assert np.array_equal(per_sample, sample_counts_numpy(geno)), (n, m)
        assert (per_sample.sum(axis=1) == m).all()


def test_counters_do_not_overflow(ctx):
    """All-ones (every sample missing at every site: each lane's `missing` counter takes every
    sample), all-zeros and a random het plane, with enough samples that every wavefront counts
    its full 504 -- FULL_CHUNKS_FROM samples at one column tile, far more than 4 x
    BLOCK_SAMPLES."""
    import torch
    n, wps = FULL_CHUNKS_FROM + 70_003, 2
    assert n >= 4 * BLOCK_SAMPLES
    for fill, column in ((-1, 3), (0, 0)):
        bits = torch.full((n, wps), fill, dtype=torch.int64, device="cuda:0")
        got = ctx.site_counts(bits, wps).cpu().numpy().view(np.uint32)
        want = np.zeros((64, 4), dtype=np.uint32)
        want[:, column] = n
        assert np.array_equal(got, want), fill
    bits = torch.zeros((n, wps), dtype=torch.int64, device="cuda:0")
    bits[:, 0] = torch.randint(-2 ** 63, 2 ** 63 - 1, (n,), dtype=torch.int64, device="cuda:0")
    het = torch.stack([((bits[:, 0] >> b) & 1).sum() for b in range(64)]).cpu().numpy()
    got = ctx.site_counts(bits, wps).cpu().numpy().view(np.uint32)
    assert np.array_equal(got[:, 1], het) and np.array_equal(got[:, 0], n - het)
    assert not got[:, 2:].any()


@pytest.fixture(scope="module")
def tiled_shapes():
    """Several sample chunks per column (5000 x 200) and several column tiles (300 x 20000)."""
    out = []
    for n, m in ((5000, 200), (300, 20000)):
        geno = random_genotypes(np.random.default_rng(n + m), n, m, missing=0.1)
        bits = pack(geno)
        out.append((geno, bits, site_counts_numpy(geno, bits.shape[1] // 2)))
    return out


def test_counts_several_chunks_and_tiles(ctx, tiled_shapes):
    import torch
    for geno, bits, want in tiled_shapes:
        assert np.array_equal(device_site_counts(ctx, bits), want), geno.shape
        got = ctx.sample_counts(ctx.upload_bitset(bits), bits.shape[1], geno.shape[1])
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy().view(np.uint32), sample_counts_numpy(geno))


def test_count_launches_are_split(ctx, tiled_shapes):
    """A cap of 3 workgroups per launch sends the work out in many launches: same counts."""
    import torch
    ctx.set_option("max_launch_blocks", 3)
    try:
        for geno, bits, want in tiled_shapes:
            assert np.array_equal(device_site_counts(ctx, bits), want), geno.shape
            got = ctx.sample_counts(ctx.upload_bitset(bits), bits.shape[1], geno.shape[1])
            torch.cuda.synchronize()
            assert np.array_equal(got.cpu().numpy().view(np.uint32), sample_counts_numpy(geno))
    finally:
        ctx.set_option("max_launch_blocks", 0)


def device_compact(ctx, d_bits, wps, keep_words, m, rows, streams=None):
    """compact_sites into a 0xA5-prefilled tensor with a guard row on either side; `streams`:
    two streams that take the two halves of the rows."""
    import torch
    kept = int(cuking_amd.site_mask_bool(keep_words, m).sum())
    wps_out = cuking_amd.words_per_sample(kept)
    whole = torch.full((rows + 2, wps_out), GUARD, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    if streams is None:
        out, got_wps, got_kept = ctx.compact_sites(d_bits, wps, keep_words, m, out=whole[1:rows + 1])
        assert (got_wps, got_kept) == (wps_out, kept)
    else:
        cut = rows // 2
        for (begin, end), stream in zip(((0, cut), (cut, rows)), streams):
            ctx.compact_sites(d_bits[begin:end], wps, keep_words, m,
                              out=whole[1 + begin:1 + end], stream=stream)
    torch.cuda.synchronize()
    host = whole.cpu().numpy()
    assert (host[0] == GUARD).all() and (host[-1] == GUARD).all()
    return host[1:rows + 1].view(np.uint64)


@pytest.mark.parametrize("n", SAMPLES)
def test_compaction_equals_host(ctx, n):
    rng = np.random.default_rng(5000 + n)
    for m in SITES:
        bits = pack(random_genotypes(rng, n, m, missing=0.1))
        wps = bits.shape[1]
        d_bits = ctx.upload_bitset(bits)
        for name, keep in masks(rng, m).items():
            words = cuking_amd.site_mask_words(keep)
            want, _, _ = cuking_amd.compact_sites_host(bits, wps, words, m)
            assert np.array_equal(device_compact(ctx, d_bits, wps, words, m, n), want), (n, m, name)


def test_compaction_large_and_on_two_streams(ctx):
    """Random 64-bit words (a bitset need not come from genotypes: padding aside, every code
    is legal), 2051 x 4099 at density 0.5: many workgroups, row groups that end inside one."""
    import torch
    rng = np.random.default_rng(77)
    n, m = 2051, 4099
    wps = cuking_amd.words_per_sample(m)
    bits = rng.integers(0, 2 ** 64, size=(n, wps), dtype=np.uint64)
    keep = rng.random(m) < 0.5
    words = cuking_amd.site_mask_words(keep)
    want, _, _ = cuking_amd.compact_sites_host(bits, wps, words, m)
    d_bits = ctx.upload_bitset(bits)
    assert np.array_equal(device_compact(ctx, d_bits, wps, words, m, n), want)
    streams = [torch.cuda.Stream("cuda:0") for _ in range(2)]
    assert np.array_equal(device_compact(ctx, d_bits, wps, words, m, n, streams), want)
    ctx.set_option("max_launch_blocks", 3)
    try:
        small = device_compact(ctx, d_bits[:130], wps, words, m, 130)
    finally:
        ctx.set_option("max_launch_blocks", 0)
    assert np.array_equal(small, want[:130])


def test_refused_before_the_device(ctx):
    import torch
    m = 700
    wps = cuking_amd.words_per_sample(m)
    bits = torch.zeros((5, wps), dtype=torch.int64, device="cuda:0")
    none = np.zeros(wps // 2, dtype=np.uint64)
    with pytest.raises(cuking_amd.CukingError, match="no site passes") as e:
        ctx.compact_sites(bits, wps, none, m)
    assert e.value.status == 1
    beyond = none.copy()
    beyond[-1] = np.uint64(1) << np.uint64(63)
    with pytest.raises(cuking_amd.CukingError) as e:
        ctx.compact_sites(bits, wps, beyond, m)
    assert e.value.status == 1
    with pytest.raises(cuking_amd.CukingError) as e:
        ctx.sample_counts(bits, wps, 300)
    assert e.value.status == 1
    with pytest.raises(cuking_amd.CukingError, match="no site passes"):
        ctx.filter_sites(bits, wps, m, min_mac=1)       # all hom-ref: nothing is polymorphic


@pytest.fixture(scope="module")
def cohort():
    """256 x 2048 with planted relatives; 300 sites missing in 30 % of the samples and 200
    monomorphic ones."""
    geno, bad = qc_cohort(21, 256, 2048, 300, 200)
    return dict(geno=geno, bad=bad, bits=pack(geno), n=256, m=2048)


def test_end_to_end_filter_then_records_and_matrix(ctx, cohort, oracle):
    import torch
    n, m, geno = cohort["n"], cohort["m"], cohort["geno"]
    wps = cuking_amd.words_per_sample(m)
    qc = ctx.filter_sites(ctx.upload_bitset(cohort["bits"]), wps, m, min_call_rate=0.95, min_mac=1)
    assert np.array_equal(qc.keep(), ~cohort["bad"])
    assert qc.num_sites == m - 500 and qc.words_per_sample == cuking_amd.words_per_sample(m - 500)
    assert np.array_equal(qc.kept_index(), np.flatnonzero(~cohort["bad"]))
    assert np.array_equal(qc.counts(), site_counts_numpy(geno, wps // 2)[:m])
    called = (geno >= 0).sum(axis=0)
    assert np.allclose(qc.call_rate(), called / n)
    assert np.allclose(qc.allele_freq(), np.where(geno > 0, geno, 0).sum(axis=0) / (2 * called))
    want_bits = pack(geno[:, ~cohort["bad"]])
    torch.cuda.synchronize()
    assert np.array_equal(qc.bits.cpu().numpy().view(np.uint64), want_bits)
    sm, thr = cuking_amd.Submatrix(n), 0.1
    got = ctx.run(sm, qc.words_per_sample, qc.bits, thr)
    exp, _, _ = oracle.compute(oracle.submatrix(n), want_bits, thr)
    assert got.tobytes() == exp.tobytes()
    pairs = {(int(r["sample_i"]), int(r["sample_j"])) for r in got}
    assert {(3, 128), (17, 251), (40, 41)} <= pairs
    a = ctx.kin_matrix(sm, qc.words_per_sample, qc.bits, symmetric=True)
    b = ctx.kin_matrix(sm, qc.words_per_sample, ctx.upload_bitset(want_bits), symmetric=True)
    torch.cuda.synchronize()
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def run_driver(*argv):
    return subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-m", "cuking_amd.run",
                           *map(str, argv)], capture_output=True, text=True, cwd=str(ROOT))


def test_driver_filters_like_a_filtered_file(tmp_path):
    import pyarrow.parquet as pq
    n, m = 200, 1500
    geno, bad = qc_cohort(33, n, m, 200, 150)
    ids = [f"sample{k}" for k in range(n)]
    plink.write_plink(tmp_path / "all" / "c", geno, sample_ids=ids)
    plink.write_plink(tmp_path / "kept" / "c", geno[:, ~bad], sample_ids=ids)
    p = run_driver("--bed-uri", tmp_path / "all" / "c", "--output-uri", tmp_path / "out_qc",
                   "--kin-threshold=0.05", "--site-min-call-rate", "0.95", "--site-min-mac", "1",
                   "--site-qc-uri", tmp_path / "q.npz")
    assert p.returncode == 0, p.stderr
    q = run_driver("--bed-uri", tmp_path / "kept" / "c", "--output-uri", tmp_path / "out_kept",
                   "--kin-threshold=0.05")
    assert q.returncode == 0, q.stderr
    a = pq.read_table(tmp_path / "out_qc" / "part-00000.snappy.parquet")
    b = pq.read_table(tmp_path / "out_kept" / "part-00000.snappy.parquet")
    assert a.num_rows > 0 and a.equals(b)
    assert ("sample3", "sample100") in set(zip(a.column("i").to_pylist(), a.column("j").to_pylist()))
    report = np.load(tmp_path / "q.npz")
    counts = site_counts_numpy(geno, cuking_amd.words_per_sample(m) // 2)[:m]
    assert np.array_equal(report["site_counts"], counts)
    assert np.array_equal(report["keep"], rule_numpy(counts, m, 0.95, 0.0, 1))
    assert np.array_equal(report["keep"], ~bad)
    assert np.array_equal(report["sample_counts"], sample_counts_numpy(geno))
    assert report["samples"].tolist() == ids
    assert (float(report["min_call_rate"]), float(report["min_maf"]), int(report["min_mac"])) == \
        (float(np.float32(0.95)), 0.0, 1)
    # a rule nothing passes: exit status 1 and the library's message
    r = run_driver("--bed-uri", tmp_path / "all" / "c", "--output-uri", tmp_path / "out_none",
                   "--site-min-maf", "0.6")
    assert r.returncode == 1 and "no site passes" in r.stderr, r.stderr
