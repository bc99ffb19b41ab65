"""LD pruning on the GPU (csrc/king_ld.hip): the transpose byte for byte against the host
function, the edge records byte for byte against the host function (the comparison is exact: no
tolerance anywhere), and the way from an unpruned cohort to the kept sites, the records and the
driver's result table."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from ld_cases import greedy_numpy, ld_cohort, ld_edges_numpy, priority_numpy, same_records
from site_qc_cases import pack

import cuking_amd
from cuking_amd import plink

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GUARD = -0x5A5A5A5A5A5A5A5B          # 0xA5A5A5A5A5A5A5A5 as int64
GUARD32 = -0x5A5A5A5B                # 0xA5A5A5A5 as int32


def device_transpose(ctx, d_bits, wps, m, n):
    """transpose_sites into a 0xA5-prefilled tensor with a guard row on either side."""
    import torch
    q = cuking_amd.ld_site_words(n)
    whole = torch.full((m + 2, 2, q), GUARD, dtype=torch.int64, device="cuda:0")
    out = ctx.transpose_sites(d_bits, wps, m, out=whole[1:m + 1])
    torch.cuda.synchronize()
    host = whole.cpu().numpy()
    assert (host[0] == GUARD).all() and (host[-1] == GUARD).all()
    return out, host[1:m + 1].view(np.uint64)


def device_edges(ctx, site_bits, m, n, window, r2, group=None, room=None):
    """ld_edges into a 0xA5-prefilled buffer of `room` records (default: the exact count's
    worth from the host) with guard records behind; returns the sorted host records."""
    import torch
    whole = torch.full((room + 8, 6), GUARD32, dtype=torch.int32, device="cuda:0")
    records, count = ctx.ld_edges(site_bits, m, n, window, r2, group=group, out=whole[:room])
    host = whole.cpu().numpy()
    assert (host[room:] == GUARD32).all()
    recs = host[:count].view(np.uint32).reshape(-1).view(cuking_amd.KING_RESULT_DTYPE).copy()
    return cuking_amd.sort_results(recs), count


@pytest.mark.parametrize("n", (1, 3, 64, 65, 130, 300))
def test_transpose_equals_host(ctx, n):
    rng = np.random.default_rng(7000 + n)
    for m in (1, 31, 64, 65, 129, 700, 4099):
        bits = pack(ld_cohort(int(rng.integers(1 << 30)), n, m))
        wps = bits.shape[1]
        want = cuking_amd.transpose_sites_host(bits, wps, m)
        _, got = device_transpose(ctx, ctx.upload_bitset(bits), wps, m, n)
        assert np.array_equal(got, want), (n, m)


@pytest.mark.parametrize("n", (1, 3, 65, 130, 300))
def test_edges_equal_host(ctx, n):
    import torch
    rng = np.random.default_rng(8000 + n)
    for m in (2, 63, 65, 129, 700):
        bits = pack(ld_cohort(int(rng.integers(1 << 30)), n, m))
        wps = bits.shape[1]
        host_bits = cuking_amd.transpose_sites_host(bits, wps, m)
        site_bits = ctx.transpose_sites(ctx.upload_bitset(bits), wps, m)
        group = (np.arange(m) >= 40).astype(np.int32) + (np.arange(m) >= 100)   # cuts inside a tile
        d_group = torch.from_numpy(group).to("cuda:0")
        for window in (2, 7, 64, 65, 1000):
            for r2 in (0.0, 0.2, 1.0):
                for g, dg in ((None, None), (group, d_group)):
                    want, count = cuking_amd.ld_edges_host(host_bits, m, n, window, r2, group=g)
                    got, got_count = device_edges(ctx, site_bits, m, n, window, r2, dg, room=count)
                    assert got_count == count and same_records(got, want), (n, m, window, r2)
                    if r2 == 1.0:
                        assert count == 0


@pytest.fixture(scope="module")
def large():
    """2051 samples x 4099 sites: 65 row tiles, five chunks of sample words."""
    n, m = 2051, 4099
    bits = pack(ld_cohort(11, n, m))
    site_bits = cuking_amd.transpose_sites_host(bits, bits.shape[1], m)
    want, count = cuking_amd.ld_edges_host(site_bits, m, n, 50, 0.2)
    return dict(n=n, m=m, bits=bits, site_bits=site_bits, want=want, count=count)


def test_several_tiles_and_chunks(ctx, large):
    n, m = large["n"], large["m"]
    assert large["count"] > 1000
    d_bits = ctx.upload_bitset(large["bits"])
    site_bits, host = device_transpose(ctx, d_bits, large["bits"].shape[1], m, n)
    assert np.array_equal(host, large["site_bits"])
    got, count = device_edges(ctx, site_bits.contiguous(), m, n, 50, 0.2, room=large["count"])
    assert count == large["count"] and same_records(got, large["want"])
    ctx.set_option("max_launch_blocks", 3)
    try:
        _, host = device_transpose(ctx, d_bits, large["bits"].shape[1], m, n)
        got, count = device_edges(ctx, site_bits.contiguous(), m, n, 50, 0.2, room=large["count"])
    finally:
        ctx.set_option("max_launch_blocks", 0)
    assert np.array_equal(host, large["site_bits"])
    assert count == large["count"] and same_records(got, large["want"])


def test_random_words(ctx):
    """A bitset need not come from genotypes: random 64-bit words, 2051 x 4099."""
    rng = np.random.default_rng(78)
    n, m = 2051, 4099
    wps = cuking_amd.words_per_sample(m)
    bits = rng.integers(0, 2 ** 64, size=(n, wps), dtype=np.uint64)
    want_bits = cuking_amd.transpose_sites_host(bits, wps, m)
    site_bits, host = device_transpose(ctx, ctx.upload_bitset(bits), wps, m, n)
    assert np.array_equal(host, want_bits)
    want, count = cuking_amd.ld_edges_host(want_bits, m, n, 50, 0.001)
    assert count > 100
    got, got_count = device_edges(ctx, site_bits.contiguous(), m, n, 50, 0.001, room=count)
    assert got_count == count and same_records(got, want)


def test_overflow_on_the_device(ctx, large):
    import torch
    n, m, count = large["n"], large["m"], large["count"]
    site_bits = ctx.upload_bitset(large["site_bits"].reshape(m, -1)).view(m, 2, -1)
    room = count // 3
    whole = torch.full((room + 8, 6), GUARD32, dtype=torch.int32, device="cuda:0")
    with pytest.raises(cuking_amd.ResourceExhaustedError) as e:
        ctx.ld_edges(site_bits, m, n, 50, 0.2, out=whole[:room])
    assert e.value.num_records == count
    host = whole.cpu().numpy()
    assert (host[room:] == GUARD32).all()
    stored = host[:room].view(np.uint32).reshape(-1).view(cuking_amd.KING_RESULT_DTYPE)
    pairs = set(zip(large["want"]["sample_i"].tolist(), large["want"]["sample_j"].tolist()))
    assert len(set(zip(stored["sample_i"].tolist(), stored["sample_j"].tolist())) & pairs) == room
    # the wrapper's default buffer (4 x sites) overflows at r^2 = 0: one retry, exact size
    want, total = cuking_amd.ld_edges_host(large["site_bits"][:300], 300, n, 50, 0.0)
    assert total > 4 * 300
    records, got = ctx.ld_edges(site_bits[:300].contiguous(), 300, n, 50, 0.0)
    assert got == total and records.shape[0] == total
    recs = records.cpu().numpy().view(np.uint32).reshape(-1).view(cuking_amd.KING_RESULT_DTYPE)
    assert same_records(cuking_amd.sort_results(recs.copy()), want)
    with pytest.raises(ValueError):
        ctx.ld_edges(site_bits, m, n, window=1)
    with pytest.raises(cuking_amd.CukingError) as e:
        ctx.transpose_sites(ctx.upload_bitset(large["bits"]), large["bits"].shape[1], 300)
    assert e.value.status == 1


def relatives_cohort(seed, n, m):
    """The LD cohort with two duplicates planted."""
    geno = ld_cohort(seed, n, m)
    geno[n // 2] = geno[3]
    geno[n - 5] = geno[17]
    return geno


def expected_prune(geno, window, r2, group=None):
    """(edges, keep): the host function's edges -- test_ld_host.py holds them bit-equal to
    ld_edges_numpy, which takes seconds at these sizes -- and greedy_numpy's kept set."""
    bits = pack(geno)
    n, m = geno.shape
    edges, _ = cuking_amd.ld_edges_host(cuking_amd.transpose_sites_host(bits, bits.shape[1], m), m,
                                        n, window, r2, group=group)
    return edges, greedy_numpy(edges, priority_numpy(geno))


def test_end_to_end_prune_then_records(ctx, oracle):
    import torch
    n, m = 256, 2048
    geno = relatives_cohort(21, n, m)
    bits = pack(geno)
    wps = bits.shape[1]
    edges, keep = expected_prune(geno, 50, 0.2)
    assert same_records(edges[edges["sample_j"] < 120], ld_edges_numpy(geno[:, :120], 50, 0.2))
    got = ctx.ld_prune(ctx.upload_bitset(bits), wps, m, window=50, r2=0.2)
    assert got.num_edges == len(edges) and same_records(got.edges(), edges)
    assert np.array_equal(got.keep(), keep) and 0 < keep.sum() < m
    assert np.array_equal(got.kept_index(), np.flatnonzero(keep))
    assert got.num_sites == int(keep.sum()) and got.rounds >= 1
    assert got.words_per_sample == cuking_amd.words_per_sample(got.num_sites)
    want_bits = pack(geno[:, keep])
    torch.cuda.synchronize()
    assert np.array_equal(got.bits.cpu().numpy().view(np.uint64), want_bits)
    sm, thr = cuking_amd.Submatrix(n), 0.1
    recs = ctx.run(sm, got.words_per_sample, got.bits, thr)
    exp, _, _ = oracle.compute(oracle.submatrix(n), want_bits, thr)
    assert recs.tobytes() == exp.tobytes()
    assert {(3, 128), (17, 251)} <= {(int(r["sample_i"]), int(r["sample_j"])) for r in recs}
    # nothing to prune: the input comes back as it is
    d_bits = ctx.upload_bitset(bits)
    same = ctx.ld_prune(d_bits, wps, m, window=50, r2=1.0)
    assert same.num_edges == 0 and same.keep().all() and same.bits is d_bits


def run_driver(*argv):
    return subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-m", "cuking_amd.run",
                           *map(str, argv)], capture_output=True, text=True, cwd=str(ROOT))


def test_driver_prunes_like_a_pruned_file(tmp_path):
    import pyarrow.parquet as pq
    n, m = 200, 1500
    geno = relatives_cohort(33, n, m)
    chromosomes = ["1"] * 700 + ["2"] * (m - 700)
    group = (np.arange(m) >= 700).astype(np.int32)
    edges, keep = expected_prune(geno, 50, 0.2, group)
    ids = [f"sample{k}" for k in range(n)]
    plink.write_plink(tmp_path / "all" / "c", geno, sample_ids=ids, chromosomes=chromosomes)
    plink.write_plink(tmp_path / "kept" / "c", geno[:, keep], sample_ids=ids)
    p = run_driver("--bed-uri", tmp_path / "all" / "c", "--output-uri", tmp_path / "out_ld",
                   "--kin-threshold=0.05", "--site-ld-window", "50", "--site-ld-r2", "0.2",
                   "--site-ld-uri", tmp_path / "ld.npz")
    assert p.returncode == 0, p.stderr
    q = run_driver("--bed-uri", tmp_path / "kept" / "c", "--output-uri", tmp_path / "out_kept",
                   "--kin-threshold=0.05")
    assert q.returncode == 0, q.stderr
    a = pq.read_table(tmp_path / "out_ld" / "part-00000.snappy.parquet")
    b = pq.read_table(tmp_path / "out_kept" / "part-00000.snappy.parquet")
    assert a.num_rows > 0 and a.equals(b)
    assert ("sample3", "sample100") in set(zip(a.column("i").to_pylist(), a.column("j").to_pylist()))
    report = np.load(tmp_path / "ld.npz")
    assert np.array_equal(report["keep"], keep)
    assert np.array_equal(report["kept_index"], np.flatnonzero(keep))
    assert int(report["num_edges"]) == len(edges)
    assert (int(report["window"]), float(report["r2"])) == (50, float(np.float32(0.2)))
