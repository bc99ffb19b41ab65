"""Unrelated set and families on the device (cuking_unrelated_set, KingContext.unrelated_set
and .prune): the device result equals BOTH the host ABI function and the pure-Python yardstick
of unrelated_cases.py, byte for byte.

Graphs: the hand-made ones of the host tests; record counts that cross the wavefront, the
workgroup and the grid-stride boundaries of the append and the compaction (0, 1, 63, 64, 65,
257, 65,537 records over 20,000 samples); a descending path of 600 (300 rounds, many batches
of the round loop); a clique of 70 (one address under more than a wavefront of atomicMax);
repeats in shuffled order; a threshold inside the records' range; and end to end from bitsets
on 384 samples x 2,048 sites with planted duplicates, parent-child, siblings and a
three-generation chain."""
import functools
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import cuking_amd
from cuking_amd import _lib, api
from unrelated_cases import (check_properties, degrees, family_graph, hand_made, path, records,
                             yardstick)

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
f32 = np.float32
CASES = hand_made()
KIN = 0.0442


def to_device(recs):
    import torch
    words = np.ascontiguousarray(recs).view(np.int32).reshape(-1, 6)
    if len(words) == 0:
        return torch.zeros((1, 6), dtype=torch.int32, device="cuda:0")
    return torch.from_numpy(words.copy()).to("cuda:0")


def run_device(ctx, recs, n, threshold=-np.inf, priority=None):
    import torch
    prio = None if priority is None else \
        torch.from_numpy(np.ascontiguousarray(priority, dtype=f32)).to("cuda:0")
    got = ctx.unrelated_set(to_device(recs), len(recs), n, threshold, priority=prio)
    return got, got.keep.cpu().numpy(), got.family.cpu().numpy().view(np.uint32)


@functools.lru_cache(maxsize=None)
def expected(name):
    recs, n, threshold, priority = CASES[name]
    return yardstick(recs, n, threshold, priority)


def check_device(ctx, recs, n, threshold=-np.inf, priority=None, exp=None):
    got, keep, family = run_device(ctx, recs, n, threshold, priority)
    host_keep, host_family = api.unrelated_set_host(recs, n, threshold, priority=priority)
    exp_keep, exp_family = exp if exp is not None else yardstick(recs, n, threshold, priority)
    assert keep.dtype == np.uint8 and keep.shape == (n,) and family.shape == (n,)
    assert keep.tobytes() == host_keep.tobytes() == exp_keep.tobytes(), \
        np.flatnonzero(keep != exp_keep)[:8]
    assert family.tobytes() == host_family.tobytes() == exp_family.tobytes(), \
        np.flatnonzero(family != exp_family)[:8]
    assert 0 <= got.rounds <= n
    return got


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_made_graph(ctx, name):
    recs, n, threshold, priority = CASES[name]
    got = check_device(ctx, recs, n, threshold, priority, exp=expected(name))
    assert sorted(got.kept().tolist() + got.dropped().tolist()) == list(range(n))
    assert got.kept().tolist() == np.flatnonzero(expected(name)[0]).tolist()
    members = got.families()
    exp_family = expected(name)[1]
    assert sorted(members) == sorted(int(r) for r in np.unique(exp_family)
                                     if (exp_family == r).sum() >= 2)
    for root, m in members.items():
        assert m.tolist() == np.flatnonzero(exp_family == root).tolist()


@functools.lru_cache(maxsize=None)
def big_graph():
    """30,000 distinct edges over 20,000 samples, in a seeded random order."""
    i, j, kin = family_graph(77, n=20000, num_edges=30000)
    recs = records(i, j, kin)
    recs.setflags(write=False)
    return recs


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 257, 65537])
def test_record_counts_across_boundaries(ctx, count):
    base = big_graph()
    recs = np.resize(base, count) if count else base[:0]     # (65,537: the graph and repeats)
    prio = np.random.default_rng(count).normal(size=20000).astype(f32)
    check_device(ctx, recs, 20000, -np.inf, prio)
    check_device(ctx, recs, 20000, -np.inf, None)


def test_descending_path_takes_300_rounds(ctx):
    """Samples 2k and 2k + 1 are decided in round k + 1 and in no other: the slow case of the
    round loop, many batches of it; `rounds` counts the rounds that had a live edge."""
    n = 600
    recs = records(*path(n))
    got = check_device(ctx, recs, n, -np.inf, -np.arange(n, dtype=f32))
    assert got.rounds == 300
    assert got.keep.cpu().numpy().tolist() == [1, 0] * 300
    assert got.families() and list(got.families()) == [0]
    # ascending: the same from the other end
    assert check_device(ctx, recs, n, -np.inf, np.arange(n, dtype=f32)).rounds == 300
    # equal priorities: the lower index wins, which is the descending order again
    assert check_device(ctx, recs, n, -np.inf, np.zeros(n, dtype=f32)).rounds == 300
    # by degree: both ends first, then the interior by index
    assert check_device(ctx, recs, n, -np.inf, None).rounds <= 300


def test_repeats_in_shuffled_order_and_reruns(ctx):
    base = big_graph()[:5000]
    rng = np.random.default_rng(9)
    recs = np.concatenate([base, base[rng.integers(0, len(base), 7000)]])
    recs = recs[rng.permutation(len(recs))]
    exp = yardstick(base, 20000)
    first = check_device(ctx, recs, 20000, exp=exp)
    again = check_device(ctx, recs, 20000, exp=exp)
    assert first.keep.cpu().numpy().tobytes() == again.keep.cpu().numpy().tobytes()
    assert first.family.cpu().numpy().tobytes() == again.family.cpu().numpy().tobytes()
    assert first.rounds == again.rounds
    check_device(ctx, base, 20000, exp=exp)                  # and without the repeats


def test_threshold_inside_the_records(ctx):
    recs = big_graph()[:9000]
    below = int((recs["kin"] <= f32(0.2)).sum())
    assert 0 < below < len(recs)                              # part of the records are no edges
    check_device(ctx, recs, 20000, 0.2, None)
    prio = np.random.default_rng(4).normal(size=20000).astype(f32)
    check_device(ctx, recs, 20000, 0.2, prio)


def test_default_priority_is_minus_degree(ctx):
    recs = np.resize(big_graph()[:4000], 6000)               # repeats: distinct partners count
    deg = degrees(recs, 20000)
    assert deg.max() >= 3
    explicit = -deg.astype(f32)
    _, keep_default, family_default = run_device(ctx, recs, 20000)
    _, keep_explicit, family_explicit = run_device(ctx, recs, 20000, priority=explicit)
    assert keep_default.tobytes() == keep_explicit.tobytes()
    assert family_default.tobytes() == family_explicit.tobytes()
    assert keep_default.tobytes() == yardstick(recs, 20000, priority=explicit)[0].tobytes()
    got = ctx.unrelated_set(to_device(recs), len(recs), 20000, families=False)
    assert got.family is None and got.keep.cpu().numpy().tobytes() == keep_default.tobytes()


def test_invalid_record_is_refused(ctx):
    """One record with sample_i > sample_j; both indices far inside every per-sample array."""
    recs = big_graph()[:300].copy()
    recs["sample_i"][131], recs["sample_j"][131] = 700, 20
    with pytest.raises(cuking_amd.CukingError) as e:
        ctx.unrelated_set(to_device(recs), len(recs), 20000)
    assert e.value.status == _lib.ERR_INVALID_ARGUMENT
    assert "sample_i < sample_j < num_samples" in e.value.message


# ---- end to end ------------------------------------------------------------------------------
N, M = 384, 2048
DUPLICATES = [(3, 200), (40, 383)]
FAMILIES = [[10, 11, 12, 13, 15, 17], [100, 101, 102, 103]]


def make_genotypes(seed=384):
    """Founders' haplotypes; children take one haplotype of each parent per site."""
    rng = np.random.default_rng(seed)
    af = rng.uniform(0.05, 0.5, size=M)
    hap = (rng.random((N, 2, M)) < af).astype(np.int8)
    sites = np.arange(M)

    def child(a, b):
        return np.stack([hap[a, rng.integers(0, 2, M), sites], hap[b, rng.integers(0, 2, M), sites]])
    hap[12], hap[13] = child(10, 11), child(10, 11)      # parent-child x 4, one sibling pair
    hap[15] = child(12, 14)                              # grandchild of 10 and 11
    hap[17] = child(15, 16)                              # great-grandchild: three generations
    hap[102], hap[103] = child(100, 101), child(100, 101)
    geno = hap.sum(axis=1).astype(np.int8)
    geno[rng.random((N, M)) < 0.03] = -1
    for a, b in DUPLICATES:
        geno[b] = geno[a]
    return geno


@functools.lru_cache(maxsize=None)
def cohort():
    from oracle import naive_oracle, pyoracle
    geno = make_genotypes()
    bits = pyoracle.bitset_from_genotypes(geno)
    recs = naive_oracle.king(geno, KIN)
    exp = yardstick(recs, N, KIN)
    for a in (bits, recs) + exp:
        a.setflags(write=False)
    return geno, bits, recs, exp


def check_planted(keep, family):
    for members in FAMILIES:
        assert len({int(family[s]) for s in members}) == 1, members
    for a, b in DUPLICATES:
        assert family[a] == family[b]
        assert int(keep[a]) + int(keep[b]) == 1, (a, b)


def test_end_to_end_prune(ctx):
    _, bits, recs, (exp_keep, exp_family) = cohort()
    check_planted(exp_keep, exp_family)
    check_properties(recs, N, KIN, exp_keep)
    d_bits = ctx.upload_bitset(np.array(bits))
    sm = cuking_amd.Submatrix(N)
    got_recs = ctx.run(sm, bits.shape[1], d_bits, KIN)
    assert got_recs.tobytes() == np.asarray(recs).tobytes()
    got = ctx.prune(sm, bits.shape[1], d_bits, KIN)
    keep, family = got.keep.cpu().numpy(), got.family.cpu().numpy().view(np.uint32)
    assert keep.tobytes() == exp_keep.tobytes() and family.tobytes() == exp_family.tobytes()
    check_planted(keep, family)
    host_keep, host_family = api.unrelated_set_host(got_recs, N, KIN)
    assert host_keep.tobytes() == keep.tobytes() and host_family.tobytes() == family.tobytes()
    # a higher threshold on the same records, with priorities
    prio = np.random.default_rng(2).normal(size=N).astype(f32)
    check_device(ctx, got_recs, N, 0.177, prio)
    with pytest.raises(ValueError, match="unrelated_set"):
        ctx.prune(cuking_amd.Submatrix(N, 2, 1), bits.shape[1], d_bits, KIN)


def test_end_to_end_concatenated_shards(ctx):
    """The three blocks of split_factor = 2 append to ONE device buffer; the unrelated set of
    that buffer is the whole cohort's."""
    import torch
    _, bits, recs, (exp_keep, exp_family) = cohort()
    results = torch.zeros((len(recs) + 8, 6), dtype=torch.int32, device="cuda:0")
    index_and_flag = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    for shard in range(3):
        sm = cuking_amd.Submatrix(N, 2, shard)
        stored = list(range(sm.i_begin, sm.i_end))
        if sm.i_begin != sm.j_begin:
            stored += list(range(sm.j_begin, sm.j_end))
        d_bits = ctx.upload_bitset(np.ascontiguousarray(np.asarray(bits)[stored]))
        ctx.compute_king(sm, bits.shape[1], d_bits, KIN, len(recs) + 8, results,
                         index_and_flag[0:1], index_and_flag[1:2])
        torch.cuda.synchronize()
    count, overflow = index_and_flag.tolist()
    assert (count, overflow) == (len(recs), 0)
    got = cuking_amd.unrelated_set(ctx, results, count, N, prune_threshold=KIN)
    assert got.keep.cpu().numpy().tobytes() == exp_keep.tobytes()
    assert got.family.cpu().numpy().view(np.uint32).tobytes() == exp_family.tobytes()
    # the same buffer twice over (every pair repeated) changes nothing
    twice = torch.cat([results[:count], results[:count]])
    got = ctx.unrelated_set(twice, 2 * count, N, KIN)
    assert got.keep.cpu().numpy().tobytes() == exp_keep.tobytes()


def test_cli_writes_the_unrelated_set(ctx, tmp_path):
    from cuking_amd.synth import cohort_to_device, plan_cohort
    seed = 11
    out = tmp_path / "u.npz"
    p = subprocess.run([sys.executable, "-m", "cuking_amd.run", "--synthetic", f"{N},{M},{seed}",
                        "--output-uri", str(tmp_path / "out"), f"--kin-threshold={KIN}",
                        "--unrelated-uri", str(out)],
                       capture_output=True, text=True, timeout=300, cwd=str(ROOT))
    assert p.returncode == 0, p.stderr[-4000:]
    with np.load(out) as z:
        keep, family, samples, threshold = z["keep"], z["family"], z["samples"], z["threshold"]
    kind, pa, pb = cohort_to_device(plan_cohort(N, seed))
    d_bits = ctx.synth_bitset(seed, kind, pa, pb, 0, N, M)
    got = ctx.prune(cuking_amd.Submatrix(N), d_bits.shape[1], d_bits, KIN)
    assert keep.dtype == np.uint8 and keep.tobytes() == got.keep.cpu().numpy().tobytes()
    assert family.tobytes() == got.family.cpu().numpy().view(np.uint32).tobytes()
    assert samples.shape == (N,) and samples[5] == "S0000005"
    assert threshold.dtype == np.float32 and threshold == f32(KIN)
    assert 0 < keep.sum() < N
