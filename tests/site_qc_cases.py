"""What the CPU and the GPU tests of site QC share: the shapes, the masks, the numpy
restatements of the counts and of the site rule, and the packed reference bitset."""
import numpy as np

import cuking_amd

SAMPLES = (1, 3, 37, 65, 130)
SITES = (1, 31, 33, 63, 64, 65, 129, 700)
GUARD = np.uint64(0xA5A5A5A5A5A5A5A5)


def pack(geno):
    """The bitset cuking_pack_host builds for int8 genotypes [samples, sites] (-1 missing)."""
    sm = cuking_amd.Submatrix(geno.shape[0])
    bits = cuking_amd.new_host_bitset(sm, geno.shape[1])
    site, sample = np.nonzero(geno.T >= 0)
    cuking_amd.pack_host(sm, bits, site, sample, geno.T[site, sample].astype(np.int32))
    return bits


def masks(rng, m):
    """name -> bool [m]: the masks every compaction test runs (none of them empty)."""
    out = {"all": np.ones(m, dtype=bool)}
    for name, at in (("first", 0), ("last", m - 1)):
        out[name] = np.zeros(m, dtype=bool)
        out[name][at] = True
    if m > 1:
        out["alternating"] = np.arange(m) % 2 == 1
    for density in (0.02, 0.5, 0.98):
        keep = rng.random(m) < density
        keep[rng.integers(m)] = True
        out[f"random {density}"] = keep
    if m > 128:  # whole empty mask words between full ones (and in front of a partial one)
        keep = np.ones(m, dtype=bool)
        keep[64:128 if m < 256 else 192] = False
        out["empty words"] = keep
        keep = np.zeros(m, dtype=bool)
        keep[128:] = True
        out["empty words first"] = keep
    for k in (32, 33, 64, 65):  # the padding rule: words_per_sample changes between them
        if m >= k:
            keep = np.zeros(m, dtype=bool)
            keep[rng.permutation(m)[:k]] = True
            out[f"exactly {k}"] = keep
    return out


def site_counts_numpy(geno, plane_words):
    """uint32 [64 P, 4]: (hom_ref, het, hom_var, missing) per plane site, padding missing."""
    n, m = geno.shape
    counts = np.zeros((plane_words * 64, 4), dtype=np.uint32)
    counts[:, 3] = n
    for col, g in enumerate((0, 1, 2, -1)):
        counts[:m, col] = (geno == g).sum(axis=0)
    return counts


def sample_counts_numpy(geno):
    """uint32 [samples, 4] over the real sites only."""
    return np.stack([(geno == g).sum(axis=1) for g in (0, 1, 2, -1)], axis=1).astype(np.uint32)


def rule_numpy(counts, num_sites, min_call_rate=0.0, min_maf=0.0, min_mac=0, also=None):
    """The site rule of include/cuking_amd.h restated: bool [num_sites].  The thresholds are
    float32 values, every product and comparison is in double."""
    c = np.asarray(counts)[:num_sites].astype(np.int64)
    called = c[:, 0] + c[:, 1] + c[:, 2]
    n = called + c[:, 3]
    alt = c[:, 1] + 2 * c[:, 2]
    minor = np.minimum(alt, 2 * called - alt)
    rate, maf = np.float64(np.float32(min_call_rate)), np.float64(np.float32(min_maf))
    keep = (called > 0) & (called.astype(np.float64) >= rate * n.astype(np.float64)) & \
        (minor.astype(np.float64) >= maf * (2 * called).astype(np.float64)) & (minor >= min_mac)
    if also is not None:
        keep &= np.asarray(also).astype(bool)
    return keep


def qc_cohort(seed, n, m, low_call, monomorphic):
    """Genotypes [n, m] with planted duplicates and a parent-child pair (the cohort of
    test_gpu_bed.py), then `low_call` sites made missing in 30 % of the samples and
    `monomorphic` sites made hom-ref wherever they are called.  Returns (geno, bad): bad =
    the bool [m] of those sites -- exactly the ones min_call_rate 0.95 / min_mac 1 drop."""
    from conftest import random_genotypes
    rng = np.random.default_rng(seed)
    geno = random_genotypes(rng, n, m, missing=0.02)
    geno[n // 2] = geno[3]
    geno[n - 5] = geno[17]
    other = random_genotypes(rng, 1, m, missing=0.0)[0]
    a = np.where(geno[40] == 1, rng.integers(0, 2, m), geno[40] // 2)
    b = np.where(other == 1, rng.integers(0, 2, m), other // 2)
    geno[41] = np.where(geno[40] < 0, -1, a + b).astype(np.int8)
    # (the few sites that miss the call rate by chance are among the ones made worse)
    base = rule_numpy(site_counts_numpy(geno, (m + 63) // 64), m, 0.95, 0.0, 1)
    sites = rng.permutation(m)
    sites = np.concatenate([sites[~base[sites]], sites[base[sites]]])
    low, mono = sites[:low_call], sites[low_call:low_call + monomorphic]
    rows = rng.permutation(n)[:int(0.3 * n)]
    geno[np.ix_(rows, low)] = -1
    geno[:, mono] = np.where(geno[:, mono] >= 0, 0, -1)
    bad = np.zeros(m, dtype=bool)
    bad[low] = bad[mono] = True
    return geno, bad
