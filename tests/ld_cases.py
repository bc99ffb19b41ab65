"""What the CPU and the GPU tests of LD pruning share (numpy only): a cohort with planted LD,
the edge rule of include/cuking_amd.h restated on the genotype matrix with Python integers and
Python floats, the sequential definition of the kept set, and the site-major bitset from
numpy."""
import numpy as np

import cuking_amd

GUARD = np.uint64(0xA5A5A5A5A5A5A5A5)


def ld_cohort(seed, n, m, block=6, copy=0.8, missing=0.1):
    """int8 [n, m] genotypes (-1 missing) with planted LD: within blocks of `block` sites a
    site copies its left neighbour for `copy` of the samples; allele frequencies 0.05 .. 0.5,
    `missing` of the genotypes missing.  With room for them: one monomorphic site, one
    all-missing site and a pair of identical sites."""
    rng = np.random.default_rng(seed)
    af = rng.uniform(0.05, 0.5, size=m)
    geno = ((rng.random((n, m)) < af).astype(np.int8) + (rng.random((n, m)) < af).astype(np.int8))
    for s in range(1, m):
        if s % block:
            take = rng.random(n) < copy
            geno[take, s] = geno[take, s - 1]
    geno[rng.random((n, m)) < missing] = -1
    if m >= 12:
        geno[:, m // 2] = np.where(geno[:, m // 2] >= 0, 0, -1)     # monomorphic
        geno[:, m // 3] = -1                                        # all missing
        geno[:, 9] = geno[:, 7]                                     # identical, 2 apart
    return geno


def sums(x, y):
    """(n, cov, vx, vy) of two genotype columns as Python integers."""
    both = (x >= 0) & (y >= 0)
    a, b = x[both].astype(np.int64), y[both].astype(np.int64)
    n, sx, sy = int(both.sum()), int(a.sum()), int(b.sum())
    sxx, syy, sxy = int((a * a).sum()), int((b * b).sum()), int((a * b).sum())
    return n, n * sxy - sx * sy, n * sxx - sx * sx, n * syy - sy * sy


def ld_edges_numpy(geno, window, r2, group=None):
    """The edge records of the contract, sorted by (a, b): the sums as Python integers from
    the genotype matrix, the comparison in Python floats (IEEE doubles) in the stated order."""
    n, m = geno.shape
    thr = float(np.float32(r2))
    out = []
    for a in range(m):
        for b in range(a + 1, min(m, a + window)):
            if group is not None and group[a] != group[b]:
                continue
            cnt, cov, vx, vy = sums(geno[:, a], geno[:, b])
            if not (vx > 0 and vy > 0):
                continue
            lhs = float(cov) * float(cov)
            rhs = (thr * float(vx)) * float(vy)
            if lhs > rhs:
                kin = np.float32(lhs / (float(vx) * float(vy)))
                out.append((a, b, kin, cnt, 0, 0))
    return np.array(out, dtype=cuking_amd.KING_RESULT_DTYPE)


def priority_numpy(geno):
    """float32 [m]: minor / (2 called), NaN without a called genotype."""
    called = (geno >= 0).sum(axis=0).astype(np.int64)
    alt = np.where(geno > 0, geno, 0).sum(axis=0).astype(np.int64)
    minor = np.minimum(alt, 2 * called - alt)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(called > 0, minor.astype(np.float64) / (2 * called).astype(np.float64),
                        np.nan).astype(np.float32)


def greedy_numpy(edges, priority):
    """bool [m]: the sites taken in descending priority (NaN last, among equals the lower
    index first); a site stays iff none of its neighbours stayed before it."""
    m = len(priority)
    adj = [[] for _ in range(m)]
    for e in edges:
        adj[int(e["sample_i"])].append(int(e["sample_j"]))
        adj[int(e["sample_j"])].append(int(e["sample_i"]))
    p = np.asarray(priority, dtype=np.float64)
    order = sorted(range(m), key=lambda s: (np.isnan(p[s]), -p[s] if not np.isnan(p[s]) else 0.0, s))
    keep = np.zeros(m, dtype=bool)
    for s in order:
        keep[s] = not any(keep[t] for t in adj[s])
    return keep


def site_bits_numpy(geno):
    """uint64 [m, 2, Q]: the site-major bitset of the contract, tail bits set."""
    n, m = geno.shape
    q = (n + 63) // 64
    planes = np.ones((m, 2, q * 64), dtype=np.uint8)
    planes[:, 0, :n] = ((geno == 1) | (geno < 0)).T
    planes[:, 1, :n] = ((geno == 2) | (geno < 0)).T
    return np.packbits(planes, axis=2, bitorder="little").view("<u8").astype(np.uint64).reshape(m, 2, q)


def check_guarantees(keep, edges):
    """No edge joins two kept sites; every dropped site has a kept neighbour."""
    i, j = edges["sample_i"].astype(np.int64), edges["sample_j"].astype(np.int64)
    assert not (keep[i] & keep[j]).any()
    covered = keep.copy()
    covered[i[keep[j]]] = True
    covered[j[keep[i]]] = True
    assert covered.all()


def same_records(a, b):
    """Record arrays sorted by (a, b): equal byte for byte?"""
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def test_the_restatement_is_the_squared_correlation():
    """On the CPU: the integer sums reproduce np.corrcoef(...)**2 over the jointly called
    samples to 1e-14, and 130 x 333 at W = 50, r^2 = 0.2 has several hundred edges."""
    geno = ld_cohort(5, 130, 333)
    checked = 0
    for a in range(0, 333, 7):
        for b in range(a + 1, min(333, a + 5)):
            n, cov, vx, vy = sums(geno[:, a], geno[:, b])
            if vx > 0 and vy > 0:
                both = (geno[:, a] >= 0) & (geno[:, b] >= 0)
                r = np.corrcoef(geno[both, a].astype(float), geno[both, b].astype(float))[0, 1]
                assert abs(cov * cov / (vx * vy) - r * r) < 1e-14
                checked += 1
    assert checked > 100
    edges = ld_edges_numpy(geno, 50, 0.2)
    assert 300 < len(edges) < 3000, len(edges)
    keep = greedy_numpy(edges, priority_numpy(geno))
    check_guarantees(keep, edges)
    assert 0 < keep.sum() < 333
