"""What the unrelated-set tests share (test_unrelated_host.py, test_gpu_unrelated.py): the
yardstick -- a pure-Python sequential greedy plus union-find that shares nothing with the
library -- and the graphs both files run.  A graph is (i, j, kin) arrays; `records` turns it
into the 24-byte records the library reads."""
import math

import numpy as np

f32 = np.float32
RESULT_DTYPE = np.dtype([("sample_i", "<u4"), ("sample_j", "<u4"), ("kin", "<f4"),
                         ("ibs0", "<u4"), ("ibs1", "<u4"), ("ibs2", "<u4")])


def records(i, j, kin=0.25):
    i = np.asarray(i, dtype=np.uint32).reshape(-1)
    out = np.zeros(i.size, dtype=RESULT_DTYPE)
    out["sample_i"], out["sample_j"] = i, np.asarray(j, dtype=np.uint32).reshape(-1)
    out["kin"] = np.broadcast_to(np.asarray(kin, dtype=f32), i.shape)
    out["ibs0"], out["ibs1"], out["ibs2"] = 1, 2, 3          # never read
    return out


# ---- the yardstick ---------------------------------------------------------------------------
def rank(p):
    """Orders float32 priorities as the contract does: NaN below every number, then by value,
    -0.0 below +0.0 (the order of the bit patterns' order-preserving map)."""
    p = float(f32(p))
    if math.isnan(p):
        return (0, 0.0, 0)
    return (1, p, 0 if math.copysign(1.0, p) < 0 else 1)


def edge_set(recs, threshold):
    thr = f32(threshold)
    return {(int(r["sample_i"]), int(r["sample_j"])) for r in recs if f32(r["kin"]) > thr}


def degrees(recs, n, threshold=-np.inf):
    """Distinct partners per sample."""
    deg = np.zeros(n, dtype=np.int64)
    for a, b in edge_set(recs, threshold):
        deg[a] += 1
        deg[b] += 1
    return deg


def yardstick(recs, n, threshold=-np.inf, priority=None):
    """(keep uint8, family uint32): the sequential greedy in descending (priority, -index)
    order over the edge set, and union-find with the lowest index as root."""
    edges = edge_set(recs, threshold)
    adj = [[] for _ in range(n)]
    for a, b in edges:
        assert 0 <= a < b < n
        adj[a].append(b)
        adj[b].append(a)
    if priority is None:
        priority = [-f32(len(adj[s])) for s in range(n)]
    order = sorted(range(n), key=lambda s: (rank(priority[s]), -s), reverse=True)
    keep = np.zeros(n, dtype=np.uint8)
    for s in order:
        if not any(keep[t] for t in adj[s]):
            keep[s] = 1
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in edges:
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    family = np.array([find(s) for s in range(n)], dtype=np.uint32)
    return keep, family


def check_properties(recs, n, threshold, keep):
    """Independent and maximal, whatever the order was."""
    edges = edge_set(recs, threshold)
    has_kept_neighbour = np.zeros(n, dtype=bool)
    for a, b in edges:
        assert not (keep[a] and keep[b]), f"edge ({a}, {b}) has both ends kept"
        has_kept_neighbour[a] |= bool(keep[b])
        has_kept_neighbour[b] |= bool(keep[a])
    assert set(np.unique(keep)) <= {0, 1}
    lonely = np.flatnonzero((keep == 0) & ~has_kept_neighbour)
    assert lonely.size == 0, f"dropped without a kept neighbour: {lonely[:8].tolist()}"


# ---- graphs -----------------------------------------------------------------------------------
def path(n):
    return np.arange(n - 1), np.arange(1, n)


def clique(n, base=0):
    i, j = np.triu_indices(n, 1)
    return i + base, j + base


def family_graph(seed, n=3000, num_edges=6000):
    """Family-like: cliques and chains of 2..6 samples planted over a shuffled cohort, random
    extra edges up to `num_edges` distinct ones; kinships in (0.05, 0.5)."""
    rng = np.random.default_rng(seed)
    order = rng.permutation(n)
    edges = set()
    at = 0
    while at + 6 <= n and len(edges) < num_edges * 2 // 3:
        size = int(rng.integers(2, 7))
        members = order[at:at + size]
        at += size
        if rng.random() < 0.5:
            pairs = [(members[a], members[b]) for a in range(size) for b in range(a + 1, size)]
        else:
            pairs = [(members[a], members[a + 1]) for a in range(size - 1)]
        edges.update((int(min(p)), int(max(p))) for p in pairs)
    while len(edges) < num_edges:
        a, b = (int(x) for x in rng.integers(0, n, 2))
        if a != b:
            edges.add((min(a, b), max(a, b)))
    e = np.array(sorted(edges), dtype=np.int64)
    e = e[rng.permutation(len(e))]
    kin = rng.uniform(0.05, 0.5, size=len(e)).astype(f32)
    return e[:, 0], e[:, 1], kin


def hand_made():
    """name -> (records, num_samples, threshold, priority or None)."""
    rng = np.random.default_rng(5)
    cases = {}
    cases["empty"] = (records([], []), 7, -np.inf, None)
    cases["one_edge"] = (records([2], [5]), 8, -np.inf, None)
    p9 = records(*path(9))
    cases["path9_ascending"] = (p9, 9, -np.inf, np.arange(9, dtype=f32))
    cases["path9_descending"] = (p9, 9, -np.inf, -np.arange(9, dtype=f32))
    cases["path9_alternating"] = (p9, 9, -np.inf, (np.arange(9) % 2).astype(f32))
    cases["path9_default"] = (p9, 9, -np.inf, None)
    star = records(np.zeros(11, dtype=int) + 4, np.arange(5, 16))
    cases["star_default"] = (star, 16, -np.inf, None)
    cases["star_centre_first"] = (star, 16, -np.inf, np.eye(16, dtype=f32)[4])
    cases["clique70"] = (records(*clique(70, base=3)), 80, -np.inf, None)
    cases["clique70_priority"] = (records(*clique(70, base=3)), 80, -np.inf,
                                  rng.normal(size=80).astype(f32))
    # two components joined only by a record BELOW the prune threshold
    two = records([0, 1, 4, 5, 2], [1, 2, 5, 6, 4], [0.3, 0.3, 0.3, 0.3, 0.06])
    cases["bridge_below_threshold"] = (two, 7, 0.0884, None)
    cases["bridge_at_threshold"] = (records([0, 2, 1], [1, 3, 2], [0.3, 0.3, 0.0884]), 4,
                                    f32(0.0884), None)       # strict: equal is no edge
    # a 5-cycle whose edge (0, 1) comes three times: with distinct partners every degree is 2
    # and the answer is {0, 2}; counting the repeats would put 0 and 1 last and give {2, 4}
    cases["edge_three_times"] = (records([0, 0, 1, 2, 0, 3, 0], [1, 1, 2, 3, 1, 4, 4]), 6,
                                 -np.inf, None)
    cases["edge_once"] = (records([0, 1, 2, 3, 0], [1, 2, 3, 4, 4]), 6, -np.inf, None)
    cases["equal_priorities"] = (records(*path(6)), 6, -np.inf, np.zeros(6, dtype=f32))
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, np.nan, 1.0, -1.0, np.inf, 0.0],
                       dtype=f32)
    cases["special_priorities_path"] = (records(*path(10)), 10, -np.inf, special)
    cases["special_priorities_clique"] = (records(*clique(10)), 10, -np.inf, special[::-1].copy())
    cases["all_nan_priorities"] = (records(*path(7)), 7, -np.inf, np.full(7, np.nan, dtype=f32))
    cases["minus_inf_threshold"] = (records([0, 1], [1, 2], [-1.0, 0.4]), 3, -np.inf, None)
    return cases
