"""The input pipeline's fuzzer, without a GPU: the generator of its cases and what every call of
a case must give (numpy and the CPU oracle only, nothing of the library's `*_host` functions).

A case is one cohort (int8 [n, m] genotypes) and a random sequence of 4 to 10 calls on it:
pack_bed, site_counts, sample_counts, compact_sites, filter_sites, transpose_sites, ld_edges,
ld_prune, unrelated_set, prune and a pair-kernel call ("pair": run or kin_matrix) on the bits
filter_sites or ld_prune returned.  `pipeline_cases` yields (tag, geno): the tag is the
reproducer -- every scalar parameter of every call; arrays (masks, bed rows, priorities, groups)
are rebuilt from the call's own `seed`.  `expect_calls(tag, geno)` walks the calls in order and
returns, per call, the arrays it takes and the outputs it must give.  fuzz_cases.run_pipeline
runs them on the device; tests/test_pipeline_cases.py judges the expectations by the loops of
ld_cases.py and by the library's host functions, and the committed sweeps by `sweep_facts`.

The cap n x m x (window - 1) <= 10^8 of ld_edges and ld_prune is met by shrinking the window
alone: the largest n x m of any size class is below 10^6 (MAX_SHAPE), so m never has to give.
ld_prune also keeps m x (window - 1) <= 2 x 10^5: greedy_numpy is a Python loop over the edges."""
import numpy as np

import cuking_amd
from cuking_amd import plink
from ld_cases import greedy_numpy, ld_cohort, priority_numpy, site_bits_numpy
from site_qc_cases import (masks, pack, qc_cohort, rule_numpy, sample_counts_numpy,
                           site_counts_numpy)
import unrelated_cases

f32 = np.float32
SIZE_CLASSES = ("small", "samples", "sites")
KINDS = ("pack_bed", "site_counts", "sample_counts", "compact_sites", "filter_sites",
         "transpose_sites", "ld_edges", "ld_prune", "unrelated_set", "prune", "pair")
NUM_STREAMS = 10                    # more than kMaxStreams = 8 of csrc/king_abi.hip
MAX_STREAMS = 8
LD_WORK = 10 ** 8                   # n x m x (window - 1)
PRUNE_BAND = 2 * 10 ** 5            # m x (window - 1) of an ld_prune draw
MAX_SHAPE = 10 ** 6
PAIR_MAX_SAMPLES = 300
MAX_GRAPH_RECORDS = 20000           # what the pure-Python yardstick takes in a blink
N_SMALL = (1, 3, 4, 5, 63, 64, 65, 128, 129, 130)
M_SMALL = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129)
N_SAMPLES = (256, 512, 1024, 2016)
M_SITES = (256, 512, 4096, 4160)
WINDOWS = (2, 3, 7, 50, 63, 64, 65, 66, 129, "m+5")
R2_MENU = (0.0, 0.001, 0.2, 0.5, 0.99, 1.0)
RATE_MENU = (0.0, 0.5, 0.9, 0.95, 1.0)
MAF_MENU = (0.0, 0.01, 0.05, 0.25, 0.5)
BED_CODES = np.array([2, -1, 1, 0], dtype=np.int8)      # 2-bit code -> n_alt, -1 missing


# ---- the generator ---------------------------------------------------------------------------
def _shape(rng, cls):
    if cls == "small":
        n = int(rng.choice(N_SMALL)) if rng.random() < 0.5 else int(rng.integers(1, 141))
        m = int(rng.choice(M_SMALL)) if rng.random() < 0.5 else int(rng.integers(1, 721))
    elif cls == "samples":
        n = int(rng.choice(N_SAMPLES)) + int(rng.integers(-9, 10))
        m = int(rng.integers(1, 201))
    else:
        n = int(rng.integers(1, 71))
        m = int(rng.choice(M_SITES)) + int(rng.integers(-9, 10))
    assert n * m <= MAX_SHAPE
    return n, m


def _cohort(rng, n, m):
    """(kind, geno): drawn from ld_cohort, qc_cohort or as random 2-bit codes, then with
    all-missing, monomorphic, identical, fully called and all-het sites and two duplicate
    samples planted where there is room."""
    kind = str(rng.choice(["ld", "ld", "qc", "bed"]))
    seed = int(rng.integers(1 << 30))
    if kind == "qc" and (n < 42 or m < 4):
        kind = "ld"
    if kind == "ld":
        geno = ld_cohort(seed, n, m, block=int(rng.choice([3, 6, 12])),
                         missing=float(rng.choice([0.0, 0.02, 0.1, 0.3])))
    elif kind == "qc":
        geno, _ = qc_cohort(seed, n, m, m // 8, m // 10)
    else:
        rows = np.random.default_rng(seed).integers(0, 256, size=(m, (n + 3) // 4), dtype=np.uint8)
        geno = bed_decode(rows, n)
    geno = np.ascontiguousarray(geno, dtype=np.int8)
    sites = rng.permutation(m)
    if m >= 8:
        geno[:, sites[0]] = -1                                           # all missing
        geno[:, sites[1]] = np.where(geno[:, sites[1]] >= 0, 2, -1)      # monomorphic
        geno[:, sites[2]] = geno[:, sites[3]]                            # identical sites
        geno[:, sites[4]] = 1                                            # frequency 0.5, rate 1
        geno[:, sites[5]] = np.where(geno[:, sites[5]] < 0, 0, geno[:, sites[5]])   # rate 1
    if m >= 16:
        geno[:, sites[6]] = -1
        geno[:, sites[7]] = 0
    if n >= 4:
        geno[n - 1] = geno[0]                                            # duplicate samples
    return kind, geno


def _site_rule_values(geno):
    """(call rates, frequencies) the sites of the cohort have, as float32."""
    called = (geno >= 0).sum(axis=0).astype(np.float64)
    alt = np.where(geno > 0, geno, 0).sum(axis=0).astype(np.float64)
    minor = np.minimum(alt, 2 * called - alt)
    some = called > 0
    rates = (called[some] / geno.shape[0]).astype(f32)
    return rates, (minor[some] / (2 * called[some])).astype(f32)


def _pair_r2(geno, a, b):
    from ld_cases import sums
    _, cov, vx, vy = sums(geno[:, a], geno[:, b])
    if not (vx > 0 and vy > 0):
        return None
    return float(f32(float(cov) * float(cov) / (float(vx) * float(vy))))


def _ld_window(rng, n, m, limit_band=None):
    w = WINDOWS[int(rng.integers(len(WINDOWS)))]
    w = m + 5 if w == "m+5" else int(w)
    w = min(w, LD_WORK // (n * m) + 1)
    if limit_band is not None:
        w = min(w, limit_band // m + 1)
    return max(w, 2)


def _ld_r2(rng, geno):
    m = geno.shape[1]
    if rng.random() < 0.25 and m >= 2:
        a = int(rng.integers(0, m - 1))
        b = min(m - 1, a + int(rng.integers(1, 4)))
        r2 = _pair_r2(geno, a, b)
        if r2 is not None and 0.0 <= r2 <= 1.0:
            return r2, [a, b]
    return float(R2_MENU[int(rng.integers(len(R2_MENU)))]), None


def _group_cuts(rng, m):
    """None or 1 to 5 cuts: some at multiples of 64, some inside a tile."""
    if rng.random() < 0.5 or m < 2:
        return None
    cuts = set()
    for _ in range(int(rng.integers(1, 6))):
        if rng.random() < 0.5 and m > 64:
            cuts.add(64 * int(rng.integers(1, (m - 1) // 64 + 1)))
        else:
            cuts.add(int(rng.integers(1, m)))
    return sorted(cuts)


def _priority_mode(rng, with_place):
    mode = str(rng.choice(["none", "random", "tied", "nan"]))
    place = str(rng.choice(["host", "device"])) if with_place else "device"
    return mode, place


def _draw_call(rng, kind, geno):
    n, m = geno.shape
    call = dict(kind=kind, seed=int(rng.integers(1 << 30)))
    if kind == "pack_bed":
        split = min(int(rng.integers(1, 4)), n)
        cuts = sorted({64 * int(rng.integers(1, (m - 1) // 64 + 1))
                       for _ in range(int(rng.integers(0, 3)))}) if m > 64 else []
        call.update(source=str(rng.choice(["encode", "random"])), split=split,
                    shard=int(rng.integers(0, split * (split + 1) // 2)), cuts=cuts,
                    offset=int(rng.choice([1, 3, 5, 7])),
                    chunk_streams=[int(rng.integers(NUM_STREAMS)) for _ in range(len(cuts) + 1)])
    elif kind == "site_counts":
        parts = min(int(rng.choice([1, 1, 2, 3])), n)
        cuts = sorted(int(c) for c in rng.choice(np.arange(1, n), size=parts - 1, replace=False)) \
            if parts > 1 else []
        bounds = [0] + cuts + [n]
        order = [int(p) for p in rng.permutation(parts)]
        call.update(ranges=[[bounds[p], bounds[p + 1]] for p in order],
                    range_streams=[int(rng.integers(NUM_STREAMS)) if rng.random() < 0.4 else -1
                                   for _ in order])
    elif kind == "compact_sites":
        mask = str(rng.choice(["menu", "loguniform", "empty_runs", "exactly"]))
        call.update(mask=mask, guarded=bool(rng.integers(0, 2)))
        if mask == "loguniform":
            call["density"] = float(np.exp(rng.uniform(np.log(1.0 / m), 0.0)))
        if mask == "exactly":
            fits = [k for k in (32, 33, 64, 65) if k <= m]
            call["kept"] = int(rng.choice(fits)) if fits else m
    elif kind == "filter_sites":
        rates, freqs = _site_rule_values(geno)
        rate = float(RATE_MENU[int(rng.integers(len(RATE_MENU)))])
        maf = float(MAF_MENU[int(rng.integers(len(MAF_MENU)))])
        exact = str(rng.choice(["none", "none", "rate", "maf"]))
        if exact == "rate" and rates.size:
            rate = float(rates[int(rng.integers(rates.size))])
        if exact == "maf" and freqs.size:
            maf = float(freqs[int(rng.integers(freqs.size))])
        call.update(min_call_rate=rate, min_maf=maf, min_mac=int(rng.integers(0, 4)),
                    also=bool(rng.random() < 0.4), nothing=bool(rng.random() < 0.08))
        if call["nothing"]:
            call["min_maf"] = 0.6
    elif kind == "ld_edges":
        r2, pair = _ld_r2(rng, geno)
        call.update(window=_ld_window(rng, n, m), r2=r2, r2_pair=pair, group=_group_cuts(rng, m),
                    buffer=str(rng.choice(["default", "default", "exact", "small"])),
                    short=float(rng.random()))
    elif kind == "ld_prune":
        r2, pair = _ld_r2(rng, geno)
        mode, place = _priority_mode(rng, True)
        call.update(window=_ld_window(rng, n, m, PRUNE_BAND), r2=r2, r2_pair=pair,
                    group=_group_cuts(rng, m), priority=mode, place=place,
                    compact=bool(rng.random() < 0.7))
    elif kind in ("unrelated_set", "prune"):
        mode, _ = _priority_mode(rng, False)
        call.update(priority=mode, families=bool(rng.integers(0, 2)),
                    quantile=float(rng.random()))
        if kind == "unrelated_set":
            call["source"] = str(rng.choice(["run", "edges"]))
    elif kind == "pair":
        call.update(call=str(rng.choice(["run", "kin_matrix"])),
                    thr=float(rng.choice([-1e30, 0.0, 0.0884, 0.3])))
    return call


def pipeline_cases(seed: int, cases: int, first_case: int = 0, size_class=None):
    """The cases of run_pipeline, without a context: yields (tag, geno).  Case k of a seed is
    drawn from a generator of its own, seeded by (seed, k, class): it is the same case whatever
    is skipped."""
    if size_class is not None and size_class not in SIZE_CLASSES:
        raise ValueError(f"size_class {size_class!r}: one of {SIZE_CLASSES} or None")
    for case in range(first_case, cases):
        rng = np.random.default_rng([seed, case, 1 + SIZE_CLASSES.index(size_class)
                                     if size_class else 0])
        cls = size_class or str(rng.choice(SIZE_CLASSES, p=[0.9, 0.05, 0.05]))
        n, m = _shape(rng, cls)
        kind, geno = _cohort(rng, n, m)
        count = int(rng.integers(4, 11))
        tour = rng.random() < 0.15       # every stream of the pool once, in one case
        if tour:
            count = NUM_STREAMS
        menu = [k for k in KINDS if k != "pair" or n <= PAIR_MAX_SAMPLES]
        calls = []
        streams = [int(s) for s in rng.permutation(NUM_STREAMS)]
        for c in range(count):
            call = _draw_call(rng, str(rng.choice(menu)), geno)
            call["stream"] = streams[c] if tour else int(rng.integers(NUM_STREAMS))
            call["max_launch_blocks"] = int(rng.choice([0, 0, 0, 3, 7]))
            calls.append(call)
        tag = dict(fuzzer="run_pipeline", seed=seed, case=case, sweep=size_class or "mixed",
                   size_class=cls, n=n, m=m, cohort=kind, calls=calls)
        yield tag, geno


def pipeline_tags(seed: int, cases: int, first_case: int = 0, size_class=None) -> list:
    return [tag for tag, _ in pipeline_cases(seed, cases, first_case, size_class)]


# ---- arrays of a call, from its seed ---------------------------------------------------------
def bed_decode(rows, n):
    """int8 [n, m] genotypes of .bed rows uint8 [m, ceil(n / 4)]: sample s of a row = bits
    2 (s % 4) .. of byte s // 4; 00 hom-var (two A1), 01 missing, 10 het, 11 hom-ref."""
    rows = np.asarray(rows, dtype=np.uint8)
    codes = np.stack([(rows >> np.uint8(s)) & np.uint8(3) for s in (0, 2, 4, 6)], axis=2)
    return np.ascontiguousarray(BED_CODES[codes.reshape(rows.shape[0], -1)[:, :n]].T)


def bed_rows_of(call, geno):
    n, m = geno.shape
    rng = np.random.default_rng(call["seed"])
    if call["source"] == "random":
        return rng.integers(0, 256, size=(m, (n + 3) // 4), dtype=np.uint8)
    rows = plink.encode_rows(geno)
    if n % 4:                            # the spare high bits of a row's last byte: set
        spare = np.uint8((0xFF << (2 * (n % 4))) & 0xFF)
        rows[:, -1] |= rng.integers(0, 256, size=m, dtype=np.uint8) & spare
        rows[0, -1] |= spare
    return rows


def block_samples(sm):
    """The stored samples of a block: its rows, then its columns (a diagonal block's once)."""
    i0, i1, j0, j1 = sm
    rows = np.arange(i0, i1)
    return rows if (i0, i1) == (j0, j1) else np.concatenate([rows, np.arange(j0, j1)])


def mask_of(call, m):
    rng = np.random.default_rng(call["seed"])
    if call["mask"] == "menu":
        menu = masks(rng, m)
        return menu[sorted(menu)[int(rng.integers(len(menu)))]]
    if call["mask"] == "loguniform":
        keep = rng.random(m) < call["density"]
    elif call["mask"] == "empty_runs":
        words = (m + 63) // 64
        full = rng.random(words) < 0.5
        keep = np.repeat(full, 64)[:m] & (rng.random(m) < 0.7)
    else:
        keep = np.zeros(m, dtype=bool)
        keep[rng.permutation(m)[:call["kept"]]] = True
    keep[int(rng.integers(m))] |= not keep.any()
    return keep


def also_of(call, m):
    if not call["also"]:
        return None
    return np.random.default_rng(call["seed"]).random(m) < 0.8


def group_of(cuts, m):
    if cuts is None:
        return None
    return np.searchsorted(np.asarray(cuts), np.arange(m), side="right").astype(np.int32)


def priority_of(call, count):
    """float32 [count] or None: random, a few distinct values (ties), or those with NaN."""
    rng = np.random.default_rng(call["seed"] + 1)
    if call["priority"] == "none":
        return None
    if call["priority"] == "random":
        return rng.random(count).astype(f32)
    p = rng.choice(np.array([0.125, 0.25, 0.5, 1.5], dtype=f32), size=count).astype(f32)
    if call["priority"] == "nan":
        p[rng.random(count) < 0.3] = np.nan
    return p


# ---- expectations ----------------------------------------------------------------------------
def ld_edges_fast(geno, window, r2, group=None):
    """ld_cases.ld_edges_numpy, vectorised: for every offset d the six integer sums of all
    column pairs (a, a + d) at once, in int64; then the same three double operations in the
    same order.  Records sorted by (a, b), byte-identical to the loop's."""
    n, m = geno.shape
    thr = float(f32(r2))
    t = np.ascontiguousarray(geno.T)
    called = (t >= 0).astype(np.int64)
    g = np.where(t > 0, t, 0).astype(np.int64)
    gg = g * g
    group = None if group is None else np.asarray(group)
    parts = []
    for d in range(1, min(window, m)):
        ca, cb, ga, gb = called[:m - d], called[d:], g[:m - d], g[d:]
        cnt = np.einsum("ij,ij->i", ca, cb)
        sx, sy = np.einsum("ij,ij->i", ga, cb), np.einsum("ij,ij->i", ca, gb)
        sxx, syy = np.einsum("ij,ij->i", gg[:m - d], cb), np.einsum("ij,ij->i", ca, gg[d:])
        sxy = np.einsum("ij,ij->i", ga, gb)
        cov, vx, vy = cnt * sxy - sx * sy, cnt * sxx - sx * sx, cnt * syy - sy * sy
        fx, fy, fc = vx.astype(np.float64), vy.astype(np.float64), cov.astype(np.float64)
        lhs = fc * fc
        rhs = (thr * fx) * fy
        edge = (vx > 0) & (vy > 0) & (lhs > rhs)
        if group is not None:
            edge &= group[:m - d] == group[d:]
        a = np.flatnonzero(edge)
        out = np.zeros(a.size, dtype=cuking_amd.KING_RESULT_DTYPE)
        out["sample_i"], out["sample_j"] = a, a + d
        out["kin"] = (lhs[a] / (fx[a] * fy[a])).astype(f32)
        out["ibs0"] = cnt[a]
        parts.append(out)
    if not parts:
        return np.zeros(0, dtype=cuking_amd.KING_RESULT_DTYPE)
    out = np.concatenate(parts)
    return np.ascontiguousarray(out[np.lexsort((out["sample_j"], out["sample_i"]))])


def band_pairs(m, window, group=None):
    """The number of pairs a < b, b - a < window, of one group."""
    total = 0
    for d in range(1, min(window, m)):
        total += m - d if group is None else int((group[:m - d] == group[d:]).sum())
    return total


def greedy_rounds(edges, count, keys):
    """The rounds of the parallel greedy that have a live edge: in a round every live vertex
    whose key is above those of all its live neighbours is kept, it and its neighbours leave."""
    i, j = np.asarray(edges[0], dtype=np.int64), np.asarray(edges[1], dtype=np.int64)
    live, rounds = np.ones(count, dtype=bool), 0
    while True:
        on = live[i] & live[j]
        if not on.any():
            return rounds
        rounds += 1
        a, b = i[on], j[on]
        top = np.zeros(count, dtype=np.uint64)
        np.maximum.at(top, a, keys[b])
        np.maximum.at(top, b, keys[a])
        wins = live & (keys > top)
        gone = wins.copy()
        gone[a[wins[b]]] = True
        gone[b[wins[a]]] = True
        live &= ~gone


def order_keys(priority, count, degree=None):
    """uint64 keys ordered like the contract: higher priority first, among equals the lower
    index, NaN last (positive zero only: the generator draws no negative zero)."""
    p = -degree.astype(np.float64) if priority is None else np.asarray(priority, np.float64)
    rank = np.zeros(count, dtype=np.uint64)
    ok = ~np.isnan(p)
    rank[ok] = 1 + np.unique(p[ok], return_inverse=True)[1].astype(np.uint64)
    return (rank << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.arange(count, dtype=np.uint64))


def _graph_facts(recs, count, thr, priority):
    edges = sorted(unrelated_cases.edge_set(recs, thr))
    e = np.array(edges, dtype=np.int64).reshape(-1, 2)
    degree = np.bincount(e.reshape(-1), minlength=count)
    return greedy_rounds((e[:, 0], e[:, 1]), count, order_keys(priority, count, degree))


def _run_records(geno, quantile):
    """(records of a run over the whole cohort, its threshold): at most 4 n records, the
    threshold a kinship the cohort has (strict `>`: that pair is not a record)."""
    from oracle import pyoracle
    n = geno.shape[0]
    osm = pyoracle.submatrix(n)
    bits = pack(geno)
    kin = np.asarray(pyoracle.all_pairs(osm, bits)[3], dtype=f32)
    kin = np.sort(kin[~np.isnan(kin) & ~np.isinf(kin)])[::-1]
    if kin.size == 0:
        thr = 0.0
    else:
        thr = float(kin[min(kin.size - 1, int(quantile * min(kin.size, 4 * n)))])
    recs, _, _ = pyoracle.compute(osm, bits, thr, threads=8)
    return recs, thr


def symmetric_matrix(geno):
    """The kinship of every pair of the cohort from the oracle: symmetric, the diagonal 0.5 (NaN
    for a sample without a het site)."""
    from oracle import pyoracle
    n = geno.shape[0]
    oi, oj, _, kin = pyoracle.all_pairs(pyoracle.submatrix(n), pack(geno))
    full = np.zeros((n, n), dtype=f32)
    full[oi, oj] = kin
    full[oj, oi] = kin
    has_het = (geno == 1).any(axis=1)
    full[np.diag_indices(n)] = np.where(has_het, f32(0.5), f32("nan"))
    return full


def expect_calls(tag, geno):
    """Per call of the case, in order: a dict of the arrays the call takes and of what it must
    give.  The walk carries what later calls read: the current LD edges (of the last ld_edges)
    and the kept sites of the last filter_sites or ld_prune."""
    n, m = geno.shape
    wps = cuking_amd.words_per_sample(m)
    state = dict(edges=None, keep=np.ones(m, dtype=bool))
    out = []
    for call in tag["calls"]:
        kind, e = call["kind"], {}
        if kind == "pack_bed":
            sm = cuking_amd.Submatrix(n, call["split"], call["shard"]).as_tuple()
            rows = bed_rows_of(call, geno)
            e.update(block=sm, rows=rows, chunks=list(zip([0] + call["cuts"], call["cuts"] + [m])),
                     bits=pack(bed_decode(rows, n)[block_samples(sm)]))
        elif kind == "site_counts":
            e.update(counts=site_counts_numpy(geno, wps // 2))
        elif kind == "sample_counts":
            e.update(counts=sample_counts_numpy(geno))
        elif kind == "compact_sites":
            keep = mask_of(call, m)
            e.update(keep=keep, bits=pack(geno[:, keep]))
        elif kind == "filter_sites":
            also = also_of(call, m)
            counts = site_counts_numpy(geno, wps // 2)
            keep = rule_numpy(counts, m, call["min_call_rate"], call["min_maf"], call["min_mac"],
                              also)
            e.update(also=also, counts=counts[:m], keep=keep, fails=not keep.any())
            if keep.any():
                e["bits"] = pack(geno[:, keep])
                state["keep"] = keep
        elif kind == "transpose_sites":
            e.update(site_bits=site_bits_numpy(geno))
        elif kind == "ld_edges":
            group = group_of(call["group"], m)
            edges = ld_edges_fast(geno, call["window"], call["r2"], group)
            default = max(1, min(m * (call["window"] - 1), 4 * m))
            room = None
            if call["buffer"] == "exact" or call["buffer"] == "small" and len(edges) == 0:
                room = len(edges)
            elif call["buffer"] == "small":
                room = len(edges) - 1 - int(call["short"] * len(edges))
            e.update(group=group, edges=edges, room=room, retries=room is None and
                     len(edges) > default, exhausted=room is not None and room < len(edges),
                     band=band_pairs(m, call["window"], group))
            state["edges"] = edges
        elif kind == "ld_prune":
            group = group_of(call["group"], m)
            edges = ld_edges_fast(geno, call["window"], call["r2"], group)
            priority = priority_of(call, m)
            used = priority_numpy(geno) if priority is None else priority
            keep = greedy_numpy(edges, used)
            e.update(group=group, edges=edges, priority=priority, used=used, keep=keep,
                     band=band_pairs(m, call["window"], group),
                     bits=pack(geno[:, keep]) if call["compact"] and not keep.all() else None)
            state["keep"] = keep if call["compact"] else np.ones(m, dtype=bool)
        elif kind in ("unrelated_set", "prune"):
            if kind == "unrelated_set" and call["source"] == "edges" and \
                    state["edges"] is not None and len(state["edges"]):
                recs, count = state["edges"][:MAX_GRAPH_RECORDS], m
                kins = np.sort(recs["kin"])
                thr = float(kins[int(call["quantile"] * len(kins) * 0.5)])
                source = "edges"
            else:
                recs, thr = _run_records(geno, call["quantile"])
                count, source = n, "run"
                if kind == "unrelated_set" and len(recs):
                    kins = np.sort(recs["kin"])
                    thr = float(kins[int(call["quantile"] * len(kins) * 0.5)])
            priority = priority_of(call, count)
            keep, family = unrelated_cases.yardstick(recs, count, thr, priority)
            e.update(records=recs, count=count, thr=thr, priority=priority, keep=keep,
                     family=family, source=source,
                     rounds=_graph_facts(recs, count, thr, priority))
        elif kind == "pair":
            from oracle import pyoracle
            sub = np.ascontiguousarray(geno[:, state["keep"]])
            e.update(keep=state["keep"].copy())
            if call["call"] == "run":
                e["records"] = pyoracle.compute(pyoracle.submatrix(n), pack(sub), call["thr"],
                                                threads=8)[0]
            else:
                e["matrix"] = symmetric_matrix(sub)
        out.append(e)
    return out


# ---- what a sweep covers, from the generator and the expectations alone ----------------------
def sweep_facts(seed: int, cases: int, size_class=None) -> dict:
    """The counts tests/test_pipeline_cases.py holds every committed sweep to."""
    f = dict(cases=0, calls={k: 0 for k in KINDS}, ld=0, ld_partial=0, retries=0, exhausted=0,
             filters=0, filter_both=0, filter_equal=0, filter_nothing=0, compact_gap=0,
             compact_kept=set(), prune_ties=0, prune_nan=0, rounds2=0, streams=set(),
             tours=0, n_mod8=0, n_mod4=0, n_values=set(), m_values=set())
    for tag, geno in pipeline_cases(seed, cases, 0, size_class):
        n, m = geno.shape
        f["cases"] += 1
        f["n_mod8"] += n % 8 != 0
        f["n_mod4"] += n % 4 != 0
        f["n_values"].add(n)
        f["m_values"].add(m)
        used = [c["stream"] for c in tag["calls"]]
        f["streams"].update(used)
        f["tours"] += len(set(used[:-1])) > MAX_STREAMS
        for call, e in zip(tag["calls"], expect_calls(tag, geno)):
            kind = call["kind"]
            f["calls"][kind] += 1
            if kind in ("ld_edges", "ld_prune"):
                f["ld"] += 1
                f["ld_partial"] += 0 < len(e["edges"]) < e["band"]
            if kind == "ld_edges":
                f["retries"] += e["retries"]
                f["exhausted"] += e["exhausted"]
            if kind == "filter_sites":
                f["filters"] += 1
                f["filter_both"] += e["keep"].any() and not e["keep"].all()
                f["filter_nothing"] += e["fails"]
                f["filter_equal"] += on_equality(e["counts"], call)
            if kind == "compact_sites":
                f["compact_kept"].add(int(e["keep"].sum()))
                words = cuking_amd.site_mask_words(e["keep"]) != 0
                on = np.flatnonzero(words)
                f["compact_gap"] += bool(on.size) and not words[on[0]:on[-1] + 1].all()
            if kind == "ld_prune" and call["priority"] in ("tied", "nan"):
                p, i, j = e["priority"], e["edges"]["sample_i"], e["edges"]["sample_j"]
                tie = (p[i] == p[j]) & (e["keep"][i] | e["keep"][j])
                f["prune_ties"] += bool(tie.any())
                f["prune_nan"] += bool(np.isnan(p).any())
            if kind == "unrelated_set":
                f["rounds2"] += e["rounds"] >= 2
    return f


def on_equality(counts, call) -> bool:
    """Does a comparison of the site rule hold with equality, at a threshold above zero?"""
    c = counts.astype(np.int64)
    called = c[:, 0] + c[:, 1] + c[:, 2]
    total = called + c[:, 3]
    alt = c[:, 1] + 2 * c[:, 2]
    minor = np.minimum(alt, 2 * called - alt)
    rate, maf = np.float64(f32(call["min_call_rate"])), np.float64(f32(call["min_maf"]))
    some = called > 0
    return bool((some & (rate > 0) & (called.astype(np.float64) == rate * total)).any() or
                (some & (maf > 0) & (minor.astype(np.float64) == maf * (2 * called))).any())


def wps_changes(kept_counts) -> bool:
    """Two draws whose kept sites differ by one and whose words_per_sample differ."""
    return any(k + 1 in kept_counts and
               cuking_amd.words_per_sample(k) != cuking_amd.words_per_sample(k + 1)
               for k in kept_counts)
