"""The cases of the site-order sweep (fuzz_cases.run_site_order, tools/fuzz_site_order.py): the
filter variant with "filter_site_order" on, over shapes, blocks of a split, thresholds, forms,
gather forms, everything run_general draws for the filter, and three to six calls in a random
order over one bitset -- without a context, so that tests/test_site_order_cases.py can hold the
committed seeds to the conditions the sweep rests on from the generator and the oracle alone.

Also here, once: where prepare() (king_abi.hip) must have ordered the layout (`expected_flag`),
and the records of any threshold from ONE oracle.all_pairs call (`records_of`)."""
import numpy as np

MENU = (0.0442, 0.0884, 0.177, 0.354)      # thresholds the filter runs for
OUTSIDE = (-0.2, 0.0, 0.5)                 # ... and does not: the order must stay off
KINDS = ("run", "run2", "tile_ranges", "relative_counts", "kin_matrix", "staged")
WHOLE = ("run", "run2", "relative_counts")  # whole-block calls that convert for the filter
GATHERS = (-1, 0, 2, 4)
MAX_PLANE_WORDS = 4096                     # (king_sort.hip site_order_scratch)
K_STEP_SITES = 256
# what the runner sets besides fuzz_cases.SHIPPED, and the shipped values it restores
SHIPPED = dict(filter_site_order=-1, filter_site_gather=-1, filter_site_order_min_tiles=24576)


def site_order_cases(seed: int, cases: int, first_case: int = 0):
    """Yields (tag, geno): the reproducer (every parameter of the case) and the cohort's int8
    [n, m] genotypes.  Every random number of a case is drawn before the `first_case` skip: a
    seed names the same cases whatever is skipped."""
    from conftest import random_genotypes
    from oracle import pyoracle
    rng = np.random.default_rng(seed)
    for case in range(cases):
        n = int(rng.integers(2, 700))
        n_tiles = int(rng.integers(1400, 2300))    # launches of >= 64 tiles
        n_tiny = int(rng.integers(2, 4))           # two or three stored samples
        size = rng.random()
        m_mid, m_short, m_long = (int(rng.integers(1024, 6000)), int(rng.integers(1, 1024)),
                                  int(rng.integers(6000, 24000)))
        m_tiny = int(rng.integers(1, 256))         # shorter than one k-step
        length, tiny_m = rng.random(), rng.random() < 0.25
        k = int(rng.integers(1, 4))
        shard = int(rng.integers(0, k * (k + 1) // 2))
        thr = float(rng.choice(MENU)) if rng.random() < 0.92 else float(rng.choice(OUTSIDE))
        thr2 = float(rng.choice(MENU))
        mode = 0 if rng.random() < 0.85 else int(rng.choice([-1, 1]))
        order = int(rng.choice([1, 1, 2, -1]))
        gather = int(rng.choice(GATHERS))
        m = m_mid if length < 0.5 else (m_tiny if tiny_m else m_short) if length < 0.8 else m_long
        if size < 0.15:
            # (the oracle lists every pair: two million of them are served at moderate lengths)
            n, m = n_tiles, m if m < 6000 else m_mid
        elif size < 0.21:
            n = n_tiny
        if n < 2 * k:                              # every block holds a pair
            k, shard = 1, 0
        # everything run_general draws for the filter
        qcap = int(rng.choice([384, 384, 0, 2]))
        ccap = int(rng.choice([1 << 20, 1 << 20, 0, 5]))
        wgs = int(rng.choice([0, 256, 256]))
        smin = int(rng.choice([8, 1, 1]))
        chk0 = int(rng.choice([1, 0, 2, 2]))
        chk1 = int(rng.choice([1, 0, 3, 5, 7, 9]))
        srt, lazy = int(rng.integers(0, 3)), int(rng.integers(0, 2))
        emit = int(rng.choice([64, 64, 0, 1, 255]))
        rot = int(rng.choice([1, 0, 2, 2, 3 + int(rng.integers(0, 64))]))
        reuse = int(rng.integers(0, 2))
        side_stream = bool(rng.random() < 0.3)
        # the cohort: spread allele frequencies, missing calls, monomorphic sites, low-call
        # samples, an all-missing sample, a duplicate inside the block
        missing = float(rng.choice([0.0, 0.02, 0.3]))
        mono_share = float(rng.choice([0.0, 0.3]))
        geno = random_genotypes(rng, n, m, missing=missing)
        mono = rng.random(m) < mono_share
        geno[:, mono] = np.where(geno[:, mono] < 0, -1, 0)
        low_call = bool(rng.random() < 0.3)
        who = rng.choice(n, size=max(1, n // 16), replace=False)
        thin = rng.random((len(who), m)) < 0.4
        all_missing = bool(rng.random() < 0.3)
        if n > 3:
            if low_call:
                geno[who] = np.where(thin, -1, geno[who])
            if all_missing:
                geno[1] = -1
        i0, _, _, j1 = pyoracle.submatrix(n, k, shard).as_tuple()
        geno[j1 - 1] = geno[i0]                    # the block's first row and last column
        # the calls
        pool = [kind for kind in KINDS if kind != "staged" or k == 1]
        picked = [pool[int(c)] for c in rng.permutation(len(pool))]
        calls = picked[:int(rng.integers(3, 7))]
        if not set(calls) & set(WHOLE):
            calls[0] = "run"
        w = int(rng.integers(2, 6))
        world, chunks = int(rng.integers(1, 5)), int(rng.integers(1, 6))
        streams = [int(rng.integers(1, 4)) for _ in range(4)][:world]
        bands = int(rng.integers(1, 5))
        thresholds = [thr] + [t for t in MENU if t > thr][:bands - 1]
        if case < first_case:
            continue
        tag = dict(fuzzer="run_site_order", seed=seed, case=case, n=n, m=m, split_factor=k,
                   shard=shard, thr=thr, thr2=thr2, thresholds=thresholds, counts_mode=mode,
                   filter_site_order=order, filter_site_gather=gather, missing=missing,
                   monomorphic=mono_share, low_call=low_call, all_missing=all_missing,
                   calls=calls, tile_ranges=w, world=world, chunks=chunks, streams=streams,
                   side_stream=side_stream, split_wgs=wgs, reuse_prepared=reuse,
                   filter_quadrant_cap=qcap, filter_cand_cap=ccap, filter_split_min_steps=smin,
                   filter_check0=chk0, filter_check1=chk1, filter_check_min_steps=4,
                   filter_sort=srt, filter_lazy_codes=lazy, filter_check_emit=emit,
                   filter_rotate=rot, filter_rotate_min_steps=4, filter_rotate_min_tiles=0,
                   filter_site_order_min_tiles=0)
        yield tag, geno


def site_order_tags(seed: int, cases: int, first_case: int = 0) -> list:
    return [tag for tag, _ in site_order_cases(seed, cases, first_case)]


def site_order_oracle(tag, geno):
    """(oracle block, its bitset, ONE all_pairs call) of a case."""
    from oracle import pyoracle
    osm = pyoracle.submatrix(tag["n"], tag["split_factor"], tag["shard"])
    bits = pyoracle.bitset_from_genotypes(geno, osm)
    return osm, bits, pyoracle.all_pairs(osm, bits)


def records_of(all_pairs, thr):
    """The records pyoracle.compute gives at `thr`, from the all_pairs result: the pairs with
    kin > thr (strict, float32), in (i, j) order (king_oracle.c fill_result)."""
    from oracle import pyoracle
    oi, oj, counts, kin = all_pairs
    with np.errstate(invalid="ignore"):
        keep = kin > np.float32(thr)
    out = np.zeros(int(keep.sum()), dtype=pyoracle.RESULT_DTYPE)
    c = counts[keep]
    out["sample_i"], out["sample_j"], out["kin"] = oi[keep], oj[keep], kin[keep]
    out["ibs0"] = c["opposing_hom"]
    out["ibs2"] = c["concordant_hom"] + c["both_het"]
    out["ibs1"] = c["shared"] - out["ibs0"] - out["ibs2"]
    return out


def stored_samples(tag) -> int:
    from oracle import pyoracle
    i0, i1, j0, j1 = pyoracle.submatrix(tag["n"], tag["split_factor"], tag["shard"]).as_tuple()
    return i1 - i0 if i0 == j0 else (i1 - i0) + (j1 - j0)


def expected_flag(tag, kind, thr):
    """"site_order_on" behind a whole-block call of `kind` at `thr`, where prepare() makes it
    plain: 0 where the filter does not run (a threshold outside (0, 1/2); the record call's
    full form), 1 where it runs and the option is 1 or 2, on at least 2 stored samples and at
    most 4,096 plane words.  None where a rule decides that the sweep only records: the
    automatic option, and the automatic choice of the form (relative_counts always counts in
    the lean form)."""
    assert kind in WHOLE
    if not 0.0 < thr < 0.5:
        return 0
    if kind != "relative_counts" and tag["counts_mode"] != 0:
        return 0 if tag["counts_mode"] == 1 else None
    if tag["filter_site_order"] == -1:
        return None
    plane_words = (tag["m"] + 63) // 64
    return int(stored_samples(tag) >= 2 and plane_words <= MAX_PLANE_WORDS)


def call_threshold(tag, kind):
    return tag["thr2"] if kind == "run2" else tag["thr"]


def expects_order(tag) -> bool:
    """A case one of whose whole-block calls must leave an ordered layout."""
    return any(expected_flag(tag, kind, call_threshold(tag, kind)) == 1
               for kind in tag["calls"] if kind in WHOLE)
