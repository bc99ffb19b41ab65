"""The cases of the PI_HAT sweep (fuzz_cases.run_pihat, tools/fuzz_pihat.py): the PI_HAT scan
among the other pair calls -- counts, KING records, kinship matrix or relative counts -- over one
bitset, at drawn shapes, blocks, models, thresholds, variants and launch shapes.  No GPU and no
test of its own: tests/test_pihat_fuzz_cases.py holds the committed seeds to the conditions the
sweep rests on, from this generator, the CPU oracle and the numpy restatement of
tests/pihat_cases.py alone.

Everything the runner compares is compared on bytes: the pair math is one sequence of IEEE
double operations (csrc/king_pihat.h), restated in numpy doubles (pihat_cases.z_of_counts_np)
over the IBS counts of ONE pyoracle.all_pairs call.

Size classes, each the smallest shapes at which these kernels can go wrong:
  "small"  n 2 .. 700, sites 1 .. 2500, every block of split_factor 1 .. 3; a quarter of the cases
           have sites 8000 .. 30000 and "split_wgs" from (3, 6, 16): remainder pieces of the k loop
           (the SPLIT instantiations) at drawn tile counts.
  "edges"  n one off 128, 256, 384, 512 (the tile of variants 5 and 6; the 256-sample tile whose
           quadrants variant 7 runs), the whole cohort as one block; sites one off the multiples of
           64 (a plane word) and of K_STEP_SITES.
  "tiles"  n 1400 .. 2300 (launches of >= 64 tiles: the XCD-aware order), sites 1 .. 600.

The cohort of a case: conftest.random_genotypes at a drawn missing rate, low-call samples in 30 %
of the cases, and planted rows (PLANTED): an all-missing sample (S = 0, NaN: never a record), a
sample without a het site, a duplicate pair, from 8 samples on two children of two cohort
members (one allele of each parent per site, as mendel_cases.transmit has it): parent-child pairs
and full siblings; and from 9 samples on a copy of sample 0 in which 2 % of the homozygous sites
are the opposite homozygote (IBS0 without IBS1: the way to z2 > 1, and under "negative e00" to
z0 < 0, that random pairs rarely take).

The model of a case (tag["model"]): "block" (no model=: the wrapper counts the block's stored
samples on the device), "cohort" (pi_hat_model_host of all n samples, by value), "founders"
(counts= of a drawn row range, counted on the device) or one of HAND_MODELS by name
(pihat_cases.MODELS; "negative e00" is the only way to the z0 < 0 step).  The model, the threshold
and the variant follow permutations drawn per seed, so that SPECS, THRESHOLDS and VARIANTS are all
met within len(SPECS) consecutive cases; two cases in three have a model made by hand."""
import functools
import subprocess
import tempfile
from dataclasses import dataclass
from pathlib import Path

import numpy as np

import pihat_cases as pc

SIZE_CLASSES = ("small", "edges", "tiles")
VARIANTS = (5, 6, 7)
THRESHOLDS = (-1.0, 0.0, 0.05, 0.25, 0.5, 1.0)
TIE_THRESHOLDS = (0.0, 0.5, 1.0)    # exact values of the bounded estimator: the strict > decides
HAND_MODELS = ("negative e00", "zero e00", "zero e00 and e11", "tiny e00", "NaN", "seeded rows")
SPECS = ("block", "cohort", "founders") + HAND_MODELS
CALLS = ("pi_hat", "pi_hat unbounded or bounded", "pi_hat tiles", "pi_hat count",
         "pi_hat one short", "counts", "run", "lean")
LEAN = ("kin_matrix", "relative_counts")
# king_mfma.hip: a k-step of the matrix-core kernels is 8 32-bit words per plane = 256 sites
# (kVariants' k_chunk 8; launch_mfma passes geo.k_words / 8 as a tile's steps)
K_STEP_SITES = 256
EDGE_N = tuple(e + d for e in (128, 256, 384, 512) for d in (-1, 0, 1))
EDGE_SITES = tuple(e + d for e in (64, 128, 192, 256, 320, 512, 576, 768, 1024, 1088)
                   for d in (-1, 0, 1))
# rows of the cohort that are planted (from PLANT_MIN samples on: all of them)
PLANTED = dict(duplicate_of=0, all_missing=1, no_het=2, parents=(3, 4), children=(5, 6),
               copy_with_errors=7)
PLANT_MIN = 8


def transmit(rng, father, mother):
    """A child of two int8 genotype rows: one allele of each parent per site; missing where a
    parent is."""
    from_f = np.where(father == 1, rng.integers(0, 2, size=father.shape), father // 2)
    from_m = np.where(mother == 1, rng.integers(0, 2, size=mother.shape), mother // 2)
    return np.where((father < 0) | (mother < 0), -1, from_f + from_m).astype(np.int8)


def cases(seed: int, cases: int, first_case: int = 0, size_class=None):
    """Yields (tag, geno, model_spec): the reproducer (every parameter of the case), the cohort's
    int8 [n, m] genotypes and tag["model"].  Every random number of a case is drawn before the
    `first_case` skip: a seed names the same cases whatever is skipped."""
    from conftest import random_genotypes
    from fuzz_cases import BIN_MENU, NUM_TILED_VARIANTS, THRESHOLD_MENU
    size_class = size_class or "small"
    if size_class not in SIZE_CLASSES:
        raise ValueError(f"size_class {size_class!r}: one of {SIZE_CLASSES}")
    rng = np.random.default_rng(seed)
    spec_order = [SPECS[int(k)] for k in rng.permutation(len(SPECS))]
    thr_order = [THRESHOLDS[int(k)] for k in rng.permutation(len(THRESHOLDS))]
    variant_order = [VARIANTS[int(k)] for k in rng.permutation(len(VARIANTS))]
    for case in range(cases):
        n, m = int(rng.integers(2, 701)), int(rng.integers(1, 2501))
        n_edge = int(rng.choice(EDGE_N))
        m_edge = int(rng.choice(EDGE_SITES))
        n_tiles, m_tiles = int(rng.integers(1400, 2301)), int(rng.integers(1, 601))
        # enough k-steps for remainder pieces of the matrix-core kernels' k loop
        pieces = rng.random() < 0.25
        m_long = int(rng.integers(8000, 30001))
        wgs = int(rng.choice([0, 256, 256]))
        wgs_long = int(rng.choice([3, 6, 16]))
        k = int(rng.integers(1, 4))
        u_shard = float(rng.random())
        if size_class == "edges":
            n, m, k = n_edge, m_edge, 1
        elif size_class == "tiles":
            n, m, k = n_tiles, m_tiles, 1
        elif pieces:
            m, wgs = m_long, wgs_long
        k = min(k, max(1, n // 4))           # (no empty block)
        shard = int(u_shard * (k * (k + 1) // 2))
        missing = float(rng.choice([0.0, 0.02, 0.3]))
        geno = random_genotypes(rng, n, m, missing=missing)
        low_call = rng.random() < 0.3
        who = rng.choice(n, size=max(1, n // 16), replace=False)
        thin = rng.random((len(who), m)) < 0.4
        if low_call:                 # a few low-call-rate samples (the sorted layout's case)
            geno[who] = np.where(thin, -1, geno[who])
        first = transmit(rng, geno[min(3, n - 1)], geno[min(4, n - 1)])
        second = transmit(rng, geno[min(3, n - 1)], geno[min(4, n - 1)])
        errors = rng.random(m) < 0.02
        if n >= PLANT_MIN:
            geno[5], geno[6] = first, second     # parent-child pairs, and full siblings
        if n > PLANT_MIN:
            # a copy of sample 0 with genotyping errors, opposite homozygotes: IBS0 without
            # IBS1 (z1 < 0 and z2 > 1 under a model of counts, z0 < 0 under "negative e00")
            geno[7] = np.where(errors & (geno[0] >= 0) & (geno[0] != 1), 2 - geno[0], geno[0])
        if n >= 5:
            geno[1] = -1             # nothing defined: S = 0, NaN with everybody
            geno[2] = 0              # no het site
        if n > 3:
            geno[n - 1] = geno[0]    # a duplicate pair: PI_HAT 1
        # the model, the variant and the threshold in the seed's order
        spec = spec_order[case % len(SPECS)]
        u_founders = rng.random(2).tolist()
        f0 = int(u_founders[0] * (n - 1))
        founders = [f0, min(n, f0 + 2 + int(u_founders[1] * (n - f0 - 1)))]
        turn = case + case // len(SPECS)     # (another pairing with the specs every time round)
        variant = variant_order[turn % len(VARIANTS)]
        matrix_variant = int(rng.integers(0, NUM_TILED_VARIANTS + 1))
        bounded = bool(rng.random() < 0.7)
        thr = thr_order[turn % len(THRESHOLDS)]
        w = int(rng.integers(2, 6))
        side_stream = bool(rng.random() < 0.3)
        swizzle = int(rng.integers(0, 3))
        dyn = int(rng.integers(0, 2))
        blocks = int(rng.choice([0, 0, 3, 17]))
        reuse = int(rng.integers(0, 2))
        srt, lazy = int(rng.integers(0, 3)), int(rng.integers(0, 2))
        band = int(rng.choice([0, 0, 1, 3, 5, 17]))
        count = int(rng.integers(1, 9))
        picked = rng.permutation(len(THRESHOLD_MENU))[:count]
        thresholds = sorted(THRESHOLD_MENU[int(p)] for p in picked)
        lean = LEAN[int(rng.integers(0, len(LEAN)))]
        symmetric = bool(rng.integers(0, 2))
        pad = int(rng.choice([0, 1, 37]))
        order = [CALLS[int(c)] for c in rng.permutation(len(CALLS))]
        if case < first_case:
            continue
        tag = dict(fuzzer="run_pihat", seed=seed, case=case, size_class=size_class, n=n, m=m,
                   split_factor=k, shard=shard, missing=missing, low_call=bool(low_call),
                   model=spec, founders=founders, variant=variant, bounded=bounded, thr=thr,
                   tile_ranges=w, side_stream=side_stream, order=order, lean=lean,
                   matrix_variant="stream" if matrix_variant == NUM_TILED_VARIANTS
                   else matrix_variant, thresholds=thresholds, bins=BIN_MENU[0],
                   symmetric=symmetric, out_pad=pad, xcd_swizzle=swizzle, band_rows=band,
                   split_wgs=wgs, dyn_tail_tiles=dyn, max_launch_blocks=blocks,
                   reuse_prepared=reuse, filter_sort=srt, filter_lazy_codes=lazy)
        yield tag, geno, spec


def tags(seed: int, count: int, first_case: int = 0, size_class=None) -> list:
    return [tag for tag, _, _ in cases(seed, count, first_case, size_class)]


# ---- the block, its model and its reference -----------------------------------------------------
def block_of(tag):
    """(i_begin, i_end, j_begin, j_end) of the case's block."""
    from oracle import pyoracle
    return pyoracle.submatrix(tag["n"], tag["split_factor"], tag["shard"]).as_tuple()


def holds(block, i, j) -> bool:
    """The pair (i, j), i < j, is one of the block's."""
    return block[0] <= i < block[1] and block[2] <= j < block[3]


def planted_pairs(tag) -> dict:
    """What the block holds of the planted rows: {"all_missing", "parent_child", "duplicate",
    "siblings"} -> bool."""
    n, block = tag["n"], block_of(tag)
    a = PLANTED["all_missing"]
    out = dict(all_missing=n >= 5 and (block[0] <= a < block[1] or block[2] <= a < block[3])
               and (block[1] - block[0]) + (block[3] - block[2]) > 1,
               duplicate=n > 3 and holds(block, PLANTED["duplicate_of"], n - 1),
               parent_child=False, siblings=False)
    if n >= PLANT_MIN:
        out["parent_child"] = any(holds(block, p, c) for p in PLANTED["parents"]
                                  for c in PLANTED["children"])
        out["siblings"] = holds(block, *PLANTED["children"])
    return out


def host_bits(geno) -> np.ndarray:
    """The host bitset of genotype rows, through the oracle's packer."""
    from oracle import pyoracle
    return pyoracle.bitset_from_genotypes(np.ascontiguousarray(geno))


@functools.lru_cache(maxsize=None)
def hand_model(name):
    from cuking_amd.pihat import PiHatModel
    return PiHatModel(*pc.MODELS[name]())


def model_rows(tag, geno):
    """The genotype rows the case's model counts: None for a model made by hand."""
    spec = tag["model"]
    if spec == "block":
        b = block_of(tag)
        idx = list(range(b[0], b[1])) + (list(range(b[2], b[3])) if b[0] != b[2] else [])
        return geno[idx]
    if spec == "cohort":
        return geno
    if spec == "founders":
        return geno[tag["founders"][0]:tag["founders"][1]]
    return None


def model_of(tag, geno):
    """The case's PiHatModel, on the host: pi_hat_model_host of the rows' counts (tests/
    test_pihat_host.py holds it to the restatement bit for bit), or the model made by hand."""
    import cuking_amd
    rows = model_rows(tag, geno)
    if rows is None:
        return hand_model(tag["model"])
    bits = host_bits(rows)
    counts = cuking_amd.pihat.site_counts_of_host_bits(bits, bits.shape[1])
    return cuking_amd.pi_hat_model_host(counts, tag["m"])


@dataclass
class Reference:
    osm: object           # the oracle's block
    bits: np.ndarray      # uint64 [stored samples, wps]
    all_pairs: tuple      # (i, j, counts, kin) of ONE pyoracle.all_pairs call
    ibs: tuple            # (ibs0, ibs1, ibs2) of ibs_of_counts
    records: dict         # (threshold, bounded) -> records_np, for the case's threshold and -1.0
    taken: dict           # bounding step -> pairs of the block that take it (pihat_cases.BRANCHES)
    ties: int             # pairs whose float32 PI_HAT (the case's `bounded`) equals the threshold


def reference(tag, geno, model, defect=None, oracle=None) -> Reference:
    """Everything the runner compares against, from ONE pyoracle.all_pairs call (`oracle`: an
    earlier reference of the same case, whose call is then used again; `defect`: one of
    pihat_cases.DEFECTS)."""
    import cuking_amd
    from oracle import pyoracle
    model = model.as_tuple() if hasattr(model, "as_tuple") else tuple(model)
    if oracle is not None:
        osm, bits, every = oracle.osm, oracle.bits, oracle.all_pairs
    else:
        osm = pyoracle.submatrix(tag["n"], tag["split_factor"], tag["shard"])
        bits = pyoracle.bitset_from_genotypes(geno, osm)
        every = pyoracle.all_pairs(osm, bits)
    oi, oj, oc, _ = every
    ibs = pc.ibs_of_counts(oc, defect=defect)
    sm = cuking_amd.Submatrix(tag["n"], tag["split_factor"], tag["shard"])
    assert sm.as_tuple() == osm.as_tuple() and len(oi) == sm.NumPairs()
    records, taken, ties = {}, {}, 0
    for bounded in (True, False):
        pi_hat = pc.z_of_counts_np(model, *ibs, bounded, taken=taken if bounded else None,
                                   defect=defect)[3]
        for thr in sorted({tag["thr"], -1.0}):
            records[(thr, bounded)] = pc.records_of_pi_hat(oi, oj, *ibs, pi_hat, thr, defect)
        if bounded == tag["bounded"]:
            with np.errstate(over="ignore", invalid="ignore"):
                ties = int((pi_hat.astype(np.float32) == np.float32(tag["thr"])).sum())
    return Reference(osm, bits, every, ibs, records, taken, ties)


# ---- which calls launch remainder pieces --------------------------------------------------------
ROOT = Path(__file__).resolve().parent.parent
_SCRATCH = []


@functools.lru_cache(maxsize=None)
def _plan_driver() -> str:
    """tests/launch_plan_driver.cc built by the host compiler against king_launch_plan.h."""
    _SCRATCH.append(tempfile.TemporaryDirectory(prefix="launch_plan_"))
    exe = Path(_SCRATCH[-1].name) / "launch_plan_driver"
    subprocess.run(["g++", "-std=c++17", "-O2", f"-I{ROOT / 'cuking_amd' / 'csrc'}",
                    str(ROOT / "tests" / "launch_plan_driver.cc"), "-o", str(exe)], check=True)
    return str(exe)


def mfma_plans(queries) -> list:
    """mfma_plan (king_launch_plan.h) of (tiles, wgs, cap, steps) tuples: (first, split_whole,
    split_tiles) each."""
    queries = list(queries)
    if not queries:
        return []
    words = [str(int(x)) for q in queries for x in q]
    out = subprocess.run([_plan_driver(), "--mfma", *words], check=True, capture_output=True,
                         text=True).stdout.split()
    assert len(out) == 3 * len(queries)
    return [tuple(int(x) for x in out[3 * k:3 * k + 3]) for k in range(len(queries))]


def num_tiles(tag) -> int:
    """The tiles of the case's block in the enumeration of its variant (KingContext.num_tiles)."""
    b = block_of(tag)
    edge = 256 if tag["variant"] == 7 else 128
    tiles_r, tiles_c = -(-(b[1] - b[0]) // edge), -(-(b[3] - b[2]) // edge)
    return tiles_r * (tiles_r + 1) // 2 if b[0] == b[2] else tiles_r * tiles_c


def plan_queries(tag) -> list:
    """The mfma_plan inputs of the case's PI_HAT launches: the whole block, then the ranges of
    tile_partition (variant 7 runs the four-product kernel on the quadrants of its tiles)."""
    import cuking_amd
    from cuking_amd.dist import tile_partition
    tiles, per_tile = num_tiles(tag), 4 if tag["variant"] == 7 else 1
    steps = -(-cuking_amd.words_per_sample(tag["m"]) // 8)
    ranges = [(0, tiles)] + [r for r in tile_partition(tiles, tag["tile_ranges"])]
    return [((end - begin) * per_tile, tag["split_wgs"], tag["max_launch_blocks"], steps)
            for begin, end in ranges if end > begin]


def split_launches(tags_of_sweep) -> list:
    """Per case, the number of its PI_HAT launches (plan_queries) whose plan has remainder pieces:
    the SPLIT instantiations of king_mfma_kernel."""
    queries = [plan_queries(tag) for tag in tags_of_sweep]
    plans = iter(mfma_plans(q for case in queries for q in case))
    return [sum(next(plans)[2] != 0 for _ in case) for case in queries]
