"""Mendelian errors of trios and duos: the cases the host and the GPU tests share, a seeded fuzz
and the naive reference -- a walk over the sites one by one on genotype arrays, which classifies
a (father, mother, child) genotype by the table of include/cuking_amd.h "Mendelian errors" as it is
written there and knows nothing of words or bit masks.

Genotype codes are those of the bitset: 0 hom-ref, 1 het, 2 hom-var, 3 missing.  An absent parent
(``NO_PARENT``, or an index at or beyond the stored samples) reads as missing everywhere.
"""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from roh_cases import pack_codes

from cuking_amd import mendel
from cuking_amd.mendel import MENDEL_TRIO_DTYPE, NO_PARENT

STEP = 64 * 64         # sites of one wavefront step: 64 lanes x 64 sites (king_mendel.hip)
SITE_COUNTS = {1, 63, 64, 65, 127, 128, 4095, 4096, 4097, STEP + 65}
R, H, V, MISSING = 0, 1, 2, 3

# ---- the naive reference --------------------------------------------------------------------------
# The table, row by row: code, what the father must be, what the mother must be, the child.
# ("is", X): exactly X; ("not", X): anything else, missing and absent included.
TABLE = (
    (1, ("is", R), ("is", R), H),
    (2, ("is", V), ("is", V), H),
    (3, ("is", V), ("not", V), R),
    (4, ("not", V), ("is", V), R),
    (5, ("is", V), ("is", V), R),
    (6, ("is", R), ("not", R), V),
    (7, ("not", R), ("is", R), V),
    (8, ("is", R), ("is", R), V),
)


def _holds(rule, genotype):
    return (genotype == rule[1]) == (rule[0] == "is")


def classify(father, mother, child):
    """The error code of one site, 0 for none.  At most one row of the table applies."""
    codes = [code for code, f, m, c in TABLE
             if child == c and _holds(f, father) and _holds(m, mother)]
    assert len(codes) <= 1, (father, mother, child, codes)
    return codes[0] if codes else 0


# (the 64 genotype triples once: the walk below looks a site up)
CODE_OF = [[[classify(f, m, c) for c in range(4)] for m in range(4)] for f in range(4)]


def naive(code, num_sites, trios, plane_words):
    """``(rows, error_bits, site_counts)`` of the listed trios over the sites ``0 .. num_sites -
    1`` of ``code`` (uint8 ``[samples, >= num_sites]``), site by site."""
    n = code.shape[0]
    rows = np.zeros(len(trios), dtype=MENDEL_TRIO_DTYPE)
    mask = np.zeros((len(trios), plane_words), dtype=np.uint64)
    counts = np.zeros(64 * plane_words, dtype=np.uint32)
    absent = [MISSING] * num_sites
    for t, (child, father, mother) in enumerate(np.asarray(trios).tolist()):
        rows[t]["child"], rows[t]["father"], rows[t]["mother"] = child, father, mother
        if child >= n:
            continue
        gc = code[child, :num_sites].tolist()
        gf = code[father, :num_sites].tolist() if father < n else absent
        gm = code[mother, :num_sites].tolist() if mother < n else absent
        errors = [0] * 8
        called = 0
        for s in range(num_sites):
            k = CODE_OF[gf[s]][gm[s]][gc[s]]
            if k:
                errors[k - 1] += 1
                mask[t, s >> 6] |= np.uint64(1 << (s & 63))
                counts[s] += 1
            called += (gc[s] != MISSING and (father == NO_PARENT or gf[s] != MISSING) and
                       (mother == NO_PARENT or gm[s] != MISSING))
        rows[t]["called"] = called
        rows[t]["errors"] = errors
    return rows, mask, counts


# ---- inputs --------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    """``kind``: "random" (independent genotypes, every shape of trio), "rows" (random, with
    sample 1 missing everywhere and sample 2 het everywhere), "family" (children draw one allele
    from each parent: no error) or "planted" (the family with errors of every code planted at
    ``planted_sites``).  ``extra``: plane words beyond ceil(sites / 64)."""
    name: str
    samples: int
    sites: int
    kind: str = "random"
    trios: int = 20
    extra: int = 0
    seed: int = 0


@dataclass
class Inputs:
    case: Case
    code: np.ndarray        # uint8 [samples, sites]
    trios: np.ndarray       # uint32 [T, 3]
    plane: int

    wps = property(lambda self: 2 * self.plane)

    def bits(self, ones_padding=False):
        return pack_codes(self.code, self.plane, ones_padding)


def draw_codes(rng, samples, sites, p=(0.36, 0.3, 0.26, 0.08)):
    return rng.choice(4, size=(samples, sites), p=p).astype(np.uint8)


def trio_list(rng, n, count):
    """Every shape of trio on ``n`` stored samples, then random ones, ``count`` in all: full
    trios, two children sharing parents, father-only and mother-only duos, no parent, a repeat, a
    parent and a child at or beyond the stored samples, a child that is its own parent."""
    k = lambda x: x % n   # noqa: E731
    fixed = [(k(0), k(1), k(2)), (k(3), k(1), k(2)), (k(0), k(1), NO_PARENT),
             (k(0), NO_PARENT, k(2)), (k(4), NO_PARENT, NO_PARENT), (k(0), k(1), k(2)),
             (k(5), n + 3, k(2)), (k(5), k(1), n), (n + 1, k(1), k(2)), (n, NO_PARENT, k(2)),
             (k(2), k(2), k(1)), (k(1), k(1), k(1)), (k(3), NO_PARENT, k(1)),
             (k(3), k(2), NO_PARENT)]
    out = fixed[:count]
    while len(out) < count:
        who = rng.integers(0, n + 2, size=3).tolist()
        for column in (1, 2):
            if rng.random() < 0.25:
                who[column] = NO_PARENT
        out.append(tuple(who))
    return np.array(out, dtype=np.uint32).reshape(-1, 3)


# The family: founders 0 .. 5, children 6 and 7 of (0, 1), 8 of (2, 3); 9 .. are unrelated.
FAMILY_SAMPLES = 12
FAMILY_TRIOS = np.array([(8, 2, 3), (6, 0, 1), (7, 0, 1), (8, 2, NO_PARENT), (8, NO_PARENT, 3),
                         (6, 0, NO_PARENT), (7, NO_PARENT, 1)], dtype=np.uint32)
PLANTED_TRIO = 0           # (8, 2, 3): the one the errors are planted into; 8 is their only child
# genotypes (father, mother, child) that give code k + 1
PLANT_GENOTYPES = ((R, R, H), (V, V, H), (V, R, R), (H, V, R), (V, V, R), (R, H, V), (H, R, V),
                   (R, R, V))


def transmit(rng, father, mother):
    """A child of two genotype rows (no missing): one allele of each parent per site."""
    from_f = np.where(father == H, rng.integers(0, 2, size=father.shape), father // 2)
    from_m = np.where(mother == H, rng.integers(0, 2, size=mother.shape), mother // 2)
    return (from_f + from_m).astype(np.uint8)


def planted_sites(case):
    """``{site: code}``: word and step edges first, one code after the other."""
    m = case.sites
    sites = [s for s in (0, 63, 64, 127, 128, 4095, 4096, m - 1, 1, 62, 65, 126, 4094, 4097,
                         STEP + 63, STEP + 64, m - 2, 200, 300, 1000, 2000, 3000, 3001, 3500)
             if 0 <= s < m]
    sites = list(dict.fromkeys(sites))
    return {s: 1 + i % 8 for i, s in enumerate(sites)}


@lru_cache(maxsize=None)
def inputs(case: Case) -> Inputs:
    rng = np.random.default_rng([case.seed, case.samples, case.sites, len(case.kind)])
    n, m = case.samples, case.sites
    plane = -(-m // 64) + case.extra
    if case.kind in ("random", "rows"):
        code = draw_codes(rng, n, m)
        if case.kind == "rows":
            code[1 % n, :] = MISSING
            code[2 % n, :] = H
        trios = trio_list(rng, n, case.trios)
    else:
        assert n == FAMILY_SAMPLES
        code = draw_codes(rng, n, m, p=(0.4, 0.35, 0.25, 0.0))
        for child, father, mother in ((6, 0, 1), (7, 0, 1), (8, 2, 3)):
            code[child] = transmit(rng, code[father], code[mother])
        if case.kind == "planted":
            child, father, mother = FAMILY_TRIOS[PLANTED_TRIO].tolist()
            for site, k in planted_sites(case).items():
                code[father, site], code[mother, site], code[child, site] = PLANT_GENOTYPES[k - 1]
        # missing calls afterwards, away from the planted sites: they hide errors, never make one
        gaps = rng.random(code.shape) < 0.03
        gaps[:, list(planted_sites(case))] = False
        code[gaps] = MISSING
        trios = FAMILY_TRIOS
    return Inputs(case, code, trios, plane)


@lru_cache(maxsize=None)
def reference(case: Case):
    inp = inputs(case)
    return naive(inp.code, case.sites, inp.trios, inp.plane)


def run_host(case: Case, ones_padding=False):
    """``(rows, error_bits, site_counts)`` of the host twin."""
    inp = inputs(case)
    rows, mask = mendel.mendel_errors_raw_host(inp.bits(ones_padding), inp.wps, case.sites,
                                               inp.trios, error_bits=True)
    return rows, mask, mendel.site_counts_host(mask)


def check_against(case: Case, rows, mask, counts, what="rows"):
    want = reference(case)
    assert rows.dtype == MENDEL_TRIO_DTYPE
    assert rows.tobytes() == want[0].tobytes(), (case.name, what, rows, want[0])
    assert np.asarray(mask).tobytes() == want[1].tobytes(), (case.name, what, "error_bits")
    assert np.asarray(counts).tobytes() == want[2].tobytes(), (case.name, what, "site counts")


CASES = [Case(f"random, {m} sites", 8 + (m % 7), m, seed=m) for m in sorted(SITE_COUNTS)] + [
    Case("24 samples, 20 trios", 24, 700, seed=1),
    Case("one sample", 1, 130, trios=14, seed=2),
    Case("two samples", 2, 65, trios=14, seed=3),
    Case("no trio", 5, 100, trios=0),
    Case("one trio", 5, 4097, trios=1, seed=4),
    Case("five trios: two workgroups", 9, 200, trios=5, seed=5),
    Case("spare plane words", 7, 130, extra=3, seed=6),
    Case("64 sites and a spare word", 7, 64, extra=1, seed=7),
    Case("a step and a spare word", 7, STEP, extra=1, seed=8),
    Case("all-missing and all-het rows", 6, 300, kind="rows", seed=9),
    Case("all-missing and all-het rows, a step", 6, STEP + 65, kind="rows", seed=10),
    Case("family, 1 site", FAMILY_SAMPLES, 1, kind="family", seed=11),
    Case("family, 700 sites", FAMILY_SAMPLES, 700, kind="family", seed=12),
    Case("family, a step and 65", FAMILY_SAMPLES, STEP + 65, kind="family", seed=13),
    Case("planted, 129 sites", FAMILY_SAMPLES, 129, kind="planted", seed=12),
    Case("planted, 4097 sites", FAMILY_SAMPLES, 4097, kind="planted", seed=14),
    Case("planted, a step and 65", FAMILY_SAMPLES, STEP + 65, kind="planted", seed=13),
]

FUZZ_SEEDS = range(30)


def fuzz_case(seed: int) -> Case:
    rng = np.random.default_rng(1000 + seed)
    edges = sorted(SITE_COUNTS) + [2, 62, 66, 129, 191, 192, 193]
    sites = int(rng.choice(edges)) if rng.random() < 0.5 else int(rng.integers(1, 4300))
    kind = str(rng.choice(["random", "random", "rows", "planted"]))
    samples = FAMILY_SAMPLES if kind == "planted" else int(rng.integers(1, 25))
    return Case(f"fuzz {seed}", samples, sites, kind, trios=int(rng.integers(0, 21)),
                extra=int(rng.choice([0, 0, 1, 3])), seed=2000 + seed)


def form_counts(cases):
    """Errors per code of the cases' references by the form of the trio: ``(full, father_duo,
    mother_duo)``, int64 ``[8]`` each.  Full: both parents stored; a duo: the other one absent."""
    sums = np.zeros((3, 8), dtype=np.int64)
    for case in cases:
        n = case.samples
        for row in reference(case)[0]:
            has_f, has_m = row["father"] < n, row["mother"] < n
            if has_f or has_m:
                sums[0 if has_f and has_m else 1 if has_f else 2] += row["errors"]
    return sums


# ---- the raw calls -------------------------------------------------------------------------------
REFUSAL_CASE = Case("refusals", 6, 180, trios=4, seed=21)
# name -> (arguments replaced, a word of the message)
TRIO_REFUSALS = {
    "wps odd": (dict(wps=5), "positive even"),
    "wps zero": (dict(wps=0), "positive even"),
    "too many sites": (dict(num_sites=193), "do not fit"),
    "null out": (dict(out=None), "null out"),
    "null trios": (dict(trios=None), "null trios"),
    "null bits": (dict(bits=None), "null bits"),
}
SITE_REFUSALS = {
    "no plane word": (dict(plane=0), "at least one word"),
    "2^32 trios": (dict(num_trios=1 << 32), "32 bits"),
    "null mask": (dict(error_bits=None), "null pointer"),
    "null counts": (dict(counts=None), "null pointer"),
}


def trio_arguments(inp, pointers, **over):
    """The argument list of cuking_mendel_trios_host (the device call adds ctx and stream around
    it), single ones replaced."""
    a = dict(bits=pointers["bits"], num_stored=inp.case.samples, wps=inp.wps,
             num_sites=inp.case.sites, trios=pointers["trios"], num_trios=len(inp.trios),
             out=pointers["out"], error_bits=pointers["error_bits"])
    a.update(over)
    return [a[k] for k in ("bits", "num_stored", "wps", "num_sites", "trios", "num_trios", "out",
                           "error_bits")]


def site_arguments(inp, pointers, **over):
    """The argument list of cuking_mendel_site_counts_host, single ones replaced."""
    a = dict(error_bits=pointers["error_bits"], num_trios=len(inp.trios), plane=inp.plane,
             counts=pointers["counts"])
    a.update(over)
    return [a[k] for k in ("error_bits", "num_trios", "plane", "counts")]


# ---- end to end ----------------------------------------------------------------------------------
E2E_FAMILIES, E2E_SITES, E2E_SEED = 6, 5000, 3


def e2e_cohort(seed=E2E_SEED):
    """60 samples x 5000 sites: six families of two founders and three children (30 samples),
    then 30 unrelated samples; 1 % missing.  Returns ``(geno int8 [60, 5000] with -1 for
    missing, true trios [18, 3])`` -- the trios as ``candidate_trios`` would give them, the
    lower-numbered parent in the father column."""
    rng = np.random.default_rng(seed)
    n, m = 60, E2E_SITES
    freq = rng.uniform(0.1, 0.5, size=m)
    code = (rng.random((n, m)) < freq).astype(np.uint8) + (rng.random((n, m)) < freq)
    trios = []
    for family in range(E2E_FAMILIES):
        a, b = 5 * family, 5 * family + 1
        for child in range(5 * family + 2, 5 * family + 5):
            code[child] = transmit(rng, code[a], code[b])
            trios.append((child, a, b))
    geno = code.astype(np.int8)
    geno[rng.random((n, m)) < 0.01] = -1
    return geno, np.array(trios, dtype=np.uint32)
