"""Shared by the Hardy-Weinberg tests (no GPU needed): the Python restatement of the walk of
csrc/king_hwe.h -- Python floats are IEEE doubles, so it is a legal restatement and must agree
with host twin and kernel bit for bit --, an oracle in exact rational arithmetic that shares nothing
with the walk (factorials, no recurrence), and the case lists.

Rows are (hom_ref, het, hom_var); count arrays are uint32 [rows, 4] with a `missing` column the
test must ignore (filled with a pattern, so that a reader of the wrong column shows)."""
import math
from fractions import Fraction
from functools import lru_cache

import numpy as np

MAX_PEOPLE = 1 << 24
TIE = 1.0 + 2.0 ** -27
INF = float("inf")
MIN_NORMAL = 2.0 ** -1022


def hwe_both(hom_ref, het, hom_var):
    """The walk, operation by operation, once for both forms (they differ in the last two
    operations only).  Returns (p, mid-p, steps up, steps down, whether the down-walk summed a
    subnormal term)."""
    n = hom_ref + het + hom_var
    if n == 0:
        return 1.0, 1.0, 0, 0, False
    if n > MAX_PEOPLE:
        return math.nan, math.nan, 0, 0, False
    r0, c0 = float(min(hom_ref, hom_var)), float(max(hom_ref, hom_var))
    total = tail = 1.0
    t, x, hr, hc = 1.0, float(het), r0, c0
    up = down = 0
    while hr > 0.0:
        t = (t * (4.0 * hr * hc)) / ((x + 2.0) * (x + 1.0))
        x += 2.0
        hr -= 1.0
        hc -= 1.0
        up += 1
        if t == 0.0:
            break
        if not t < INF:
            return 0.0, 0.0, up, down, False
        total += t
        if t <= TIE:
            tail += t
    t, x, hr, hc = 1.0, float(het), r0, c0
    subnormal = False
    while x >= 2.0:
        t = (t * (x * (x - 1.0))) / (4.0 * (hr + 1.0) * (hc + 1.0))
        x -= 2.0
        hr += 1.0
        hc += 1.0
        down += 1
        if t == 0.0:
            break
        if not t < INF:
            return 0.0, 0.0, up, down, subnormal
        subnormal = subnormal or t < MIN_NORMAL
        total += t
        if t <= TIE:
            tail += t
    return tail / total, (tail - 0.5) / total, up, down, subnormal


def hwe_walk(hom_ref, het, hom_var, midp=False):
    """(p or mid-p, steps up, steps down, subnormal term in the down-walk)."""
    got = hwe_both(hom_ref, het, hom_var)
    return (got[1] if midp else got[0],) + got[2:]


def hwe_p(hom_ref, het, hom_var, midp=False):
    return hwe_walk(hom_ref, het, hom_var, midp)[0]


def table_terms(hom_ref, het, hom_var):
    """Exact: {hets: P(table with that many hets) / P(observed table)} over every table with the
    observed allele counts, from the closed form 2^h n! / (a! h! c!) -- no recurrence."""
    n = hom_ref + het + hom_var
    rare = 2 * min(hom_ref, hom_var) + het

    def weight(h):
        a = (rare - h) // 2
        return Fraction(2 ** h * math.factorial(n),
                        math.factorial(a) * math.factorial(h) * math.factorial(n - h - a))
    own = weight(het)
    return {h: weight(h) / own for h in range(rare % 2, min(rare, 2 * n - rare) + 1, 2)}


def hwe_p_exact(hom_ref, het, hom_var, midp=False):
    """The p-value as a Fraction (n >= 1)."""
    terms = table_terms(hom_ref, het, hom_var)
    tail = sum(t for t in terms.values() if t <= 1)
    if midp:
        tail -= Fraction(1, 2)
    return tail / sum(terms.values())


# ---- case lists ------------------------------------------------------------------------------
SMALL_N = 24


@lru_cache(maxsize=None)
def small_tables():
    """Every (hom_ref, het, hom_var) with n <= SMALL_N: 2925 rows."""
    return tuple((a, h, n - a - h) for n in range(SMALL_N + 1) for a in range(n + 1)
                 for h in range(n - a + 1))


# Wigginton, Cutler and Abecasis (2005), the worked example: 100 people, 21 copies of the rare
# allele; p-values as printed there (six decimals).
WIGGINTON = (((83, 13, 4), 0.010293), ((81, 17, 2), 0.284042), ((80, 19, 1), 1.0))

SUBNORMAL_ROW = (40000, 45000, 15000)   # (its down-walk decays through the subnormals to 0)
# (row, what it is there for)
EDGE_ROWS = (
    ((0, 0, 0), "n = 0"),
    ((0, 1, 0), "one het"),
    ((0, 1000, 0), "all het"),
    ((0, 1001, 0), "all het, odd"),
    ((700, 0, 300), "all hom"),
    ((1000, 0, 0), "monomorphic"),
    ((0, 0, 1000), "monomorphic, the other allele"),
    ((900, 100, 0), "r0 = 0: no up-walk"),
    ((0, 100, 900), "r0 = 0, mirrored"),
    ((950, 47, 3), "odd rare copies (53)"),
    ((950, 48, 2), "even rare copies (52)"),
    ((3, 47, 950), "hom_var is the common class"),
    ((MAX_PEOPLE, 0, 0), "n = 2^24, monomorphic"),
    ((MAX_PEOPLE // 2, MAX_PEOPLE // 2, 0), "n = 2^24, r0 = 0: the down-walk overflows"),
    ((MAX_PEOPLE // 4, MAX_PEOPLE // 2, MAX_PEOPLE // 4), "n = 2^24 at equilibrium"),
    ((MAX_PEOPLE - 3000, 2990, 10), "n = 2^24, a rare allele"),
    ((MAX_PEOPLE, 1, 0), "n = 2^24 + 1: NaN"),
    ((0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), "n far above 2^24: NaN, no uint32 wrap"),
    ((8_000_000, 100, 8_000_000), "0.0 through the inf rule"),
    (SUBNORMAL_ROW, "down-walk ends in subnormals"),
    ((15000, 45000, 40000), "the same, mirrored"),
)

FUZZ_ROWS, FUZZ_SEED = 2000, 20221


@lru_cache(maxsize=None)
def fuzz_tables():
    """2000 seeded rows: n log-uniform in [1, 2^24], the het share uniform in [0, 1], the
    homozygotes split uniformly."""
    rng = np.random.default_rng(FUZZ_SEED)
    rows = []
    for _ in range(FUZZ_ROWS):
        n = min(MAX_PEOPLE, int(2.0 ** rng.uniform(0.0, 24.0)))
        het = int(round(rng.uniform(0.0, 1.0) * n))
        ref = int(round(rng.uniform(0.0, 1.0) * (n - het)))
        rows.append((ref, het, n - het - ref))
    return tuple(rows)


NEAR_ROWS, NEAR_SEED = 300, 20222


@lru_cache(maxsize=None)
def near_equilibrium_tables():
    """300 seeded rows drawn from Hardy-Weinberg proportions (n log-uniform up to 2^20, allele
    frequency log-uniform in [1e-4, 0.5]): the rows whose p-values are not 0 or 1, with ties,
    long two-sided walks and rare alleles."""
    rng = np.random.default_rng(NEAR_SEED)
    rows = []
    for _ in range(NEAR_ROWS):
        n = int(2.0 ** rng.uniform(3.0, 20.0))
        q = 10.0 ** rng.uniform(-4.0, math.log10(0.5))
        ref, het, var = rng.multinomial(n, [(1 - q) ** 2, 2 * q * (1 - q), q * q])
        rows.append((int(ref), int(het), int(var)) if rng.random() < 0.5
                    else (int(var), int(het), int(ref)))
    return tuple(rows)


@lru_cache(maxsize=None)
def all_tables():
    """Every case, one list (about 5250 rows): small tables, the paper's, the edge rows, both
    fuzzes."""
    return (small_tables() + tuple(r for r, _ in WIGGINTON) + tuple(r for r, _ in EDGE_ROWS) +
            fuzz_tables() + near_equilibrium_tables())


def counts_array(rows):
    """uint32 [len(rows), 4]: the rows and a `missing` column nobody may read."""
    out = np.empty((len(rows), 4), dtype=np.uint32)
    out[:, :3] = np.asarray(rows, dtype=np.uint64).astype(np.uint32)
    out[:, 3] = (np.arange(len(rows), dtype=np.uint64) * 2654435761 % (1 << 32)).astype(np.uint32)
    return out


@lru_cache(maxsize=None)
def _expected_both():
    got = np.array([hwe_both(*row)[:2] for row in all_tables()], dtype=np.float64)
    got.setflags(write=False)
    return got


def expected(midp):
    """The restatement on all_tables(), float64 [rows]: computed once, shared, read-only."""
    return _expected_both()[:, 1 if midp else 0]


def bits(p):
    """float64 -> its uint64 bits, for bytewise comparison (NaN included)."""
    return np.ascontiguousarray(p, dtype=np.float64).view(np.uint64)
