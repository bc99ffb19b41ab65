"""Cases and restatements for the PI_HAT tests (include/cuking_amd.h "PI_HAT (PLINK --genome)"):
the definition once more in Python floats, in the order csrc/king_pihat.h writes it, so that the
host twin, the kernel and this file must agree bit for bit; the same terms in exact rationals; a
per-site numpy walk that derives IBS0/1/2 from the genotypes; seeded count rows and IBS triples;
and the smoke() cohort with its planted pairs."""
import random
from fractions import Fraction
from functools import lru_cache

import numpy as np

from cuking_amd import KING_RESULT_DTYPE

MAX_PEOPLE = 1 << 24


# ---- the restatement, in Python floats (IEEE doubles, one rounding per operation) ---------------
def falling(a: float, k: int) -> float:
    p = 1.0
    for i in range(k):
        f = a - float(i)
        if f == 0.0:
            return 0.0
        p = p * f
    return p


def site_terms(r: int, h: int, v: int):
    x, y = float(h + 2 * v), float(h + 2 * r)
    n = x + y
    x1, x2, x3, x4 = (falling(x, k) for k in (1, 2, 3, 4))
    y1, y2, y3, y4 = (falling(y, k) for k in (1, 2, 3, 4))
    n3, n4 = falling(n, 3), falling(n, 4)
    x2y2, x3y1, x1y3, x2y1, x1y2 = x2 * y2, x3 * y1, x1 * y3, x2 * y1, x1 * y2
    return ((2.0 * x2y2) / n4,
            (4.0 * (x3y1 + x1y3)) / n4,
            ((x4 + y4) + 4.0 * x2y2) / n4,
            (2.0 * (x2y1 + x1y2)) / n3,
            (((x3 + y3) + x2y1) + x1y2) / n3)


def model_of_rows(rows):
    """(e00, e01, e02, e11, e12, sites_used) of count rows (r, h, v)."""
    sums, used = [0.0] * 5, 0
    for r, h, v in rows:
        assert r + h + v <= MAX_PEOPLE
        if r + h + v < 2:
            continue
        for k, t in enumerate(site_terms(r, h, v)):
            sums[k] = sums[k] + t
        used += 1
    nan = float("nan")
    # (0.0 / 0.0 raises in Python: IEEE gives NaN)
    return tuple(s / float(used) if used else nan for s in sums) + (used,)


def _div(a: float, b: float) -> float:
    """IEEE a / b, where Python raises."""
    if b == 0.0:
        if a != a or a == 0.0:
            return float("nan")
        return float("-inf") if np.signbit(a) != np.signbit(b) else float("inf")
    return a / b


def z_of_counts(model, ibs0: int, ibs1: int, ibs2: int, bounded: bool = True):
    """(z0, z1, z2, pi_hat) of a pair."""
    e00, e01, e02, e11, e12 = model[:5]
    s = (float(ibs0) + float(ibs1)) + float(ibs2)
    z0 = _div(float(ibs0), e00 * s)
    z1 = _div(float(ibs1) - z0 * (e01 * s), e11 * s)
    z2 = _div((float(ibs2) - z0 * (e02 * s)) - z1 * (e12 * s), s)
    if bounded:
        if z0 > 1.0:
            z0, z1, z2 = 1.0, 0.0, 0.0
        if z1 > 1.0:
            z0, z1, z2 = 0.0, 1.0, 0.0
        if z2 > 1.0:
            z0, z1, z2 = 0.0, 0.0, 1.0
        if z0 < 0.0:
            t = z1 + z2
            z0, z1, z2 = 0.0, _div(z1, t), _div(z2, t)
        if z1 < 0.0:
            t = z0 + z2
            z1, z0, z2 = 0.0, _div(z0, t), _div(z2, t)
        if z2 < 0.0:
            t = z0 + z1
            z2, z0, z1 = 0.0, _div(z0, t), _div(z1, t)
    return z0, z1, z2, z1 / 2.0 + z2


def pi_hat_f32(model, ibs0, ibs1, ibs2, bounded=True) -> np.float32:
    return np.float32(z_of_counts(model, ibs0, ibs1, ibs2, bounded)[3])


def bits(a) -> np.ndarray:
    """The bit patterns of doubles; every NaN as the one canonical NaN (IEEE leaves the sign and
    payload of an invalid operation's result to the implementation: x86 gives -NaN for 0 / 0)."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    return np.where(np.isnan(a), np.float64("nan"), a).view(np.uint64)


# ---- exact rationals ---------------------------------------------------------------------------
def falling_exact(a: int, k: int) -> int:
    p = 1
    for i in range(k):
        p *= a - i
    return p


def site_terms_exact(r: int, h: int, v: int):
    x, y = h + 2 * v, h + 2 * r
    n = x + y
    F = falling_exact
    n3, n4 = F(n, 3), F(n, 4)
    return (Fraction(2 * F(x, 2) * F(y, 2), n4),
            Fraction(4 * (F(x, 3) * F(y, 1) + F(x, 1) * F(y, 3)), n4),
            Fraction(F(x, 4) + F(y, 4) + 4 * F(x, 2) * F(y, 2), n4),
            Fraction(2 * (F(x, 2) * F(y, 1) + F(x, 1) * F(y, 2)), n3),
            Fraction(F(x, 3) + F(y, 3) + F(x, 2) * F(y, 1) + F(x, 1) * F(y, 2), n3))


def small_rows(max_people: int = 12):
    """Every count row (r, h, v) of 2 .. max_people people."""
    return [(r, h, n - r - h) for n in range(2, max_people + 1)
            for r in range(n + 1) for h in range(n + 1 - r)]


# ---- seeded cases ------------------------------------------------------------------------------
def seeded_count_rows(seed: int = 20240, num: int = 600):
    rng = random.Random(seed)
    rows = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (2, 0, 0), (0, 0, 2), (0, 2, 0), (1, 1, 0),
            (MAX_PEOPLE, 0, 0), (0, MAX_PEOPLE, 0), (1, 2, MAX_PEOPLE - 3),
            (MAX_PEOPLE // 2, MAX_PEOPLE // 4, MAX_PEOPLE // 4)]
    for _ in range(num):
        n = rng.choice((3, 17, 333, 5000, 100000, MAX_PEOPLE))
        n = rng.randint(0, n)
        r = rng.randint(0, n)
        h = rng.randint(0, n - r)
        rows.append((r, h, n - r - h))
    return rows


def counts_array(rows) -> np.ndarray:
    """uint32 [n, 4] as site_counts lays it out; the missing column holds junk."""
    out = np.empty((len(rows), 4), dtype=np.uint32)
    for s, (r, h, v) in enumerate(rows):
        out[s] = (r, h, v, (0xDEADBEEF + s) & 0xFFFFFFFF)
    return out


# Triples that drive every bounding branch of a plausible model, and the edges.
BRANCH_TRIPLES = [
    (0, 0, 0),            # S = 0: NaN
    (900, 100, 0),        # z0 > 1
    (0, 1000, 0),         # z1 > 1 (or z0 = 0, z2 < 0)
    (0, 0, 1000),         # duplicates: z2 = 1, z1 = 0
    (0, 300, 700),        # parent-child like: z0 = 0
    (10, 900, 90),        # z2 < 0
    (60, 40, 900),        # z1 < 0
    (1, 0, 5000), (5000, 0, 1), (0, 1, 0), (1, 1, 1), (0xFFFFFF, 0xFFFFFF, 0xFFFFFF),
]


def seeded_triples(seed: int = 777, num: int = 400):
    rng = random.Random(seed)
    out = list(BRANCH_TRIPLES)
    for _ in range(num):
        s = rng.choice((5, 100, 5000, 100000, 1 << 22))
        a = rng.randint(0, s)
        b = rng.randint(0, s - a)
        out.append((a, b, s - a - b))
    return out


def records_of_triples(triples) -> np.ndarray:
    recs = np.zeros(len(triples), dtype=KING_RESULT_DTYPE)
    for k, (a, b, c) in enumerate(triples):
        recs[k] = (k, k + 1, np.float32(-1.0), a, b, c)
    return recs


# ---- a per-site numpy walk ---------------------------------------------------------------------
def genotypes_of_bits(bit_sets: np.ndarray, words_per_sample: int) -> np.ndarray:
    """uint8 [samples, 64 P]: 0 hom-ref, 1 het, 2 hom-var, 3 missing."""
    rows = np.ascontiguousarray(bit_sets, dtype=np.uint64).reshape(-1, words_per_sample)
    flat = np.unpackbits(rows.view(np.uint8), axis=1, bitorder="little")
    half = flat.shape[1] // 2
    het, hom = flat[:, :half], flat[:, half:]
    return np.where((het & hom) != 0, 3, het + 2 * hom).astype(np.uint8)


def site_counts_of_genotypes(g: np.ndarray) -> np.ndarray:
    return np.stack([(g == k).sum(axis=0) for k in range(4)], axis=1).astype(np.uint32)


def walk_records(sm, g: np.ndarray, model, min_pi_hat: float, bounded: bool = True) -> np.ndarray:
    """The records of block `sm` (a cuking_amd.Submatrix; g holds its stored samples: rows, then
    an off-diagonal block's columns) in ascending (i, j): IBS from the genotypes site by site."""
    diag = sm.i_begin == sm.j_begin
    out = []
    thr = np.float32(min_pi_hat)
    for i in range(sm.i_begin, sm.i_end):
        gi = g[i - sm.i_begin]
        for j in range(i + 1 if diag else sm.j_begin, sm.j_end):
            gj = g[j - sm.j_begin if diag else sm.NumRows() + j - sm.j_begin]
            both = (gi != 3) & (gj != 3)
            d = np.abs(gi.astype(np.int32) - gj.astype(np.int32))[both]
            ibs0, ibs1, ibs2 = int((d == 2).sum()), int((d == 1).sum()), int((d == 0).sum())
            p = pi_hat_f32(model, ibs0, ibs1, ibs2, bounded)
            if p > thr:
                out.append((i, j, p, ibs0, ibs1, ibs2))
    return np.array(out, dtype=KING_RESULT_DTYPE)


def random_bits(rng, samples: int, num_sites: int, words_per_sample: int, pad: str = "ones",
                missing: float = 0.03) -> np.ndarray:
    """A host bitset [samples, words_per_sample] of random genotypes; the bits behind num_sites
    are all ones (`missing`, as the packers leave them) or all zeros."""
    planes = words_per_sample // 2
    g = rng.choice(4, size=(samples, num_sites),
                   p=[0.5 * (1 - missing), 0.3 * (1 - missing), 0.2 * (1 - missing), missing])
    het = np.zeros((samples, 64 * planes), dtype=np.uint8)
    hom = np.zeros((samples, 64 * planes), dtype=np.uint8)
    het[:, :num_sites] = (g == 1) | (g == 3)
    hom[:, :num_sites] = (g == 2) | (g == 3)
    if pad == "ones":
        het[:, num_sites:] = 1
        hom[:, num_sites:] = 1
    both = np.concatenate([het, hom], axis=1)
    return np.packbits(both, axis=1, bitorder="little").view(np.uint64).copy()


# ---- the smoke() cohort ------------------------------------------------------------------------
SMOKE = dict(n=333, m=5000, seed=7)
# The host twin on this cohort with the model of its own 333 samples (measured on the CPU, see
# tests/test_pihat_host.py::test_smoke_cohort): the largest PI_HAT of a pair that is not planted
# and the smallest of one that is (the cohort plants 17 pairs: 14 parent-child, 1 duplicate, 1
# full-sibling, 1 half-sibling).
SMOKE_GAP = (0.14300692081451416, 0.2648268938064575)   # (float32 values, exactly)


@lru_cache(maxsize=None)
def smoke_cohort():
    """(cohort, host bits uint64 [n, wps], wps) of __graft_entry__.smoke()."""
    import cuking_amd
    from cuking_amd.synth import plan_cohort
    from oracle import pyoracle
    n, m, seed = SMOKE["n"], SMOKE["m"], SMOKE["seed"]
    cohort = plan_cohort(n, seed)
    host = pyoracle.synth_bitset(seed, cohort.kind, cohort.pa, cohort.pb, 0, n, m)
    wps = cuking_amd.words_per_sample(m)
    host = np.ascontiguousarray(host).view(np.uint64).reshape(n, wps)
    host.setflags(write=False)
    return cohort, host, wps
