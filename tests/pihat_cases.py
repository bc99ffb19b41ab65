"""Cases and restatements for the PI_HAT tests (include/cuking_amd.h "PI_HAT (PLINK --genome)"):
the definition once more in Python floats, in the order csrc/king_pihat.h writes it, so that the
host twin, the kernel and this file must agree bit for bit; the same terms in exact rationals; a
per-site numpy walk that derives IBS0/1/2 from the genotypes; seeded count rows and IBS triples;
the smoke() cohort with its planted pairs; the pair math once more for arrays of counts
(z_of_counts_np, records_np: what the sweep of tests/pihat_fuzz_cases.py is judged by), the IBS
counts of the oracle's sums (ibs_of_counts), the models made by hand (MODELS) and the bare ABI
call the GPU tests share (raw_call)."""
import ctypes as C
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


# ---- the restatement once more, vectorised (numpy float64: the same IEEE operations) -----------
# The bounding steps in the order of csrc/king_pihat.h, and "nan": a pair whose PI_HAT is NaN.
STEPS = ("z0 > 1", "z1 > 1", "z2 > 1", "z0 < 0", "z1 < 0", "z2 < 0")
BRANCHES = STEPS + ("nan",)
# Subtly wrong restatements (tests/test_pihat_fuzz_cases.py: the sweeps' inputs tell each from
# the right one): what z_of_counts_np, records_np and ibs_of_counts do under `defect=`.
DEFECTS = ("threshold >=", "no z2 < 0 step", "z1 > 1 step last", "ibs1 = shared - ibs2",
           "no float32 rounding", "bounded ignored")


def z_of_counts_np(model, ibs0, ibs1, ibs2, bounded: bool = True, taken=None, defect=None):
    """z_of_counts for arrays of counts: (z0, z1, z2, pi_hat) as float64 arrays, the same
    operations in the same order, the branches as np.where steps in the order of the header; x / 0
    and 0 / 0 give what IEEE gives.  `taken`, a dict, gains per step of STEPS the number of pairs
    that took it (a step runs on what the steps before it left) and under "nan" the pairs whose
    pi_hat is NaN."""
    e00, e01, e02, e11, e12 = (np.float64(e) for e in model[:5])
    a0, a1, a2 = (np.asarray(a).astype(np.float64) for a in (ibs0, ibs1, ibs2))
    if defect == "bounded ignored":
        bounded = True
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        s = (a0 + a1) + a2
        z0 = a0 / (e00 * s)
        z1 = (a1 - z0 * (e01 * s)) / (e11 * s)
        z2 = ((a2 - z0 * (e02 * s)) - z1 * (e12 * s)) / s
        z = [z0, z1, z2]

        def note(name, c):
            if taken is not None:
                taken[name] = taken.get(name, 0) + int(np.count_nonzero(c))

        def above_one(k):
            c = z[k] > 1.0
            note(STEPS[k], c)
            for q in range(3):
                z[q] = np.where(c, 1.0 if q == k else 0.0, z[q])

        def below_zero(k):
            c = z[k] < 0.0
            note(STEPS[3 + k], c)
            a, b = (q for q in range(3) if q != k)
            t = z[a] + z[b]
            z[k] = np.where(c, 0.0, z[k])
            z[a], z[b] = np.where(c, z[a] / t, z[a]), np.where(c, z[b] / t, z[b])

        if bounded:
            above_one(0)
            if defect != "z1 > 1 step last":
                above_one(1)
            above_one(2)
            below_zero(0)
            below_zero(1)
            if defect != "no z2 < 0 step":
                below_zero(2)
            if defect == "z1 > 1 step last":
                above_one(1)
        pi_hat = z[1] / 2.0 + z[2]
    if taken is not None:
        taken["nan"] = taken.get("nan", 0) + int(np.isnan(pi_hat).sum())
    return z[0], z[1], z[2], pi_hat


def records_of_pi_hat(i, j, ibs0, ibs1, ibs2, pi_hat, min_pi_hat, defect=None) -> np.ndarray:
    """The pairs with float32(pi_hat) > float32(min_pi_hat) as records in ascending (i, j)."""
    thr = np.float32(min_pi_hat)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        kin = np.asarray(pi_hat, dtype=np.float64).astype(np.float32)
        if defect == "threshold >=":
            keep = kin >= thr
        elif defect == "no float32 rounding":
            keep = np.asarray(pi_hat, dtype=np.float64) > np.float64(thr)
        else:
            keep = kin > thr
    i, j = np.asarray(i), np.asarray(j)
    keep = np.flatnonzero(keep)
    keep = keep[np.lexsort((j[keep], i[keep]))]
    out = np.zeros(keep.size, dtype=KING_RESULT_DTYPE)
    out["sample_i"], out["sample_j"], out["kin"] = i[keep], j[keep], kin[keep]
    out["ibs0"], out["ibs1"], out["ibs2"] = (np.asarray(a)[keep] for a in (ibs0, ibs1, ibs2))
    return out


def records_np(sm, i, j, ibs0, ibs1, ibs2, model, min_pi_hat, bounded: bool = True,
               defect=None) -> np.ndarray:
    """What the scan returns for block `sm` (a cuking_amd.Submatrix) whose pairs (i, j) have
    the counts ibs0/1/2: KING_RESULT_DTYPE rows in ascending (i, j), the pairs with
    float32(pi_hat) > float32(min_pi_hat)."""
    i, j = np.asarray(i), np.asarray(j)
    assert ((i >= sm.i_begin) & (i < sm.i_end) & (j >= sm.j_begin) & (j < sm.j_end)).all()
    pi_hat = z_of_counts_np(model, ibs0, ibs1, ibs2, bounded, defect=defect)[3]
    return records_of_pi_hat(i, j, ibs0, ibs1, ibs2, pi_hat, min_pi_hat, defect)


def ibs_of_counts(oc, defect=None):
    """(ibs0, ibs1, ibs2) uint32 of the COUNTS_DTYPE rows of pyoracle.all_pairs, as the oracle's
    own records have them (tests/test_pihat_fuzz_cases.py holds this to the ibs fields of
    pyoracle.compute): opposite homozygotes; what is left; the same genotype."""
    ibs0 = oc["opposing_hom"].astype(np.uint32)
    ibs2 = (oc["concordant_hom"] + oc["both_het"]).astype(np.uint32)
    if defect == "ibs1 = shared - ibs2":
        return ibs0, (oc["shared"] - ibs2).astype(np.uint32), ibs2
    return ibs0, (oc["shared"] - ibs0 - ibs2).astype(np.uint32), ibs2


# ---- models ------------------------------------------------------------------------------------
MODELS = {
    "seeded rows": lambda: model_of_rows(seeded_count_rows()),
    "333 x 5000": lambda: model_of_rows([(150, 140, 40), (300, 30, 1), (100, 160, 70)] * 50),
    "zero e00": lambda: model_of_rows([(40, 0, 0), (0, 0, 7)]),
    "zero e00 and e11": lambda: (0.0, 0.0, 1.0, 0.0, 1.0, 3),
    "tiny e00": lambda: (1e-300, 0.4, 0.6, 0.36, 0.64, 9),
    "NaN": lambda: model_of_rows([]),
    # (no count row gives a negative expectation: z0 = ibs0 / (e00 S) >= 0 under every model of
    #  counts, so the z0 < 0 step can only be driven by a model made by hand)
    "negative e00": lambda: (-0.1, 0.4, 0.5, 0.4, 0.6, 3),
}


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


# ---- the bare ABI call on the device -----------------------------------------------------------
def raw_call(ctx, sm, wps, d_bits, model, capacity, tile_range=None, stream=None,
             min_pi_hat=0.05, sentinel_rows=4, flags=0):
    """The bare ABI call into a buffer of `capacity` records followed by `sentinel_rows` rows
    of 0x55 bytes: (records written as host rows, count, overflow flag, the rows behind)."""
    import torch
    import cuking_amd
    from cuking_amd import _lib
    dev = f"cuda:{ctx.device}"
    buf = torch.full((capacity + sentinel_rows, 6), 0x55555555, dtype=torch.int32, device=dev)
    words = torch.zeros(2, dtype=torch.int32, device=dev)
    head = (ctx.handle, C.byref(sm.c), wps, d_bits.data_ptr())
    tail = (C.byref(model.c), min_pi_hat, flags, capacity, buf.data_ptr() if capacity else None,
            words[0:1].data_ptr(), words[1:2].data_ptr(),
            stream.cuda_stream if stream is not None else None)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    if tile_range is None:
        _lib.check(ctx.lib.cuking_compute_pihat(*head, *tail))
    else:
        _lib.check(ctx.lib.cuking_compute_pihat_tiles(*head, *tile_range, *tail))
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize(ctx.device)
    count, overflow = (int(x) & 0xFFFFFFFF for x in words.tolist())
    host = buf.cpu().numpy()
    rows = np.ascontiguousarray(host[:min(count, capacity)]).view(cuking_amd.KING_RESULT_DTYPE)
    return rows.reshape(-1), count, overflow, host[capacity:]
