"""What the host and the GPU tests of PC-Relate for listed pairs share (no GPU, no test of its
own): the case list, the integer formula of the exact cases, a float64 numpy reference written
from the definition of include/cuking_amd.h "PC-Relate for listed pairs" (taking the same
float32 X, beta and f), first-order tolerances for kin, k0, k1 and k2, the defects the
tolerances must catch, and the checks -- each written against a callable so that the host twin
and the device meet the same code.  pcrelate_cases.py supplies the base inputs (pitch padding
filled with NaN, an all-missing sample, sites around the bounds) as it is.

Every case's list starts with the special pairs (SPECIALS): a duplicate (kin 1/2, above the k0
switch; random pairs lie around 0, below it), a pair copied with half its sites redrawn, a self pair,
i > j, a repeat, the all-missing sample, the pair without a jointly valid site (exact cases)
and two with an index out of range; random pairs follow.

Tolerances.  With e(i, s) the error of a float32 mu (pcrelate_cases.Reference.e), the element
errors are eps_r = 2 e + 2^-24 |r|, eps_v = e |1 - 2 mu| / (2 sd) + 3 2^-24, eps_s2 = |1 + f| e
|1 - 2 mu| + 4 2^-24 |s2|, eps_e = e + 2^-24 + eps_s2 + 2^-24 |e|, eps_a = e_i (1 - mu_j) + mu_i
e_j + 2 2^-24 a (b likewise; a term of hden moves by 2 a eps_a).  A sum of T terms moves by its
propagated element errors plus (T + 2) 2^-24 sum |term|; a quotient N / D by dN / |D| + |q| dD /
|D| + 2 2^-24 |q|; k0 above the switch by 4 d kin + d k2 + 2^-24 (|1 - 4 kin| + |k0|), k1 by
d k2 + d k0 + 2^-24 (|1 - k2| + |k1|); every bound is doubled at the end.

Measured on the CPU with this file (test_pcrelate_pairs_host.py prints them): over the
real-valued cases the largest host-twin error is 0.0538 of its tolerance (kin of "P63 S1 d3"),
and the smallest defect, over every case and every defect the case is not immune to by
construction (Case.immune, with the reason beside the case), moves its best entry by 79.2
times that entry's tolerance ("switch ignored" on "P1 S63 d3"; the bound is 10 times).
"""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import pcrelate_cases as pc

from cuking_amd.api import KING_RESULT_DTYPE
from cuking_amd.pcrelate import PCRELATE_PAIR_DTYPE

EPS = pc.EPS
WORKGROUP_PAIRS = 512   # the kernel's threads per workgroup x pairs per thread (512 x 1)
STEP = 64               # the kernel's site step, which is also its word-prefetch step
SWITCH = np.float32(2.0 ** -2.5)
N = 40                  # samples of every case
FLOATS = ("kin", "k0", "k1", "k2")
# (i, j): duplicate, half-redrawn copy, self, i > j, [repeat of the first random pair],
# all-missing sample, no jointly valid site in the exact cases, out of range twice
SPECIALS = ((3, 4), (5, 6), (7, 7), (9, 1), None, (2, 8), (0, 1), (N, 0), (1, 0xFFFFFFFF))


@dataclass(frozen=True)
class Case:
    name: str
    pairs: int
    sites: int
    d: int
    stride: int = 8
    f: bool = False       # random f in (-0.1, 0.3); otherwise null
    seed: int = 1
    exact: bool = False
    pad: int = 0
    edge_every: int = 7
    immune: tuple = ()    # the DEFECTS that cannot show on this case, by its construction
    n: int = N            # samples
    lo: float = 0.01
    extra_word: object = None   # as pcrelate_cases.Case
    pads: object = None


def specials(n: int) -> tuple:
    """SPECIALS for a cohort of n samples: the out-of-range index is n; a special that names a
    sample the cohort does not have is left out."""
    kept = []
    for special in SPECIALS:
        if special is None:
            kept.append(None)
        elif special[0] == N:
            kept.append((n, 0))
        elif special[1] == 0xFFFFFFFF or max(special) < n:
            kept.append(special)
    return tuple(kept)


_NO_F = ("f ignored",)    # f is null: ignoring it changes nothing
CASES = (
    Case("exact P257 S700", 257, 700, 1, exact=True, pad=3),
    Case("exact P513 S65 stride 24", 513, 65, 1, stride=24, exact=True),
    Case("exact P512 S64", 512, 64, 1, exact=True),
    # (its one pair is the duplicate: no discordant site, and kin = 1/2 is above the switch, where
    #  k0 reads neither ibs0 nor hden)
    Case("P1 S63 d3", 1, 63, 3,
         immune=_NO_F + ("ibs0 counting het/hom", "b term of hden dropped")),
    # (seed 3: at seeds 1 and 2 the one site is invalid for most samples, or no pair with ibs0 > 0
    #  lies below the switch)
    Case("P63 S1 d3", 63, 1, 3, stride=24, f=True, seed=3),
    Case("P64 S64 d11", 64, 64, 11, f=True, pad=5),
    Case("P65 S65 d32", 65, 65, 32, stride=24, immune=_NO_F),
    Case("P257 S700 d3", 257, 700, 3, f=True, pad=1),
    Case("P512 S128 d1", 512, 128, 1, stride=24, f=True),
    Case("P513 S129 d11", 513, 129, 11, pad=7, immune=_NO_F),
    Case("P257 S700 d32", 257, 700, 32, stride=24, f=True, pad=1, edge_every=40),
)
REAL_CASES = tuple(c for c in CASES if not c.exact)
EXACT_CASES = tuple(c for c in CASES if c.exact)

# ---- the d ladder (pcrelate_cases.py has the reasons): every d from 1 to 32 at 130 samples and
# 97 sites (a partial step of 64), a list of 513 pairs (one more than a workgroup's), both
# strides, with and without f.  LADDER_SEEDS[d] is the smallest seed at which
# Reference.margin_violations() is 0 -- no element within e of a bound and no pair within its
# tolerance of the k0 switch --, found on the CPU: seed 1 at every d; check_reference asserts it
# on every rung, on the CPU in test_pcrelate_pairs_host.py.
LADDER_SEEDS = {d: 1 for d in range(1, 33)}
LADDER_FORMS = ((8, False), (8, True), (24, False), (24, True))    # (stride, f)


def ladder_case(d: int, stride: int = 8, f: bool = False, seed=None) -> Case:
    seed = LADDER_SEEDS[d] if seed is None else seed
    return Case(f"ladder P513 S{pc.LADDER_SITES} d{d} stride {stride}{' f' if f else ''}",
                WORKGROUP_PAIRS + 1, pc.LADDER_SITES, d, stride=stride, f=f, seed=seed,
                pad=d % 3, edge_every=7 + d, n=pc.LADDER_N)


def ladder(d: int) -> tuple:
    return tuple(ladder_case(d, stride, f) for stride, f in LADDER_FORMS)


@dataclass
class Inputs:
    case: Case
    code: np.ndarray      # uint8 [N, S]
    bits: np.ndarray      # uint64 [N, wps]
    x: np.ndarray         # float32 [N, d] (a view with pitch d + pad, NaN between)
    beta: np.ndarray      # float32 [S, d] (likewise)
    f: object             # float32 [N] or None
    lo: float
    hi: float
    index: np.ndarray     # uint32 [P, 2]
    pairs: np.ndarray     # what the call takes: index itself, or KING_RESULT_DTYPE records
    wps: int


def cohort(case: Case):
    """(code, bits, x, beta, lo, hi, rng) of a case: the cohort of pcrelate_cases.inputs with
    genotypes that follow the model and the planted relatives (from 10 samples on); `rng` goes
    on to draw the list and f."""
    n = case.n
    base = pc.inputs(pc.Case("pairs " + case.name, n, case.sites, case.d, (0, n, 0, n),
                             seed=case.seed, exact=case.exact, pad=case.pad, lo=case.lo,
                             edge_every=case.edge_every, extra_word=case.extra_word,
                             pads=case.pads))
    rng = np.random.default_rng(77 * case.seed + case.pairs + 3 * case.sites + 11 * case.d)
    code, x = np.array(base.code), np.array(base.x)
    planted = n >= 10
    # the planted relatives: 4 duplicates 3, 6 copies 5 with half its sites redrawn; both share
    # the model row of their original
    if planted:
        x[4], x[6] = x[3], x[5]

    def draw():   # codes [N, S]: 5 % missing
        if case.exact:
            return rng.choice(4, size=code.shape, p=(0.45, 0.3, 0.2, 0.05)).astype(np.uint8)
        # genotypes that FOLLOW the model, binomial(2, mu): unrelated pairs then have kin around
        # 0, below the switch (the codes of pcrelate_cases.py are independent of mu, which puts
        # every pair above it)
        mu = 0.5 * (x.astype(np.float64) @ np.asarray(base.beta, dtype=np.float64).T)
        drawn = rng.binomial(2, np.clip(mu, 0.02, 0.98)).astype(np.uint8)
        return np.where(rng.random(code.shape) < 0.05, 3, drawn).astype(np.uint8)

    if not case.exact:
        code = draw()
        if n > 2:
            code[2] = 3                          # the all-missing sample
    if planted:
        code[4] = code[3]
        code[6] = np.where(rng.random(case.sites) < 0.5, code[5], draw()[5])
    extra = case.sites % 3 == 0 if case.extra_word is None else case.extra_word
    bits = pc.pack_codes(code, rng, extra_words=1 if extra else 0)
    for a in (code, bits):
        a.setflags(write=False)
    return code, bits, pc._padded(x, base.case.pad_of(0)), base.beta, base.lo, base.hi, rng


def pair_list(index, stride: int, rng):
    """What the call takes for `index` uint32 [P, 2]: index itself at stride 8, records whose
    other fields hold garbage at stride 24."""
    if stride == 8:
        return index
    words = rng.integers(0, 2 ** 32, size=(index.shape[0], 6), dtype=np.uint64).astype(np.uint32)
    pairs = np.ascontiguousarray(words).view(KING_RESULT_DTYPE).reshape(-1)
    pairs["sample_i"], pairs["sample_j"] = index[:, 0], index[:, 1]
    return pairs


@lru_cache(maxsize=None)
def inputs(case: Case) -> Inputs:
    code, bits, x, beta, lo, hi, rng = cohort(case)
    n, special = case.n, specials(case.n)
    index = rng.integers(0, n, size=(case.pairs + len(special), 2), dtype=np.uint32)
    for k, pair in enumerate(special):
        index[k] = index[len(special)] if pair is None else pair
    index = np.ascontiguousarray(index[:case.pairs])
    pairs = pair_list(index, case.stride, rng)
    f = rng.uniform(-0.1, 0.3, size=n).astype(np.float32) if case.f else None
    for a in (index, pairs):
        a.setflags(write=False)
    return Inputs(case, code, bits, x, beta, f, lo, hi, index, pairs, bits.shape[1])


DEFECTS = ("f ignored", "het dominance not zero", "ibs0 counting het/hom", "switch ignored",
           "b term of hden dropped", "k1 with the wrong sign", "last site step skipped",
           "planes swapped")


class Reference:
    """The definition in float64 on the float32 inputs, one row per pair; the tolerances;
    optionally with one of DEFECTS built in."""

    def __init__(self, inp, defect=None):
        """`inp`: an Inputs, or anything with its arrays (code, x, beta, f, lo, hi, index): the
        shape comes from the arrays, as in pcrelate_cases.Reference."""
        sites, d = inp.code.shape[1], inp.x.shape[1]
        x64 = np.asarray(inp.x, dtype=np.float64)
        beta64 = np.asarray(inp.beta, dtype=np.float64)[:sites]
        code = inp.code.astype(np.int64)
        if defect == "planes swapped":
            code = np.where(code == 1, 2, np.where(code == 2, 1, code))
        n = code.shape[0]
        f = np.zeros(n) if inp.f is None or defect == "f ignored" else inp.f.astype(np.float64)
        mu = 0.5 * (x64 @ beta64.T)
        self.called = code != 3
        valid = self.called & (inp.lo < mu) & (mu < inp.hi)
        if defect == "last site step skipped" and sites:
            valid = valid & (np.arange(sites) < STEP * ((sites - 1) // STEP))
        self.mu, self.valid, self.bounds = mu, valid, (inp.lo, inp.hi)
        self.e = e_mu = (d + 2) * EPS * 0.5 * (np.abs(x64) @ np.abs(beta64).T)
        var = np.maximum(mu * (1.0 - mu), 0.0)
        sd = np.sqrt(var)
        r, v = code - 2.0 * mu, sd
        s2 = (1.0 + f)[:, None] * var
        dom = np.where(code == 0, mu, np.where(code == 1, 0.0, 1.0 - mu))
        if defect == "het dominance not zero":
            dom = np.where(code == 1, mu, dom)
        ee = dom - s2
        eps_r = 2.0 * e_mu + EPS * np.abs(r)
        eps_v = e_mu * np.abs(1.0 - 2.0 * mu) / (2.0 * np.where(sd > 0, sd, 1.0)) + 3 * EPS
        eps_s2 = np.abs(1.0 + f)[:, None] * e_mu * np.abs(1.0 - 2.0 * mu) + 4 * EPS * np.abs(s2)
        eps_e = e_mu + EPS + eps_s2 + EPS * np.abs(ee)

        # ---- the pairs: the smaller index leads (symmetric in float64 anyway)
        ok = (inp.index < n).all(axis=1)
        i = np.where(ok, inp.index.min(axis=1), 0).astype(np.int64)
        j = np.where(ok, inp.index.max(axis=1), 0).astype(np.int64)
        joint = valid[i] & valid[j] & ok[:, None]
        terms = (sites + 2) * EPS

        def chain(p, q, eps_p, eps_q):
            prod = np.where(joint, p[i] * q[j], 0.0)
            moved = np.where(joint, np.abs(p[i]) * eps_q[j] + eps_p[i] * np.abs(q[j]), 0.0)
            return prod.sum(axis=1), moved.sum(axis=1) + terms * np.abs(prod).sum(axis=1)

        num, d_num = chain(r, r, eps_r, eps_r)
        den, d_den = chain(v, v, eps_v, eps_v)
        dnum, d_dnum = chain(ee, ee, eps_e, eps_e)
        dden, d_dden = chain(s2, s2, eps_s2, eps_s2)
        a = np.where(joint, mu[i] * (1.0 - mu[j]), 0.0)
        b = np.where(joint, (1.0 - mu[i]) * mu[j], 0.0)
        eps_a = e_mu[i] * (1.0 - mu[j]) + mu[i] * e_mu[j] + 2 * EPS * a
        eps_b = e_mu[i] * mu[j] + (1.0 - mu[i]) * e_mu[j] + 2 * EPS * b
        if defect == "b term of hden dropped":
            b = np.zeros_like(b)
        hden = (a * a + b * b).sum(axis=1)
        d_hden = np.where(joint, 2 * a * eps_a + 2 * b * eps_b, 0.0).sum(axis=1) \
            + (2 * sites + 2) * EPS * hden
        ci, cj = code[i], code[j]
        differ = ci != cj if defect == "ibs0 counting het/hom" else (ci ^ cj) == 2
        self.ibs0 = (joint & differ).sum(axis=1).astype(np.uint32)
        self.sites = joint.sum(axis=1).astype(np.uint32)

        def quotient(n, dn, q, dq):
            with np.errstate(divide="ignore", invalid="ignore"):
                value = n / q
                return value, dn / np.abs(q) + np.abs(value) * dq / np.abs(q) \
                    + 2 * EPS * np.abs(value)

        with np.errstate(divide="ignore", invalid="ignore"):
            kin, d_kin = quotient(num, d_num, 4.0 * den, 4.0 * d_den)
            k2, d_k2 = quotient(dnum, d_dnum, dden, d_dden)
            low, d_low = quotient(self.ibs0.astype(np.float64), 0.0, hden, d_hden)
            high = (1.0 - 4.0 * kin) + k2
            d_high = 4.0 * d_kin + d_k2 + EPS * (np.abs(1.0 - 4.0 * kin) + np.abs(high))
            above = kin > float(SWITCH)
            if defect == "switch ignored":
                above = np.zeros_like(above)
            k0, d_k0 = np.where(above, high, low), np.where(above, d_high, d_low)
            sign = -1.0 if defect == "k1 with the wrong sign" else 1.0
            k1 = (1.0 - k2) - sign * k0
            d_k1 = d_k2 + d_k0 + EPS * (np.abs(1.0 - k2) + np.abs(k1))
        self.value = dict(kin=kin, k0=k0, k1=k1, k2=k2)
        self.tol = dict(kin=2.0 * d_kin, k0=2.0 * d_k0, k1=2.0 * d_k1, k2=2.0 * d_k2)
        self.above = above

    @classmethod
    def of(cls, code, x, beta, f, lo, hi, index, defect=None):
        """The Reference of bare arrays."""
        from types import SimpleNamespace
        return cls(SimpleNamespace(code=code, x=x, beta=beta, f=f, lo=lo, hi=hi, index=index),
                   defect)

    def margin_violations(self):
        """Called elements whose float64 mu lies within e of a bound, plus pairs whose kin lies
        within its tolerance of the switch: there float32 and float64 could take different
        paths."""
        near = (np.abs(self.mu - self.bounds[0]) <= self.e) | \
            (np.abs(self.mu - self.bounds[1]) <= self.e)
        kin, tol = self.value["kin"], self.tol["kin"]
        with np.errstate(invalid="ignore"):
            at_switch = np.abs(kin - float(SWITCH)) <= tol
        return int((self.called & near).sum()) + int(at_switch.sum())


@lru_cache(maxsize=None)
def reference(case: Case, defect=None) -> Reference:
    return Reference(inputs(case), defect)


def _canonical(a):
    return np.where(np.isnan(a), np.float32(np.nan), a).astype(np.float32)


def exact_expected(case: Case) -> np.ndarray:
    """The integer formula of the exact cases, PCRELATE_PAIR_DTYPE [P]: where beta is 1, mu is
    0.5, r = g - 1, v = 1/2, s2 = 1/4, e = +1/4 (hom) or -1/4 (het) and a = b = 1/4; elsewhere
    the site is invalid.  With n the jointly valid sites: 4 den = n, dden = n / 16, hden = n / 8
    and 16 dnum = (sites of equal zygosity) - (the others), all exact below 2^24, so every
    result is a chain of correctly rounded float32 operations on integers."""
    return exact_expected_of(inputs(case))


def exact_expected_of(inp) -> np.ndarray:
    """exact_expected on arrays: anything with code, beta and index of the exact construction."""
    f32 = np.float32
    ok = (inp.index < inp.code.shape[0]).all(axis=1)
    i, j = np.where(ok, inp.index[:, 0], 0), np.where(ok, inp.index[:, 1], 0)
    site_ok = inp.beta[:inp.code.shape[1], 0] == 1.0
    ci, cj = inp.code[i].astype(np.int64), inp.code[j].astype(np.int64)
    joint = (ci != 3) & (cj != 3) & site_ok[None, :] & ok[:, None]
    n = joint.sum(axis=1)
    num = ((ci - 1) * (cj - 1) * joint).sum(axis=1)
    same = joint & ((ci == 1) == (cj == 1))
    zyg = same.sum(axis=1) - (joint & ~same).sum(axis=1)
    ibs0 = (joint & ((ci ^ cj) == 2)).sum(axis=1)
    assert n.max() < 2 ** 24
    out = np.zeros(inp.index.shape[0], dtype=PCRELATE_PAIR_DTYPE)
    with np.errstate(divide="ignore", invalid="ignore"):
        kin = num.astype(f32) / n.astype(f32)
        k2 = zyg.astype(f32) / n.astype(f32)
        high = (f32(1.0) - f32(4.0) * kin) + k2
        low = ibs0.astype(f32) / (n.astype(f32) / f32(8.0))
        k0 = np.where(kin > SWITCH, high, low).astype(f32)
        k1 = (f32(1.0) - k2) - k0
    assert all(a.dtype == f32 for a in (kin, k2, high, low, k0, k1))
    out["sample_i"], out["sample_j"] = inp.index[:, 0], inp.index[:, 1]
    out["kin"], out["k0"], out["k1"], out["k2"] = (_canonical(a) for a in (kin, k0, k1, k2))
    out["ibs0"], out["sites"] = ibs0, n
    return out


def _in_tolerances(move, tol) -> float:
    """The largest move / tolerance; a tolerance of zero (the exact zero of 0 / hden) admits no
    move at all."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(move == 0.0, 0.0, move / tol).max())


# ---- the end-to-end fixture: pcrelate_cases.e2e_cohort() with more sites ----------------------
# e2e_cohort() as it is (2000 sites, seed 2) does not satisfy the conditions of the end-to-end
# test: on the float64 reference its largest parent-child k0 is 0.119, above the 0.1 that splits
# first degree.  This is the same construction (same populations, couples, Fst, missing rate and
# seed) at E2E_SITES = 8000 sites, where the sampling error of k0 is half as large.
E2E_SITES = 8000


@lru_cache(maxsize=None)
def e2e_cohort(seed=2):
    """(geno int8 [132, E2E_SITES] with -1 missing, fit bool [132] = the founders, parent_child:
    list of (i, j), siblings: list of (i, j))."""
    rng = np.random.default_rng(seed)
    ancestral = rng.uniform(0.1, 0.9, size=E2E_SITES)
    a = ancestral * (1 - pc.FST) / pc.FST
    b = (1 - ancestral) * (1 - pc.FST) / pc.FST
    freq = rng.beta(a, b, size=(pc.POPS, E2E_SITES))
    population = np.repeat(np.arange(pc.POPS), pc.PER_POP)
    founders = rng.binomial(2, freq[population]).astype(np.int8)
    n0 = founders.shape[0]
    children, parent_child, siblings = [], [], []
    for father, mother in pc.COUPLES:
        kids = []
        for _ in range(2):
            from_f = np.where(founders[father] == 1, rng.integers(0, 2, E2E_SITES),
                              founders[father] // 2)
            from_m = np.where(founders[mother] == 1, rng.integers(0, 2, E2E_SITES),
                              founders[mother] // 2)
            kids.append(n0 + len(children))
            children.append((from_f + from_m).astype(np.int8))
        parent_child += [(p, k) for k in kids for p in (father, mother)]
        siblings.append((kids[0], kids[1]))
    geno = np.concatenate([founders, np.stack(children)])
    geno[rng.random(geno.shape) < pc.MISSING] = -1
    geno.setflags(write=False)
    return geno, np.arange(geno.shape[0]) < n0, parent_child, siblings


def check_rows(case: Case, rows):
    check_rows_of(inputs(case).index, rows)


def check_rows_of(index, rows):
    """check_rows on arrays: the rows of the list `index`."""
    assert rows.dtype == PCRELATE_PAIR_DTYPE and rows.shape == (index.shape[0],)
    assert np.array_equal(rows["sample_i"], index[:, 0])
    assert np.array_equal(rows["sample_j"], index[:, 1])
    # every NaN is the one quiet NaN
    for name in FLOATS:
        bad = np.isnan(rows[name])
        assert (rows[name].view(np.uint32)[bad] == 0x7FC00000).all(), name


def check_exact(case: Case, backend):
    got, want = backend(case), exact_expected(case)
    check_rows(case, got)
    assert got.tobytes() == want.tobytes(), [
        (name, np.flatnonzero(got[name].view(np.uint32) != want[name].view(np.uint32))[:5])
        for name in PCRELATE_PAIR_DTYPE.names]
    if case.pairs >= len(SPECIALS):
        assert got["kin"][0] > SWITCH and (got["kin"][len(SPECIALS):] < SWITCH).any()
        for k in (5, 6, 7, 8):   # all-missing, no jointly valid site, out of range twice
            assert np.isnan([got[name][k] for name in FLOATS]).all(), k
            assert got["ibs0"][k] == 0 and got["sites"][k] == 0, k


def check_reference(case: Case, backend, label=""):
    """A float32 backend against the float64 reference: identical counts and NaN positions,
    every other value within the reference's tolerance.  Returns the largest error /
    tolerance."""
    ref = reference(case)
    worst = check_reference_of(ref, inputs(case).index, backend(case), case.name, label)
    if case.pairs >= len(SPECIALS) and case.sites >= 63:   # both sides of the switch
        below = ~ref.above & np.isfinite(ref.value["kin"])
        assert ref.above[0] and below[len(SPECIALS):].any()
    return worst


def check_reference_of(ref: Reference, index, got, name, label="", quiet=False):
    """check_reference on arrays: the rows `got` of the list `index` against its Reference."""
    assert ref.margin_violations() == 0, f"{name}: choose another seed"
    check_rows_of(index, got)
    assert np.array_equal(got["ibs0"], ref.ibs0) and np.array_equal(got["sites"], ref.sites)
    worst = 0.0
    for field in FLOATS:
        want, tol = ref.value[field], ref.tol[field]
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got[field]), nan), field
        inf = np.isinf(want)
        assert np.array_equal(got[field][inf], want[inf].astype(np.float32)), field
        ok = ~nan & ~inf
        if ok.any():
            ratio = _in_tolerances(np.abs(got[field].astype(np.float64) - want)[ok], tol[ok])
            if not quiet:
                print(f"{name} {label}: {field} largest tolerance {tol[ok].max():.3g}, largest "
                      f"error / tolerance {ratio:.3g}")
            worst = max(worst, ratio)
    assert worst <= 1.0, (name, label, worst)
    return worst


def defect_ratio(case: Case, defect: str) -> float:
    """The largest move of a value by `defect`, in units of that value's tolerance (a count
    that changes, or a value that becomes or stops being NaN or infinite, is infinitely far)."""
    return defect_ratio_of(reference(case), reference(case, defect))


def defect_ratio_of(ref: Reference, bad: Reference) -> float:
    """defect_ratio on two References of the same arrays, `bad` with the defect."""
    if not np.array_equal(ref.ibs0, bad.ibs0) or not np.array_equal(ref.sites, bad.sites):
        return float("inf")
    worst = 0.0
    for name in FLOATS:
        a, b, tol = ref.value[name], bad.value[name], ref.tol[name]
        if (np.isfinite(a) != np.isfinite(b)).any():
            return float("inf")
        ok = np.isfinite(a)
        if ok.any():
            worst = max(worst, _in_tolerances(np.abs(b - a)[ok], tol[ok]))
    return worst


# ---- the refusals: single arguments of a valid call on the case "P65 S65 d32" replaced (40
# samples x 65 sites, four words per sample); every one must come back as INVALID_ARGUMENT with
# out untouched
REFUSAL_CASE = next(c for c in CASES if c.name == "P65 S65 d32")
REFUSALS = {
    "d zero": dict(d=0),
    "d above the maximum": dict(d=33, ldx=40, ldbeta=40),
    "ldx below d": dict(ldx=31),
    "ldbeta below d": dict(ldbeta=31),
    "too many sites": dict(sites=129),
    "words_per_sample zero": dict(wps=0),
    "words_per_sample odd": dict(wps=3),
    "lo negative": dict(lo=-0.1),
    "lo not below hi": dict(lo=0.5, hi=0.5),
    "hi above one": dict(hi=1.5),
    "lo NaN": dict(lo=float("nan")),
    "stride below 8": dict(stride=4),
    "stride not a multiple of 4": dict(stride=10),
    "stride zero": dict(stride=0),
    "null bits": dict(bits=None),
    "null x": dict(x=None),
    "null beta": dict(beta=None),
    "null pairs": dict(pairs=None),
    "null out": dict(out=None),
}


def raw_arguments(inp: Inputs, pointers: dict, **over):
    """The argument list of cuking_pcrelate_pairs_host / cuking_pcrelate_pairs behind the
    context: `pointers` holds bits, x, beta, f, pairs, out, ldx, ldbeta."""
    case = inp.case
    a = dict(pointers, num_stored=case.n, wps=inp.wps, sites=case.sites, d=case.d, lo=inp.lo,
             hi=inp.hi, num_pairs=case.pairs, stride=case.stride)
    a.update(over)
    return (a["bits"], a["num_stored"], a["wps"], a["sites"], a["x"], a["ldx"], a["beta"],
            a["ldbeta"], a["d"], a["lo"], a["hi"], a["f"], a["pairs"], a["num_pairs"],
            a["stride"], a["out"])
