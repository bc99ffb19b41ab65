"""What the host and the GPU tests of PC-Relate share (no GPU, no test of its own): the case
list, a dense float64 numpy reference written from the definition of include/cuking_amd.h
"PC-Relate" (taking the same float32 X and beta), the tolerance functions, the defects the
tolerance must catch, the checks -- each written against a callable so that the host twin and
the device meet the same code -- and the seeded admixed cohort of the end-to-end test.

Measured on the CPU with this file (test_pcrelate_host.py prints them): over the real-valued
cases the largest tolerance of an entry against the float64 reference is 2.94e-4 (case
"257x700 d3"), the largest host-twin error is 0.048 of its entry's tolerance ("33x1 d3"), and
the smallest defect, over every case and every defect the case is not immune to by
construction (Case.immune, with the reason beside the case), moves its best entry by 20.4
times that entry's tolerance ("missing as hom-ref" on the single entry of "130x700 d3 one
entry"; 299 times on the whole-block cases; the bound is 10 times).  The d = 32 case at 700
sites has one site in 40 near each bound, not one in 7: (d + 2) 2^-24 makes e(i, s) five times
that of d = 3, and at one in 7 the expected number of elements within e of a bound was above
one per seed.
"""
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

EPS = 2.0 ** -24
STEP = 32   # the kernel's site step: what "the last site step skipped" drops


@dataclass(frozen=True)
class Case:
    name: str
    n: int
    sites: int
    d: int
    block: tuple          # (i_begin, i_end, j_begin, j_end)
    seed: int = 1
    exact: bool = False
    pad: int = 0          # extra elements in ldx, ldbeta and ldo
    lo: float = 0.01
    edge_every: int = 7   # one site in this many has mu around lo, another one around hi
    immune: tuple = ()    # the DEFECTS that cannot show on this case, by its construction
    extra_word: object = None   # a garbage plane word beyond the sites (None: where sites % 3 == 0)
    pads: object = None   # (x, beta, out) pitch pads of their own (None: `pad` for all three)

    def pad_of(self, which: int) -> int:
        return self.pad if self.pads is None else self.pads[which]


def _whole(n):
    return (0, n, 0, n)


CASES = (
    Case("exact 130x700", 130, 700, 1, _whole(130), exact=True, pad=3),
    Case("exact 33x65 block", 33, 65, 1, (0, 10, 10, 33), exact=True),
    Case("exact 257x64", 257, 64, 1, _whole(257), exact=True),
    # (its one element is a called hom-ref with mu inside the bounds, and it has one column)
    Case("1x1 d1", 1, 1, 1, _whole(1),
         immune=("missing as hom-ref", "planes swapped", "bounds ignored", "beta reversed")),
    Case("33x63 d3", 33, 63, 3, _whole(33)),
    Case("130x64 d11", 130, 64, 11, _whole(130), pad=5),
    Case("257x65 d32", 257, 65, 32, _whole(257)),
    Case("257x700 d3", 257, 700, 3, _whole(257), pad=1),
    Case("257x700 d32", 257, 700, 32, _whole(257), pad=1, edge_every=40),
    Case("257x700 d11 block", 257, 700, 11, (5, 70, 97, 257), pad=7),
    Case("130x700 d3 one entry", 130, 700, 3, (77, 78, 77, 78), pad=2),
    # (at its single site every sample's mu lies inside the bounds: 0.64 .. 0.84)
    Case("33x1 d3", 33, 1, 3, _whole(33), immune=("bounds ignored",)),
)
REAL_CASES = tuple(c for c in CASES if not c.exact)
EXACT_CASES = tuple(c for c in CASES if c.exact)

# ---- the d ladder: every d from 1 to 32 -- every bucket of pcrelate_dispatch_columns (4, 8, 16,
# 32) at its width, below it and at the first d of the next -- at the smallest shape that still
# has a partial tile (130 = 128 + 2), a partial site step (97 = 3 x 32 + 1) and a partial beta
# staging pass; the whole block and an off-diagonal one that starts and ends off a tile edge.
# One site in 7 + d has mu around lo and as many around hi: e(i, s) grows with d + 2 (the reason
# is in the module docstring).  LADDER_SEEDS[d] is the smallest seed at which
# Reference.margin_violations() is 0, found on the CPU: seed 1 at every d (about 0.02 elements
# within e of a bound are expected per rung); check_reference asserts it on every rung, on the
# CPU in test_pcrelate_host.py.
LADDER_N, LADDER_SITES = 130, 97
LADDER_BLOCKS = (_whole(LADDER_N), (5, 70, 97, 130))
LADDER_SEEDS = {d: 1 for d in range(1, 33)}


def ladder_case(d: int, block=LADDER_BLOCKS[0], seed=None, n=LADDER_N, sites=LADDER_SITES) -> Case:
    """The rung of the ladder at `d` (or the same construction at another shape or seed)."""
    seed = LADDER_SEEDS[d] if seed is None else seed
    kind = "" if block == _whole(n) else " block"
    return Case(f"ladder {n}x{sites} d{d}{kind}", n, sites, d, tuple(block), seed=seed,
                pad=d % 3, edge_every=7 + d)


LADDER = tuple(ladder_case(d, block) for d in range(1, 33) for block in LADDER_BLOCKS)


def pack_codes(code, rng, extra_words=0):
    """uint64 [n, 2 P] from codes [n, S] in 0..3 (het bit + 2 hom_var bit), P = ceil(S / 64) +
    extra_words, every bit at or beyond S random garbage."""
    n, sites = code.shape
    plane = max((sites + 63) // 64, 1) + extra_words
    bit = rng.integers(0, 2, size=(n, 2, plane * 64), dtype=np.uint8)
    bit[:, 0, :sites] = code & 1
    bit[:, 1, :sites] = code >> 1
    packed = np.packbits(bit.reshape(n, 2 * plane * 64), axis=1, bitorder="little")
    return np.ascontiguousarray(packed).view("<u8").astype(np.uint64).reshape(n, 2 * plane)


@dataclass
class Inputs:
    case: Case
    code: np.ndarray      # uint8 [n, S]
    bits: np.ndarray      # uint64 [n, wps]
    x: np.ndarray         # float32 [n, d] (a view with pitch d + pad)
    beta: np.ndarray      # float32 [S, d] (likewise)
    lo: float
    hi: float
    wps: int = field(init=False)

    def __post_init__(self):
        self.wps = self.bits.shape[1]


def _padded(a, pad):
    wide = np.full((a.shape[0], a.shape[1] + pad), np.float32(np.nan), dtype=np.float32)
    wide[:, :a.shape[1]] = a
    return wide[:, :a.shape[1]]


@lru_cache(maxsize=None)
def inputs(case: Case) -> Inputs:
    rng = np.random.default_rng(1000 * case.seed + case.n + 7 * case.sites + 13 * case.d)
    n, sites, d = case.n, case.sites, case.d
    code = rng.choice(4, size=(n, sites), p=(0.45, 0.3, 0.2, 0.05)).astype(np.uint8)
    lo = float(np.float32(case.lo))
    hi = float(np.float32(1.0) - np.float32(case.lo))
    if case.exact:
        x = np.ones((n, 1), dtype=np.float32)
        beta = rng.integers(0, 3, size=(sites, 1)).astype(np.float32)
        # the planted pair without a jointly valid site: sample 0 is called at the even
        # sites only, sample 1 at the odd ones
        if n > 1:
            code[0, 1::2] = 3
            code[1, 0::2] = 3
    else:
        # mu = p_s + a sample-specific shift: most sites inside the bounds for everybody, one
        # in edge_every with mu around or below lo (invalid for many), as many near 1
        p = rng.uniform(0.08, 0.92, size=sites)
        kind = rng.integers(0, case.edge_every, size=sites)
        p = np.where(kind == 0, rng.uniform(-0.04, 0.03, size=sites), p)
        p = np.where(kind == 1, rng.uniform(0.97, 1.04, size=sites), p)
        x = np.ones((n, d), dtype=np.float64)
        x[:, 1:] = rng.normal(0.0, 1.0, size=(n, d - 1))
        beta = np.empty((sites, d), dtype=np.float64)
        beta[:, 0] = 2.0 * p
        beta[:, 1:] = rng.normal(0.0, 0.06 / np.sqrt(max(d - 1, 1)), size=(sites, d - 1))
        if sites > 2:
            beta[1] = 0.0                    # a site with a zero row: invalid for everybody
        x, beta = x.astype(np.float32), beta.astype(np.float32)
    if n > 2:
        code[2] = 3                          # an all-missing sample
    extra = sites % 3 == 0 if case.extra_word is None else case.extra_word
    bits = pack_codes(code, rng, extra_words=1 if extra else 0)
    for a in (code, bits):
        a.setflags(write=False)
    return Inputs(case, code, bits, _padded(x, case.pad_of(0)), _padded(beta, case.pad_of(1)), lo,
                  hi)


DEFECTS = ("missing as hom-ref", "factor 4 dropped", "last step skipped", "planes swapped",
           "bounds ignored", "beta reversed")


class Reference:
    """The definition in float64 on the float32 inputs, for one block; the error terms of the
    tolerances; optionally with one of DEFECTS built in."""

    def __init__(self, code, x, beta, lo, hi, block, defect=None):
        sites, d = code.shape[1], x.shape[1]
        x64, beta64 = np.asarray(x, dtype=np.float64), np.asarray(beta, dtype=np.float64)[:sites]
        if defect == "beta reversed":
            beta64 = beta64[:, ::-1]
        code = code.astype(np.int64)
        if defect == "planes swapped":
            code = np.where(code == 1, 2, np.where(code == 2, 1, code))
        called = code != 3
        if defect == "missing as hom-ref":
            code, called = np.where(called, code, 0), np.ones_like(called)
        self.mu = mu = 0.5 * (x64 @ beta64.T)                       # [n, S]
        valid = called & (lo < mu) & (mu < hi)
        if defect == "bounds ignored":
            valid = called
        if defect == "last step skipped" and sites:
            valid = valid & (np.arange(sites) < STEP * ((sites - 1) // STEP))
        var = np.maximum(mu * (1.0 - mu), 0.0)
        self.called, self.valid = called, valid
        self.r = r = np.where(valid, code - 2.0 * mu, 0.0)
        self.v = v = np.where(valid, np.sqrt(var), 0.0)
        # element errors of a float32 evaluation (the fmaf chain of d terms, the halving, r, v)
        self.e = e = (d + 2) * EPS * 0.5 * (np.abs(x64) @ np.abs(beta64).T)
        eps_r = np.where(valid, 2.0 * e + EPS * np.abs(r), 0.0)
        sd = np.sqrt(var)
        eps_v = np.where(valid & (sd > 0), e * np.abs(1.0 - 2.0 * mu) / (2.0 * np.where(sd > 0, sd, 1.0))
                         + 3 * EPS, 0.0)
        i0, i1, j0, j1 = block
        ri, rj, vi, vj = r[i0:i1], r[j0:j1], v[i0:i1], v[j0:j1]
        self.num, self.den = ri @ rj.T, vi @ vj.T
        self.abs_num = np.abs(ri) @ np.abs(rj).T
        with np.errstate(divide="ignore", invalid="ignore"):
            self.kin = self.num / ((1.0 if defect == "factor 4 dropped" else 4.0) * self.den)
        self.d_num = np.abs(ri) @ eps_r[j0:j1].T + eps_r[i0:i1] @ np.abs(rj).T
        self.d_den = vi @ eps_v[j0:j1].T + eps_v[i0:i1] @ vj.T
        self.sites = sites
        self._bounds = (lo, hi)

    def _tolerance(self, d_num, d_den):
        acc = (self.sites + 2) * EPS
        with np.errstate(divide="ignore", invalid="ignore"):
            kin = np.abs(self.kin)
            return 2.0 * ((acc * self.abs_num + d_num) / (4.0 * self.den)
                          + (acc * self.den + d_den) * kin / self.den + 2 * EPS * kin)

    def twin_tolerance(self):
        """Device against host twin: the float32 accumulation bound of both sums, pushed
        through the quotient to first order and doubled: 2 [(S + 2) 2^-24 (sum |r r| / (4 den)
        + |kin|) + 2 2^-24 |kin|]."""
        return self._tolerance(0.0, 0.0)

    def tolerance(self):
        """A float32 backend against this reference: the bound above plus the propagated
        element errors, sum (|r_i| eps_r,j + |r_j| eps_r,i) on num and the same with v on den."""
        return self._tolerance(self.d_num, self.d_den)

    def margin_violations(self):
        """Called elements whose float64 mu lies within e of a bound: there float32 and float64
        could disagree on validity."""
        lo_hi = self._bounds
        near = (np.abs(self.mu - lo_hi[0]) <= self.e) | (np.abs(self.mu - lo_hi[1]) <= self.e)
        return int((self.called & near).sum())


@lru_cache(maxsize=None)
def reference(case: Case, defect=None) -> Reference:
    inp = inputs(case)
    return Reference(inp.code, inp.x, inp.beta, inp.lo, inp.hi, case.block, defect)


def exact_expected_of(code, beta, block) -> np.ndarray:
    """The integer formula of the exact construction, float32 [rows, cols]: where beta is 1, mu
    is 0.5, r = g - 1 and v = 0.5; elsewhere the site is invalid.  num is an integer, 4 den the
    count of the jointly called valid sites, both below 2^24, so kin = fl(num / count), NaN for
    0 / 0."""
    site_ok = beta[:code.shape[1], 0] == 1.0
    called = ((code != 3) & site_ok).astype(np.int64)
    g = (code.astype(np.int64) - 1) * called
    i0, i1, j0, j1 = block
    num, count = g[i0:i1] @ g[j0:j1].T, called[i0:i1] @ called[j0:j1].T
    assert np.abs(num).max() < 2 ** 24 and count.max() < 2 ** 24
    with np.errstate(invalid="ignore"):
        return num.astype(np.float32) / count.astype(np.float32)


def exact_expected(case: Case) -> np.ndarray:
    inp = inputs(case)
    return exact_expected_of(inp.code, inp.beta, case.block)


def check_exact(case: Case, backend):
    got = backend(case)
    want = exact_expected(case)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert got.tobytes() == want.tobytes(), np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:5]
    if case.block == _whole(case.n):
        assert np.isnan(got[0, 1]) and np.isnan(got[1, 0])   # the planted pair
        assert np.isnan(got[2]).all()                        # the all-missing sample


def check_reference(case: Case, backend, label=""):
    """A float32 backend against the float64 reference: identical NaN positions, every other
    entry within the reference's tolerance.  Returns the largest error / tolerance."""
    return check_reference_of(reference(case), backend(case), case.name, label)


def check_reference_of(ref: Reference, got, name, label="", quiet=False):
    """check_reference on arrays: `got` against a Reference of the same block."""
    assert ref.margin_violations() == 0, f"{name}: choose another seed"
    tol = ref.tolerance()
    assert got.dtype == np.float32 and got.shape == ref.kin.shape
    nan = np.isnan(ref.kin)
    assert np.array_equal(np.isnan(got), nan), np.argwhere(np.isnan(got) != nan)[:5]
    ratio = (np.abs(got - ref.kin)[~nan] / tol[~nan]).max() if (~nan).any() else 0.0
    if not quiet:
        print(f"{name} {label}: largest tolerance {tol[~nan].max() if (~nan).any() else 0:.3g}, "
              f"largest error / tolerance {ratio:.3g}")
    assert ratio <= 1.0, (name, label, ratio)
    return ratio


def check_twin(case: Case, device_backend, host_backend):
    """Device against host twin: identical NaN positions, the accumulation bound."""
    check_twin_of(reference(case), device_backend(case), host_backend(case), case.name)


def check_twin_of(ref: Reference, dev, host, name, quiet=False):
    """check_twin on arrays."""
    tol = ref.twin_tolerance()
    nan = np.isnan(host)
    assert np.array_equal(np.isnan(dev), nan) and np.array_equal(np.isnan(ref.kin), nan)
    ratio = (np.abs(dev.astype(np.float64) - host)[~nan] / tol[~nan]).max() if (~nan).any() else 0.0
    if not quiet:
        print(f"{name}: device against host twin, largest error / tolerance {ratio:.3g}")
    assert ratio <= 1.0, (name, ratio)
    return ratio


def defect_ratio(case: Case, defect: str) -> float:
    """The largest move of an entry by `defect`, in units of that entry's tolerance (an entry
    that becomes or stops being NaN counts as infinitely far)."""
    return defect_ratio_of(reference(case), reference(case, defect))


def defect_ratio_of(ref: Reference, bad: Reference) -> float:
    """defect_ratio on two References of the same arrays and block, `bad` with the defect."""
    tol = ref.tolerance()
    if (np.isnan(ref.kin) != np.isnan(bad.kin)).any():
        return float("inf")
    ok = ~np.isnan(ref.kin)
    return float((np.abs(bad.kin - ref.kin)[ok] / tol[ok]).max()) if ok.any() else 0.0


# ---- the refusals: single arguments of a valid call on CASES[4] (33 samples x 63 sites, d = 3,
# two plane words) replaced; every one must come back as INVALID_ARGUMENT with out untouched
REFUSALS = {
    "d zero": dict(d=0),
    "d above the maximum": dict(d=33, ldx=40, ldbeta=40),
    "ldx below d": dict(ldx=2),
    "ldbeta below d": dict(ldbeta=2),
    "too many sites": dict(sites=129),
    "words_per_sample zero": dict(wps=0),
    "words_per_sample odd": dict(wps=1),
    "lo negative": dict(lo=-0.1),
    "lo not below hi": dict(lo=0.5, hi=0.5),
    "hi above one": dict(hi=1.5),
    "lo NaN": dict(lo=float("nan")),
    "rows outside": dict(block=(0, 34, 0, 34), ldo=34),
    "columns outside": dict(block=(0, 10, 10, 34), ldo=40),
    "block reversed": dict(block=(5, 4, 5, 4)),
    "pitch below the columns": dict(ldo=32),
    "null bits": dict(bits=None),
    "null x": dict(x=None),
    "null beta": dict(beta=None),
    "null out": dict(out=None),
}


# ---- the end-to-end fixture: an admixed cohort with planted families -------------------------
POPS, PER_POP, E2E_SITES, FST, MISSING, E2E_K = 3, 40, 2000, 0.1, 0.02, 2
# (father, mother) founder indices: three couples within a population, three across
COUPLES = ((0, 1), (40, 41), (80, 81), (2, 42), (43, 82), (83, 3))


@lru_cache(maxsize=None)
def e2e_cohort(seed=2):
    """(geno int8 [132, 2000] with -1 missing, population [132] with -1 for the children, fit
    bool [132] = the founders, related: set of (i, j) i < j first-degree pairs)."""
    rng = np.random.default_rng(seed)
    ancestral = rng.uniform(0.1, 0.9, size=E2E_SITES)
    a = ancestral * (1 - FST) / FST
    b = (1 - ancestral) * (1 - FST) / FST
    freq = rng.beta(a, b, size=(POPS, E2E_SITES))
    population = np.repeat(np.arange(POPS), PER_POP)
    founders = rng.binomial(2, freq[population]).astype(np.int8)
    n0 = founders.shape[0]
    children, related = [], set()
    for c, (f, m) in enumerate(COUPLES):
        kids = []
        for _ in range(2):
            # one allele from each parent: a het parent passes the alt allele half the time
            from_f = np.where(founders[f] == 1, rng.integers(0, 2, E2E_SITES), founders[f] // 2)
            from_m = np.where(founders[m] == 1, rng.integers(0, 2, E2E_SITES), founders[m] // 2)
            kids.append(n0 + len(children))
            children.append((from_f + from_m).astype(np.int8))
        for k in kids:
            related.update({(f, k), (m, k)})
        related.add((kids[0], kids[1]))
    geno = np.concatenate([founders, np.stack(children)])
    geno[rng.random(geno.shape) < MISSING] = -1
    geno.setflags(write=False)
    population = np.concatenate([population, np.full(len(children), -1)])
    fit = np.arange(geno.shape[0]) < n0
    return geno, population, fit, related


def e2e_masks():
    """(related bool [n, n], cross bool [n, n] = unrelated founder pairs from different
    populations), both over i < j."""
    geno, population, fit, related = e2e_cohort()
    n = geno.shape[0]
    upper = np.triu(np.ones((n, n), dtype=bool), 1)
    rel = np.zeros((n, n), dtype=bool)
    for i, j in related:
        rel[min(i, j), max(i, j)] = True
    founder = population >= 0
    cross = upper & founder[:, None] & founder[None, :] & \
        (population[:, None] != population[None, :]) & ~rel
    return rel, cross, upper


def check_e2e(result, bits, naive):
    """A PCRelateResult (its `kin` already a host array) of the end-to-end fixture: the
    conditions on the fixture on the float64 reference fed with the backend's own X and beta,
    the backend's beta against the float64 regression, its entries against the reference."""
    geno, population, fit, _ = e2e_cohort()
    n, sites = geno.shape
    code = np.where(geno < 0, 3, geno).astype(np.uint8)
    lo, hi = float(np.float32(0.01)), float(np.float32(1.0) - np.float32(0.01))
    ref = Reference(code, result.x, result.beta, lo, hi, (0, n, 0, n))
    ref._bounds = (lo, hi)
    rel, cross, upper = e2e_masks()
    # -- conditions on the fixture
    first = ref.kin[rel]
    assert first.min() > 0.177 and first.max() < 0.354, (first.min(), first.max())
    others = ref.kin[upper & ~rel]
    assert others.max() < 0.0884, others.max()
    cross_mean = ref.kin[cross].mean()
    assert abs(cross_mean) <= 0.005, cross_mean
    ii, jj, counts = naive.all_pairs_matmul(np.asarray(geno))
    king = np.full((n, n), np.nan)
    king[ii, jj] = naive.kin_f32(counts[:, 0], counts[:, 1], counts[:, 2], counts[:, 3])
    king_cross = king[cross].mean()
    assert king_cross < -0.05, king_cross
    print(f"first degree {first.min():.3f} .. {first.max():.3f}, largest other {others.max():.3f}, "
          f"cross-population mean {cross_mean:.5f} (KING-robust {king_cross:.3f})")
    # -- beta against the float64 regression on the backend's X
    x64 = result.x.astype(np.float64)[fit]
    sub = geno[fit].astype(np.float64)
    called = (geno[fit] >= 0)
    count = called.sum(axis=0)
    p = np.where(called, sub, 0.0).sum(axis=0) / (2.0 * count)
    used = (count > 0) & (p > 0) & (p < 1)
    assert np.array_equal(result.sites_used, used) and np.array_equal(result.fit, fit)
    g = np.where(called, sub, 2.0 * p) * used
    gram_inv = np.linalg.inv(x64.T @ x64)
    beta64 = (g.T @ x64) @ gram_inv
    n_fit = int(fit.sum())
    # (4 (n_fit + 2) 2^-24 sum |X g| on X^T G, pushed through the solve; one rounding of 2p in
    #  the table and one of beta to float32 on top)
    bound = (4 * (n_fit + 2) * EPS * (np.abs(g).T @ np.abs(x64))) @ np.abs(gram_inv) \
        + EPS * np.abs(beta64)
    err = np.abs(result.beta - beta64)
    print(f"beta: largest error / bound {(err / np.maximum(bound, 1e-300)).max():.3g}")
    assert (err <= bound).all()
    assert (result.beta[~used] == 0).all()
    # -- the entries against the reference (the backend judged on its own inputs: X and beta
    #    are exactly what the reference was fed, so the scores' tolerance adds nothing).  The
    #    price: nothing here compares one backend's scores with another's; the scores are held
    #    to their own reference by the PCA tests, and beta to the float64 regression above.
    assert ref.margin_violations() == 0
    tol = ref.tolerance()
    kin = np.asarray(result.kin)
    assert kin.dtype == np.float32 and not np.isnan(kin).any() and not np.isnan(ref.kin).any()
    ratio = (np.abs(kin - ref.kin) / tol).max()
    print(f"kin: largest tolerance {tol.max():.3g}, largest error / tolerance {ratio:.3g}")
    assert ratio <= 1.0
    assert np.allclose(result.inbreeding(), 2.0 * np.diagonal(kin) - 1.0)
