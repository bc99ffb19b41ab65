"""What the host and the GPU tests of the PCA share (no GPU, no test of its own): the seeded
three-population fixture, the dense float64 reference (numpy.linalg.eigh on the decoded
standardized matrix), a float64 twin of the randomized iteration written from the definition,
the tolerance computed from the reference data, and the checks, each written against a result
so that the host backend and the device backend meet the same code."""
from functools import lru_cache

import numpy as np

from site_qc_cases import pack, site_counts_numpy

import cuking_amd
from cuking_amd.pca import pca_omega

POPS, PER_POP, SITES, FST, MISSING, K = 3, 40, 640, 0.1, 0.02, 2
MONOMORPHIC = (5, 64, 333, 639)
OVERSAMPLE = 10
# The iteration count of the fixture: the float64 twin of the iteration then agrees with eigh
# in relative eigenvalue error and in 1 - sigma_min(U_ref^T U): measured on the CPU with this
# file, 4.4e-15 and 2.2e-16 fitted on all samples, 5.4e-15 and 0 fitted on 90 of them (at 6
# iterations 1.9e-9 / 4.6e-11 and 2.7e-9 / 6.5e-11: too few).  The bound on both is fixed: 1e-9.
# Tolerance of the float32 backends, from the reference's data (Reference.tolerance): 4 (K + 2)
# 2^-24 A with K = 640 and the per-column amplification A = 1.74 (both fits): 2.66e-4 -- a wrong
# divisor (640 sites for the 636 used: 6.3e-3), a swapped pair or a 1 % scale error all miss
# it.  The host backend's measured errors are 6.4e-9 (eigenvalues), 7.6e-8 (scores), 9.1e-8
# (loadings) and 7.8e-16 (subspace).
ITERATIONS = 10
TWIN_BOUND = 1e-9
EPS = 2.0 ** -24


@lru_cache(maxsize=None)
def cohort():
    """(geno int8 [120, 640] with -1 = missing, population [120]): a Balding-Nichols draw."""
    rng = np.random.default_rng(2024)
    ancestral = rng.uniform(0.1, 0.9, size=SITES)
    a = ancestral * (1 - FST) / FST
    b = (1 - ancestral) * (1 - FST) / FST
    freq = rng.beta(a, b, size=(POPS, SITES))
    population = np.repeat(np.arange(POPS), PER_POP)
    geno = rng.binomial(2, freq[population]).astype(np.int8)
    geno[:, MONOMORPHIC] = 0
    geno[rng.random(geno.shape) < MISSING] = -1
    geno.setflags(write=False)
    return geno, population


def standardized(geno, fit):
    """(Z_all float64 [n, m], used bool [m], p float64 [m]) from the definition: frequencies of
    the fit rows, (g - 2p) / sqrt(2p(1-p)), missing and unused sites 0."""
    sub = geno[fit]
    called = (sub >= 0).sum(axis=0)
    alt = np.where(sub >= 0, sub, 0).sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        p = alt / (2.0 * called)
        used = (called > 0) & (p > 0) & (p < 1)
        z = (geno - 2.0 * p) / np.sqrt(2.0 * p * (1.0 - p))
    z[:, ~used] = 0.0
    z[geno < 0] = 0.0
    return z, used, p


def sign_rule(v):
    """Each column's entry of largest magnitude (the lowest index among ties) positive."""
    top = np.argmax(np.abs(v), axis=0)
    return v * np.where(v[top, np.arange(v.shape[1])] < 0, -1.0, 1.0)


class Reference:
    """eigh of Z Z^T / M_used on the fit rows; loadings, scores of every row; the tolerance."""

    def __init__(self, geno, fit):
        self.fit = fit
        self.z_all, self.used, self.p = standardized(geno, fit)
        z = self.z = self.z_all[fit]
        self.m_used = int(self.used.sum())
        evals, evecs = np.linalg.eigh(z @ z.T / self.m_used)
        self.all_eigenvalues = evals[::-1]
        self.eigenvalues = evals[::-1][:K]
        self.u = evecs[:, ::-1][:, :K]
        sigma = np.sqrt(self.eigenvalues * self.m_used)
        self.loadings = sign_rule(z.T @ self.u / sigma)
        self.u = z @ self.loadings / sigma            # (signed like the loadings)
        self.scores = self.z_all @ self.loadings
        # Amplification of the two products Z^T U and Z V, in the norm the errors are measured
        # in (relative to a column's largest entry): per column, the largest sum |z w| over the
        # largest |sum z w|.  The entry-wise ratio sum |z w| / |sum z w|, taken at its largest
        # over all entries, is never smaller (at the entry with the largest sum |z w| it has
        # the same numerator and a denominator that is no larger) but one near-cancelling
        # entry sets it -- 7.35e4 and 3.60e3 on this fixture, tolerances of 11.3 and 0.55 that
        # nothing could miss --, so the tests hold the code to the per-column value.
        ratios, entrywise = [], []
        for left, right in ((z.T, self.u), (z, self.loadings)):
            total, absolute = np.abs(left @ right), np.abs(left) @ np.abs(right)
            ratios.append((absolute.max(axis=0) / total.max(axis=0)).max())
            entrywise.append((absolute[absolute > 0] / total[absolute > 0]).max())
        self.amplification = float(max(ratios))
        self.entrywise_amplification = float(max(entrywise))
        assert self.amplification <= self.entrywise_amplification
        self.tolerance = 4 * (max(z.shape) + 2) * EPS * self.amplification


@lru_cache(maxsize=None)
def reference(fit_name="all"):
    geno, population = cohort()
    ref = Reference(geno, fit_mask(fit_name))
    if fit_name == "all":   # the condition on the input
        assert ref.all_eigenvalues[1] / ref.all_eigenvalues[2] >= 3, ref.all_eigenvalues[:4]
    return ref


def fit_mask(name):
    """all, or 30 of each population's 40 (the rest are projected)."""
    geno, population = cohort()
    if name == "all":
        return np.ones(geno.shape[0], dtype=bool)
    return np.arange(geno.shape[0]) % PER_POP < 30


def twin(z, m_used, iterations=ITERATIONS, seed=0):
    """The iteration of cuking_amd/pca.py in float64 numpy, from its definition, with the same
    Omega: (eigenvalues [K], loadings [m, K])."""
    width = K + OVERSAMPLE
    q = np.linalg.qr(pca_omega(z.shape[0], width, seed).astype(np.float64))[0]
    for _ in range(iterations):
        q = np.linalg.qr(z @ (z.T @ q))[0]
    b = z.T @ q
    evals, evecs = np.linalg.eigh(b.T @ b)
    order = np.argsort(evals)[::-1][:K]
    v = b @ evecs[:, order]
    return evals[order] / m_used, sign_rule(v / np.linalg.norm(v, axis=0))


def subspace_gap(u_ref, u):
    """1 - sigma_min(U_ref^T U), U orthonormalized."""
    q = np.linalg.qr(u)[0]
    return 1.0 - np.linalg.svd(u_ref.T @ q, compute_uv=False).min()


def twin_error(ref):
    evals, v = twin(ref.z, ref.m_used)
    u = ref.z @ v
    return (np.abs(evals / ref.eigenvalues - 1).max(), subspace_gap(ref.u, u))


def bits_of_cohort():
    geno, _ = cohort()
    bits = pack(np.asarray(geno))
    return bits, bits.shape[1]


def check_result(got, ref, twin_gap):
    """A PCAResult against the dense reference, at the tolerance of the reference's data."""
    geno, population = cohort()
    tol = ref.tolerance
    n, m = geno.shape
    assert got.eigenvalues.shape == (K,) and got.scores.shape == (n, K)
    assert got.loadings.shape == (m, K) and got.allele_freq.shape == (m,)
    assert got.scores.dtype == np.float32 and got.loadings.dtype == np.float32
    assert np.array_equal(got.fit, ref.fit) and np.array_equal(got.sites_used, ref.used)
    assert not got.sites_used[list(MONOMORPHIC)].any()
    assert np.array_equal(got.allele_freq, ref.p, equal_nan=True)
    eig_err = np.abs(got.eigenvalues / ref.eigenvalues - 1).max()
    score_err = (np.abs(got.scores - ref.scores) / np.abs(ref.scores).max(axis=0)).max()
    load_err = (np.abs(got.loadings - ref.loadings) / np.abs(ref.loadings).max(axis=0)).max()
    u = got.scores[ref.fit].astype(np.float64)
    gap = subspace_gap(ref.u, u)
    print(f"amplification {ref.amplification:.4g}, tolerance {tol:.4g}: eigenvalue error "
          f"{eig_err:.3g}, score error {score_err:.3g}, loading error {load_err:.3g}, "
          f"subspace gap {gap:.3g} (twin {twin_gap:.3g})")
    assert (np.diff(got.eigenvalues) < 0).all()
    assert eig_err <= tol
    assert score_err <= tol
    assert load_err <= tol
    assert gap <= tol ** 2 + twin_gap
    # definition: unit columns, zero at unused sites, the sign rule
    assert np.abs(np.linalg.norm(got.loadings.astype(np.float64), axis=0) - 1).max() <= 4 * EPS
    assert (got.loadings[~ref.used] == 0).all()
    top = np.argmax(np.abs(got.loadings), axis=0)
    assert (got.loadings[top, np.arange(K)] > 0).all()
    # the scores are Z_all V with the FIT's frequencies, fit rows and projected rows alike
    want = ref.z_all @ got.loadings.astype(np.float64)
    bound = (m + 2) * EPS * (np.abs(ref.z_all) @ np.abs(got.loadings.astype(np.float64)))
    # (the table is rounded to float32 once: one more rounding per term)
    assert (np.abs(got.scores - want) <= bound + EPS * bound).all()


def check_separation(scores):
    """PC1 and PC2 separate the three populations: for every pair of populations, on the axis
    on which their centres lie further apart, the gap between them exceeds the spread of
    either."""
    _, population = cohort()
    for a in range(POPS):
        for b in range(a + 1, POPS):
            sa, sb = scores[population == a], scores[population == b]
            axis = int(np.argmax(np.abs(sa.mean(axis=0) - sb.mean(axis=0))))
            lo, hi = (sa, sb) if sa[:, axis].mean() < sb[:, axis].mean() else (sb, sa)
            gap = hi[:, axis].min() - lo[:, axis].max()
            spread = max(np.ptp(sa[:, axis]), np.ptp(sb[:, axis]))
            assert gap > spread, (a, b, axis, gap, spread)
