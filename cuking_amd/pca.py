"""Principal components of the standardized genotype matrix, fitted on a subset of the samples
(the unrelated ones) with every sample projected: PC-AiR style ancestry PCA on the bitset
where it lies.  The only contact with the genotypes is the 2-bit matrix product
(``KingContext.geno_matmul`` / ``geno_matmul_host``): no expanded matrix, no N x N matrix.

Definition.  With the genotype counts of the FIT rows (``site_counts``), per site ``called``
and ``alt`` as ``site_mask_host`` defines them and ``p = alt / (2 called)``: a site is USED iff
``called > 0`` and ``0 < p < 1``; its standardized genotypes are ``(g - 2p) / sqrt(2p(1-p))``
for g = 0, 1, 2 and 0 for a missing one (mean imputation: PLINK, Hail's
``hwe_normalized_pca``); an unused site is all zeros (``hwe_table``).  Z is that matrix over
the fit rows, M_used the number of used sites.  ``eigenvalues[j] = sigma_j^2 / M_used`` with
sigma_j the singular values of Z, descending; ``loadings`` are the right singular vectors
``[num_sites, k]``, unit columns, each signed so that its entry of largest magnitude (the
lowest index among ties) is positive; ``scores = Z_all loadings`` for EVERY stored row with
the FIT's table, so fit and projected samples get their scores from one formula.

Algorithm (``pca``): randomized subspace iteration with ``L = k + oversample <= 64`` columns.
Omega ``[n_fit, L]`` standard normal from a seeded CPU generator (``pca_omega``); ``Q =
qr(Omega)``; ``iterations`` times ``W = Z^T Q``, ``Y = Z W``, ``Q = qr(Y)``; then ``B = Z^T Q``
and the eigenvectors of the ``L x L`` Gram matrix of B.  The two products run in float32 on the
backend; QR, the Gram matrix and the small eigenproblem in float64 (torch or numpy).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _lib
from .api import (_count, geno_matmul_host, ld_site_words, transpose_sites_host)

RHS_MAX = _lib.GENO_RHS_MAX


@dataclass
class PCAResult:
    """What ``KingContext.pca`` / ``pca_host`` return, as host arrays: ``eigenvalues``
    (float64 ``[k]``, descending), ``scores`` (float32 ``[rows, k]``, every stored row),
    ``loadings`` (float32 ``[num_sites, k]``, unit columns, zero at unused sites),
    ``allele_freq`` (float64 ``[num_sites]``, of the fit rows; NaN without a called genotype),
    ``sites_used`` (bool ``[num_sites]``) and ``fit`` (bool ``[rows]``)."""
    eigenvalues: np.ndarray
    scores: np.ndarray
    loadings: np.ndarray
    allele_freq: np.ndarray
    sites_used: np.ndarray
    fit: np.ndarray


def hwe_table(site_counts, num_sites: int):
    """The table of the standardized genotypes from the ``[>= num_sites, 4]`` site counts
    (hom_ref, het, hom_var, missing): float32 ``[num_sites, 4]`` rows ``[(0-2p)/s, (1-2p)/s,
    (2-2p)/s, 0]`` with ``p = alt / (2 called)`` and ``s = sqrt(2p(1-p))``, computed in float64
    and rounded once; four zeros for a site that is not used (``called == 0``, ``p`` 0 or 1).
    Returns ``(table, used, p)``; ``p`` is NaN where nothing is called."""
    num_sites = _count(num_sites, "num_sites")
    counts = np.asarray(site_counts)
    if counts.ndim != 2 or counts.shape[1] != 4 or counts.shape[0] < num_sites:
        raise ValueError(f"site_counts must be [>= {num_sites}, 4], not {counts.shape}")
    c = counts[:num_sites].view(np.uint32) if counts.dtype == np.int32 else counts[:num_sites]
    c = c.astype(np.int64)
    called = c[:, 0] + c[:, 1] + c[:, 2]
    alt = c[:, 1] + 2 * c[:, 2]
    used = (called > 0) & (alt > 0) & (alt < 2 * called)
    p = np.full(num_sites, np.nan, dtype=np.float64)
    np.divide(alt.astype(np.float64), (2 * called).astype(np.float64), out=p, where=called > 0)
    table = np.zeros((num_sites, 4), dtype=np.float64)
    pu = p[used]
    s = np.sqrt(2.0 * pu * (1.0 - pu))
    for g in range(3):
        table[used, g] = (g - 2.0 * pu) / s
    return table.astype(np.float32), used, p


def pca_omega(n_fit: int, num_columns: int, seed: int) -> np.ndarray:
    """The start matrix of ``pca``: float32 ``[n_fit, num_columns]``, standard normal, from
    ``numpy.random.default_rng(seed)``."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n_fit, num_columns)).astype(np.float32)


def check_pca_arguments(n_fit: int, num_used: int, k: int, oversample: int, iterations: int):
    """The refusals of ``pca``, with the numbers in the message."""
    k, oversample = _count(k, "k"), _count(oversample, "oversample")
    _count(iterations, "iterations")
    if n_fit < 2:
        raise ValueError(f"pca: {n_fit} fit samples, at least 2 are needed")
    if num_used < 1:
        raise ValueError("pca: no used site (0 sites with a called genotype and 0 < p < 1 "
                         "among the fit samples)")
    if k < 1:
        raise ValueError(f"pca: k = {k}, at least 1 component is needed")
    if k + oversample > min(RHS_MAX, n_fit):
        raise ValueError(f"pca: k + oversample = {k} + {oversample} = {k + oversample} exceeds "
                         f"min({RHS_MAX}, {n_fit} fit samples) = {min(RHS_MAX, n_fit)}")


class HostOperator:
    """Z of the fit rows and Z_all over host bitsets, on ``geno_matmul_host`` and numpy."""

    def __init__(self, bits: np.ndarray, words_per_sample: int, num_sites: int, fit=None):
        assert bits.dtype == np.uint64 and bits.flags.c_contiguous
        self.words_per_sample, self.num_sites = words_per_sample, num_sites
        self.bits = bits.reshape(-1, words_per_sample)
        self.fit = _fit_mask(fit, self.bits.shape[0])
        self.fit_bits = np.ascontiguousarray(self.bits[self.fit])
        self.n_fit = self.fit_bits.shape[0]
        self.table, self.used, self.p = hwe_table(host_site_counts(self.fit_bits), num_sites)
        self.q2 = 2 * ld_site_words(self.n_fit)
        self.site_bits = transpose_sites_host(self.fit_bits, words_per_sample,
                                              num_sites).reshape(num_sites, self.q2)

    def from_host(self, a):
        return np.ascontiguousarray(a, dtype=np.float32)

    def to_host64(self, a):
        return np.asarray(a, dtype=np.float64)

    def zt(self, a):  # Z^T A: [num_sites, L]
        return geno_matmul_host(self.site_bits, self.q2, self.n_fit, self.table, a, per_row=True)

    def z(self, b):  # Z B: [n_fit, L]
        return geno_matmul_host(self.fit_bits, self.words_per_sample, self.num_sites, self.table, b)

    def z_all(self, b):
        return geno_matmul_host(self.bits, self.words_per_sample, self.num_sites, self.table, b)

    def qr(self, y):
        return self.from_host(np.linalg.qr(np.asarray(y, dtype=np.float64))[0])

    def gram_eigh(self, b):
        b64 = np.asarray(b, dtype=np.float64)
        return np.linalg.eigh(b64.T @ b64)


class DeviceOperator:
    """Z of the fit rows and Z_all over device bitsets, on ``KingContext.geno_matmul`` and
    torch."""

    def __init__(self, ctx, bits, words_per_sample: int, num_sites: int, fit=None):
        import torch
        self.ctx, self.words_per_sample, self.num_sites = ctx, words_per_sample, num_sites
        rows = ctx._rows_of(bits, words_per_sample)
        self.dev = f"cuda:{ctx.device}"
        self.bits = bits.view(rows, words_per_sample)
        if isinstance(fit, torch.Tensor):
            fit = fit.cpu().numpy()
        self.fit = _fit_mask(fit, rows)
        if self.fit.all():
            self.fit_bits = self.bits
        else:
            index = torch.from_numpy(np.flatnonzero(self.fit)).to(self.dev)
            self.fit_bits = self.bits.index_select(0, index).contiguous()
        self.n_fit = self.fit_bits.shape[0]
        if self.n_fit:
            counts = ctx.site_counts(self.fit_bits, words_per_sample).cpu().numpy().view(np.uint32)
        else:
            counts = np.zeros((words_per_sample // 2 * 64, 4), dtype=np.uint32)
        table, self.used, self.p = hwe_table(counts, num_sites)
        self.table = torch.from_numpy(table).to(self.dev)
        self.q2 = 2 * ld_site_words(self.n_fit)
        self.site_bits = ctx.transpose_sites(self.fit_bits, words_per_sample,
                                             num_sites).view(num_sites, self.q2) \
            if self.n_fit else None

    def from_host(self, a):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.dev)

    def to_host64(self, a):
        return a.double().cpu().numpy()

    def zt(self, a):
        return self.ctx.geno_matmul(self.site_bits, self.q2, self.n_fit, self.table, a,
                                    per_row=True)

    def z(self, b):
        return self.ctx.geno_matmul(self.fit_bits, self.words_per_sample, self.num_sites,
                                    self.table, b)

    def z_all(self, b):
        return self.ctx.geno_matmul(self.bits, self.words_per_sample, self.num_sites,
                                    self.table, b)

    def qr(self, y):
        import torch
        return torch.linalg.qr(y.double())[0].float().contiguous()

    def gram_eigh(self, b):
        import torch
        b64 = b.double()
        w, v = torch.linalg.eigh(b64.T @ b64)
        return w.cpu().numpy(), v.cpu().numpy()


def _fit_mask(fit, rows: int) -> np.ndarray:
    if fit is None:
        return np.ones(rows, dtype=bool)
    fit = np.asarray(fit)
    if fit.shape != (rows,):
        raise ValueError(f"fit must hold one entry per stored sample ({rows}), not {fit.shape}")
    return fit.astype(bool)


def host_site_counts(bits: np.ndarray) -> np.ndarray:
    """(hom_ref, het, hom_var, missing) per plane site of a host bitset ``[rows, words]``:
    uint32 ``[64 P, 4]``, what ``KingContext.site_counts`` gives on the device."""
    rows, wps = bits.shape
    plane = wps // 2
    counts = np.zeros((plane * 64, 4), dtype=np.uint32)
    for begin in range(0, rows, 1024):  # (bounded expansion: 1024 rows at a time)
        part = np.ascontiguousarray(bits[begin:begin + 1024]).astype("<u8")
        bit = np.unpackbits(part.view(np.uint8).reshape(part.shape[0], wps * 8), axis=1,
                            bitorder="little")
        code = bit[:, :plane * 64] + 2 * bit[:, plane * 64:]
        for g in range(4):
            counts[:, g] += (code == g).sum(axis=0).astype(np.uint32)
    return counts


def pca(op, k: int, oversample: int = 10, iterations: int = 10, seed: int = 0) -> PCAResult:
    """Randomized subspace iteration over an operator (``HostOperator``, ``DeviceOperator``:
    ``z``, ``zt``, ``z_all``, ``qr``, ``gram_eigh``); the module docstring has the definition
    of the result.  ValueError: fewer than 2 fit samples, no used site, ``k < 1``, ``k +
    oversample > min(64, n_fit)``."""
    num_used = int(op.used.sum())
    check_pca_arguments(op.n_fit, num_used, k, oversample, iterations)
    width = k + oversample
    q = op.qr(op.from_host(pca_omega(op.n_fit, width, seed)))
    for _ in range(iterations):
        q = op.qr(op.z(op.zt(q)))
    b = op.zt(q)                                  # [num_sites, L]
    evals, evecs = op.gram_eigh(b)                # ascending
    order = np.argsort(evals)[::-1][:k]
    sigma2 = np.maximum(evals[order], 0.0)
    v = op.to_host64(b) @ evecs[:, order]         # [num_sites, k], columns of length sigma
    norms = np.linalg.norm(v, axis=0)
    v = v / np.where(norms > 0, norms, 1.0)
    loadings = v.astype(np.float32)
    top = np.argmax(np.abs(loadings), axis=0)     # (the first among ties)
    flip = loadings[top, np.arange(k)] < 0
    loadings[:, flip] = -loadings[:, flip]
    scores = op.z_all(op.from_host(loadings))
    scores = np.asarray(op.to_host64(scores), dtype=np.float32)
    return PCAResult(sigma2 / num_used, scores, loadings, op.p, op.used, op.fit)


def pca_host(bits: np.ndarray, words_per_sample: int, num_sites: int, k: int = 10, fit=None,
             oversample: int = 10, iterations: int = 10, seed: int = 0) -> PCAResult:
    """``KingContext.pca`` on host memory and the host twin of the product: no GPU."""
    op = HostOperator(bits, _count(words_per_sample, "words_per_sample"),
                      _count(num_sites, "num_sites"), fit)
    return pca(op, k, oversample, iterations, seed)


def pca_device(ctx, bits, words_per_sample: int, num_sites: int, k: int = 10, fit=None,
               oversample: int = 10, iterations: int = 10, seed: int = 0) -> PCAResult:
    op = DeviceOperator(ctx, bits, _count(words_per_sample, "words_per_sample"),
                        _count(num_sites, "num_sites"), fit)
    return pca(op, k, oversample, iterations, seed)
