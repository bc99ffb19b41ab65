"""PC-Relate: the ancestry-adjusted kinship of every pair of a block (Conomos et al. 2016;
GENESIS ``pcrelate``, ``hl.pc_relate``), the step behind ``pca`` in PC-AiR / PC-Relate.
include/cuking_amd.h "PC-Relate" holds the definition of the matrix; this module fits the
model it needs on existing primitives and wraps the kernel call.

Fit (``isaf_fit``).  ``X = [1, scores]`` float32 ``[num_stored, d]``.  With the genotype counts
of the FIT rows (``site_counts``), ``p = alt / (2 called)``; a site is USED iff ``called > 0`` and
``0 < p < 1`` (``hwe_table``).  The per-site regression of the fit rows' genotypes (missing =
``2p``, mean imputation; an unused site all zeros) on ``X_fit``: ``XtG = G^T X_fit`` is one
``geno_matmul`` over ``transpose_sites`` of the fit rows with the per-row table ``[0, 1, 2, 2p]``,
``beta = XtG (X_fit^T X_fit)^-1`` solved in float64 and stored as float32 ``[num_sites, d]``.
The rows of unused sites are zero, so ``mu = 0`` there and the site is invalid for everybody.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import check
from .api import Submatrix, _count, _geno_host_matrix, geno_matmul_host
from .pca import DeviceOperator, HostOperator

COLUMNS_MAX = _lib.PCRELATE_COLUMNS_MAX


@dataclass
class PCRelateResult:
    """What ``KingContext.pcrelate`` / ``pcrelate_host`` return: ``kin`` (float32 ``[rows,
    cols]`` of the block: a device tensor, or a host array from the host twin), ``beta``
    (float32 ``[num_sites, d]``, host), ``sites_used`` (bool ``[num_sites]``), ``fit`` (bool
    ``[num_stored]``), ``x`` (float32 ``[num_stored, d]``, host: ``[1, scores]``) and ``block``
    (the ``Submatrix``)."""
    kin: object
    beta: np.ndarray
    sites_used: np.ndarray
    fit: np.ndarray
    x: np.ndarray
    block: Submatrix

    def inbreeding(self) -> np.ndarray:
        """``2 kin(i, i) - 1`` of a diagonal block's samples, as a host array."""
        if self.block.i_begin != self.block.j_begin:
            raise ValueError(f"inbreeding() needs a diagonal block, not {self.block!r}")
        kin = self.kin if isinstance(self.kin, np.ndarray) else self.kin.cpu().numpy()
        return 2.0 * np.diagonal(kin) - 1.0


def design_matrix(scores, num_stored: int) -> np.ndarray:
    """``[1, scores]`` as float32 ``[num_stored, 1 + k]`` on the host."""
    if not isinstance(scores, np.ndarray):
        scores = scores.detach().cpu().numpy()
    if scores.dtype != np.float32 or scores.ndim != 2 or scores.shape[0] != num_stored:
        raise ValueError(f"scores must be float32 [{num_stored}, k], not "
                         f"{scores.dtype} {scores.shape}")
    d = scores.shape[1] + 1
    if d > COLUMNS_MAX:
        raise ValueError(f"pcrelate: 1 + {scores.shape[1]} score columns = {d} exceeds "
                         f"{COLUMNS_MAX}")
    return np.concatenate([np.ones((num_stored, 1), dtype=np.float32), scores], axis=1)


def isaf_table(used: np.ndarray, p: np.ndarray) -> np.ndarray:
    """The per-site table of the regression's genotypes: float32 ``[num_sites, 4]`` rows ``[0,
    1, 2, 2p]`` (missing = the mean), four zeros for an unused site."""
    table = np.zeros((used.shape[0], 4), dtype=np.float64)
    table[used, 1], table[used, 2], table[used, 3] = 1.0, 2.0, 2.0 * p[used]
    return table.astype(np.float32)


class HostIsafOperator(HostOperator):
    """The fit rows' site-major bitset and ``G^T A`` on ``geno_matmul_host``."""

    def xtg(self, table, a):
        return geno_matmul_host(self.site_bits, self.q2, self.n_fit,
                                np.ascontiguousarray(table), self.from_host(a), per_row=True)


class DeviceIsafOperator(DeviceOperator):
    """The fit rows' site-major bitset and ``G^T A`` on ``KingContext.geno_matmul``."""

    def xtg(self, table, a):
        return self.ctx.geno_matmul(self.site_bits, self.q2, self.n_fit, self.from_host(table),
                                    self.from_host(a), per_row=True)


def isaf_fit(op, scores):
    """The individual-specific allele frequency model over an operator (``HostIsafOperator``,
    ``DeviceIsafOperator``): returns ``(x, beta, used)`` as host arrays, ``x = [1, scores]``
    float32 ``[num_stored, d]`` and ``beta`` float32 ``[num_sites, d]`` (the module docstring
    has the definition).  ValueError: ``X_fit^T X_fit`` of rank below ``d``, fewer than ``d + 1``
    fit samples, no used site."""
    x = design_matrix(scores, op.fit.shape[0])
    d = x.shape[1]
    if op.n_fit < d + 1:
        raise ValueError(f"pcrelate: {op.n_fit} fit samples, at least d + 1 = {d + 1} are needed")
    num_used = int(op.used.sum())
    if num_used < 1:
        raise ValueError("pcrelate: no used site (0 sites with a called genotype and 0 < p < 1 "
                         "among the fit samples)")
    x_fit = np.ascontiguousarray(x[op.fit])
    x64 = x_fit.astype(np.float64)
    gram = x64.T @ x64
    rank = int(np.linalg.matrix_rank(gram))
    if rank < d:
        raise ValueError(f"pcrelate: X_fit^T X_fit has rank {rank}, below d = {d}")
    xtg = op.to_host64(op.xtg(isaf_table(op.used, op.p), x_fit))   # [num_sites, d]
    beta = np.linalg.solve(gram, xtg.T).T.astype(np.float32)
    beta[~op.used] = 0.0
    return x, np.ascontiguousarray(beta), op.used


def _bounds(min_maf) -> tuple:
    min_maf = float(min_maf)
    if not 0.0 <= min_maf < 0.5:
        raise ValueError(f"pcrelate: min_maf = {min_maf} must be in [0, 0.5)")
    return float(np.float32(min_maf)), float(np.float32(1.0) - np.float32(min_maf))


def _block(block, num_stored: int) -> Submatrix:
    if block is None:
        return Submatrix.from_ranges(0, num_stored, 0, num_stored)
    if not isinstance(block, Submatrix):
        block = Submatrix.from_ranges(*(_count(v, "block") for v in block))
    return block


def pcrelate_matrix_host(bits: np.ndarray, words_per_sample: int, num_sites: int, x, beta,
                         lo: float, hi: float, block=None, out=None) -> np.ndarray:
    """cuking_pcrelate_matrix_host: the kinship of every pair of ``block`` (a ``Submatrix`` or
    ``(i_begin, i_end, j_begin, j_end)`` over the stored samples; None = all) from the host
    bitset, ``x`` float32 ``[num_stored, d]`` and ``beta`` float32 ``[>= num_sites, d]``; sums in
    double, rounded once, divided in float32: the specification of
    ``KingContext.pcrelate_matrix`` in executable form.  ``out``: float32 ``[rows, cols]`` to
    write into (may be a column slice of a wider array)."""
    assert bits.dtype == np.uint64 and bits.flags.c_contiguous
    words_per_sample = _count(words_per_sample, "words_per_sample")
    num_sites = _count(num_sites, "num_sites")
    num_stored = bits.size // words_per_sample if words_per_sample else 0
    x = _geno_host_matrix(x, "x", num_stored)
    beta = _geno_host_matrix(beta, "beta", num_sites, x.shape[1])
    block = _block(block, num_stored)
    rows, cols = block.i_end - block.i_begin, block.j_end - block.j_begin
    if out is None:
        out = np.empty((max(rows, 0), max(cols, 0)), dtype=np.float32)
    else:
        _geno_host_matrix(out, "out", rows, cols)
    d = x.shape[1]
    pad = np.zeros(4, dtype=np.float32)
    check(_lib.load().cuking_pcrelate_matrix_host(
        (bits if bits.size else pad).ctypes.data, num_stored, words_per_sample, num_sites,
        (x if x.size else pad).ctypes.data, max(x.strides[0] // 4, d),
        (beta if beta.size else pad).ctypes.data, max(beta.strides[0] // 4, d), d, lo, hi,
        C.byref(block.c), (out if out.size else pad).ctypes.data,
        max(out.strides[0] // 4, cols)))
    return out


def pcrelate_host(bits: np.ndarray, words_per_sample: int, num_sites: int, scores, fit=None,
                  min_maf: float = 0.01, block=None, out=None) -> PCRelateResult:
    """``KingContext.pcrelate`` on host memory and the host twins: no GPU."""
    lo, hi = _bounds(min_maf)
    op = HostIsafOperator(bits, _count(words_per_sample, "words_per_sample"),
                          _count(num_sites, "num_sites"), fit)
    x, beta, used = isaf_fit(op, scores)
    block = _block(block, op.bits.shape[0])
    kin = pcrelate_matrix_host(bits, words_per_sample, num_sites, x, beta, lo, hi, block, out)
    return PCRelateResult(kin, beta, used, op.fit, x, block)


def pcrelate_matrix_device(ctx, bits, words_per_sample: int, num_sites: int, x, beta, lo: float,
                           hi: float, block=None, out=None, stream=None):
    import torch
    from .api import _device_tensor, _stream_handle
    num_stored = ctx._rows_of(bits, words_per_sample)
    num_sites = _count(num_sites, "num_sites")
    x = ctx._geno_matrix(x, "x", num_stored)
    d = x.shape[1]
    beta = ctx._geno_matrix(beta, "beta", num_sites, d)
    block = _block(block, num_stored)
    rows, cols = block.i_end - block.i_begin, block.j_end - block.j_begin
    if out is None:
        out = torch.empty((max(rows, 0), max(cols, 0)), dtype=torch.float32,
                          device=f"cuda:{ctx.device}")
    else:
        _device_tensor(ctx.device, out, "out", torch.float32, shape=(rows, cols),
                       contiguous=False)
        if rows > 1 and cols > 0 and out.stride(0) < cols or cols > 1 and out.stride(1) != 1:
            raise ValueError("out must have unit column stride and a row stride of at least "
                             "the block's columns")
    ldo = out.stride(0) if rows > 1 else max(out.stride(0), cols)
    check(ctx.lib.cuking_pcrelate_matrix(
        ctx.handle, bits.data_ptr(), num_stored, words_per_sample, num_sites, x.data_ptr(),
        max(x.stride(0), d), beta.data_ptr(), max(beta.stride(0), d), d, lo, hi,
        C.byref(block.c), out.data_ptr(), ldo, _stream_handle(stream)))
    return out


def pcrelate_device(ctx, bits, words_per_sample: int, num_sites: int, scores, fit=None,
                    min_maf: float = 0.01, block=None, out=None, stream=None) -> PCRelateResult:
    import torch
    lo, hi = _bounds(min_maf)
    op = DeviceIsafOperator(ctx, bits, _count(words_per_sample, "words_per_sample"),
                            _count(num_sites, "num_sites"), fit)
    x, beta, used = isaf_fit(op, scores)
    block = _block(block, op.bits.shape[0])
    # (the fit ran on the current stream: `stream` waits for it and for the two copies)
    d_x, d_beta = op.from_host(x), op.from_host(beta)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    kin = pcrelate_matrix_device(ctx, bits, words_per_sample, num_sites, d_x, d_beta, lo, hi,
                                 block, out, stream)
    if stream is not None:  # (d_x and d_beta are freed when this returns)
        d_x.record_stream(stream)
        d_beta.record_stream(stream)
    return PCRelateResult(kin, beta, used, op.fit, x, block)
