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

Listed pairs (``pcrelate_pairs``; include/cuking_amd.h "PC-Relate for listed pairs" holds the
definition).  The same model evaluated on a list of pairs -- the records of ``compute_king`` or
an int ``[P, 2]`` array -- gives ``kin``, ``k0``, ``k1``, ``k2``, ``ibs0`` and ``sites`` per
pair without a matrix; the inbreeding coefficients its ``k2`` needs come from the self pairs
``(s, s)``: ``f = 2 kin(s, s) - 1``.

Records (``pcrelate_records``; include/cuking_amd.h "PC-Relate records" holds the definition).
The pairs of a block with ``kin > min_kinship`` as the records ``compute_king`` writes, without
a matrix: the list ``pcrelate_pairs`` and ``unrelated_set`` take, drawn from the ancestry-adjusted
kinship itself.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import check
from .api import (KING_CUTOFFS, KING_RESULT_DTYPE, Submatrix, _count, _counted_buffer,
                  _geno_host_matrix, _out_capacity, geno_matmul_host)
from .pca import DeviceOperator, HostOperator

COLUMNS_MAX = _lib.PCRELATE_COLUMNS_MAX
# cuking_pcrelate_pair
PCRELATE_PAIR_DTYPE = np.dtype(
    [("sample_i", "<u4"), ("sample_j", "<u4"), ("kin", "<f4"), ("k0", "<f4"), ("k1", "<f4"),
     ("k2", "<f4"), ("ibs0", "<u4"), ("sites", "<u4")])
# The codes of PCRelatePairs.relationship()
UNRELATED, THIRD_DEGREE, SECOND_DEGREE, FULL_SIBLING, PARENT_CHILD, DUPLICATE = range(6)
RELATIONSHIP_NAMES = ("unrelated", "3rd degree", "2nd degree", "full sibling", "parent-child",
                      "duplicate/MZ")


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


# ---- listed pairs ------------------------------------------------------------------------------

@dataclass
class PCRelatePairs:
    """What ``KingContext.pcrelate_pairs`` / ``pcrelate_pairs_host`` return, as host arrays:
    ``rows`` (``PCRELATE_PAIR_DTYPE`` ``[P]``, the output rows in input order) and its fields
    ``sample_i``, ``sample_j`` (uint32, as given), ``kin``, ``k0``, ``k1``, ``k2`` (float32),
    ``ibs0``, ``sites`` (uint32: counts over the jointly valid sites); ``inbreeding`` (float32
    ``[num_stored]``, the ``f`` the call used); and the model: ``beta``, ``sites_used``, ``fit``,
    ``x`` as in ``PCRelateResult``."""
    rows: np.ndarray
    inbreeding: np.ndarray
    beta: np.ndarray
    sites_used: np.ndarray
    fit: np.ndarray
    x: np.ndarray

    sample_i = property(lambda self: self.rows["sample_i"])
    sample_j = property(lambda self: self.rows["sample_j"])
    kin = property(lambda self: self.rows["kin"])
    k0 = property(lambda self: self.rows["k0"])
    k1 = property(lambda self: self.rows["k1"])
    k2 = property(lambda self: self.rows["k2"])
    ibs0 = property(lambda self: self.rows["ibs0"])
    sites = property(lambda self: self.rows["sites"])

    def relationship(self, thresholds=KING_CUTOFFS, parent_child_k0: float = 0.1) -> np.ndarray:
        """One code per pair (uint8; ``RELATIONSHIP_NAMES[code]``): ``UNRELATED``,
        ``THIRD_DEGREE``, ``SECOND_DEGREE``, ``FULL_SIBLING``, ``PARENT_CHILD``, ``DUPLICATE``.
        On the host in numpy.  The degree is the number of the four ascending ``thresholds``
        that ``kin`` exceeds, in the strict float32 comparison ``kin > t`` the relative counts
        use (a NaN exceeds none: unrelated); first degree is parent-child where ``k0 <
        parent_child_k0`` (strict float32; false for a NaN) and full siblings otherwise.  The
        0.1 is a convention -- a parent and a child share an allele at every site, siblings at
        three sites in four --, an argument and not a measured value."""
        thr = np.asarray(thresholds, dtype=np.float32)
        if thr.shape != (4,) or not (np.diff(thr) > 0).all():
            raise ValueError(f"thresholds must be four ascending values, not {thresholds!r}")
        with np.errstate(invalid="ignore"):
            degree = (self.kin[:, None] > thr[None, :]).sum(axis=1)
            parent = self.k0 < np.float32(parent_child_k0)
        code = np.array([UNRELATED, THIRD_DEGREE, SECOND_DEGREE, FULL_SIBLING, DUPLICATE],
                        dtype=np.uint8)[degree]
        code[(degree == 3) & parent] = PARENT_CHILD
        return code


def _host_pairs(pairs, num_records=None):
    """(array that owns the memory, pointer, count, stride in bytes) of a host pair list:
    ``KING_RESULT_DTYPE`` records or ``[*, 6]`` int32 / uint32 (the first ``num_records``;
    stride 24), or an integer ``[P, 2]`` array (stride 8)."""
    pairs = np.asarray(pairs)
    if pairs.dtype == KING_RESULT_DTYPE and pairs.ndim == 1 or \
            pairs.ndim == 2 and pairs.shape[1] == 6 and pairs.dtype in (np.int32, np.uint32):
        recs = np.ascontiguousarray(pairs)
        count = recs.shape[0] if num_records is None else _count(num_records, "num_records")
        if count > recs.shape[0]:
            raise ValueError(f"pairs holds {recs.shape[0]} records, num_records is {count}")
        return recs, recs.ctypes.data, count, 24
    if num_records is not None:
        raise ValueError("num_records goes with a record buffer, not with a [P, 2] array")
    if pairs.ndim != 2 or pairs.shape[1] != 2 or pairs.dtype.kind not in "iu":
        raise ValueError("pairs must be KING_RESULT_DTYPE records, [*, 6] int32 / uint32 records "
                         f"or an integer [P, 2] array, not {pairs.dtype} {pairs.shape}")
    if pairs.size and (int(pairs.min()) < 0 or int(pairs.max()) > 0xFFFFFFFF):
        raise ValueError("pairs must hold sample indices in [0, 2^32)")
    flat = np.ascontiguousarray(pairs, dtype=np.uint32)
    return flat, flat.ctypes.data, flat.shape[0], 8


def _pair_indices(owner, count: int, stride: int) -> np.ndarray:
    """uint32 ``[count, 2]`` of what ``_host_pairs`` returned."""
    if stride == 8:
        return owner[:count]
    if owner.dtype == KING_RESULT_DTYPE:
        return np.stack([owner["sample_i"][:count], owner["sample_j"][:count]], axis=1)
    return owner[:count, :2].view(np.uint32) if owner.dtype == np.int32 else owner[:count, :2]


def _check_pair_range(indices, num_stored: int):
    if indices.size and int(indices.max()) >= num_stored:
        bad = int(np.argmax((indices >= num_stored).any(axis=1)))
        raise ValueError(f"pcrelate pairs: pair {bad} = ({int(indices[bad, 0])}, "
                         f"{int(indices[bad, 1])}) is outside the {num_stored} stored samples")


def _host_inbreeding(f, num_stored: int):
    if f is None:
        return None
    f = np.ascontiguousarray(f)
    if f.dtype != np.float32 or f.shape != (num_stored,):
        raise ValueError(f"inbreeding must be float32 [{num_stored}], not {f.dtype} {f.shape}")
    return f


def pcrelate_pairs_raw_host(bits: np.ndarray, words_per_sample: int, num_sites: int, x, beta,
                            lo: float, hi: float, pairs, f=None, num_records=None) -> np.ndarray:
    """cuking_pcrelate_pairs_host, the bare call: one ``PCRELATE_PAIR_DTYPE`` row per pair of
    ``pairs`` (records with ``num_records``, or an integer ``[P, 2]`` array), from the host
    bitset, ``x`` float32 ``[num_stored, d]``, ``beta`` float32 ``[>= num_sites, d]`` and ``f``
    float32 ``[num_stored]`` (None = all zero).  The same float32 chains as the kernel: bit for
    bit what ``KingContext.pcrelate_pairs_raw`` gives.  An index outside the stored samples is
    not an error here: its row holds NaN."""
    assert bits.dtype == np.uint64 and bits.flags.c_contiguous
    words_per_sample = _count(words_per_sample, "words_per_sample")
    num_sites = _count(num_sites, "num_sites")
    num_stored = bits.size // words_per_sample if words_per_sample else 0
    x = _geno_host_matrix(x, "x", num_stored)
    beta = _geno_host_matrix(beta, "beta", num_sites, x.shape[1])
    f = _host_inbreeding(f, num_stored)
    owner, ptr, count, stride = _host_pairs(pairs, num_records)
    out = np.empty(count, dtype=PCRELATE_PAIR_DTYPE)
    d = x.shape[1]
    pad = np.zeros(4, dtype=np.float32)
    check(_lib.load().cuking_pcrelate_pairs_host(
        (bits if bits.size else pad).ctypes.data, num_stored, words_per_sample, num_sites,
        (x if x.size else pad).ctypes.data, max(x.strides[0] // 4, d),
        (beta if beta.size else pad).ctypes.data, max(beta.strides[0] // 4, d), d, lo, hi,
        None if f is None else (f if f.size else pad).ctypes.data, ptr if count else None, count,
        stride, out.ctypes.data if count else None))
    return out


def _self_pairs(num_stored: int) -> np.ndarray:
    s = np.arange(num_stored, dtype=np.uint32)
    return np.ascontiguousarray(np.stack([s, s], axis=1))


def _inbreeding_of(self_rows: np.ndarray) -> np.ndarray:
    """``f = 2 kin(s, s) - 1`` in float32 (a NaN stays NaN)."""
    return np.float32(2.0) * self_rows["kin"] - np.float32(1.0)


def _model_of(model):
    for name in ("x", "beta", "sites_used", "fit"):
        if not hasattr(model, name):
            raise ValueError("model must be a PCRelateResult, PCRelateRecords or PCRelatePairs, not "
                             f"{type(model).__name__}")
    return model.x, model.beta, model.sites_used, model.fit


def pcrelate_pairs_host(bits: np.ndarray, words_per_sample: int, num_sites: int, pairs,
                        scores=None, model=None, fit=None, min_maf: float = 0.01,
                        inbreeding=None, num_records=None) -> PCRelatePairs:
    """``KingContext.pcrelate_pairs`` on host memory and the host twins: no GPU."""
    lo, hi = _bounds(min_maf)
    words_per_sample = _count(words_per_sample, "words_per_sample")
    num_sites = _count(num_sites, "num_sites")
    if (scores is None) == (model is None):
        raise ValueError("pcrelate pairs: give either scores or model")
    if model is not None:
        x, beta, used, fit_mask = _model_of(model)
    else:
        op = HostIsafOperator(bits, words_per_sample, num_sites, fit)
        x, beta, used = isaf_fit(op, scores)
        fit_mask = op.fit
    num_stored = bits.size // words_per_sample if words_per_sample else 0
    owner, _, count, stride = _host_pairs(pairs, num_records)
    _check_pair_range(_pair_indices(owner, count, stride), num_stored)
    if inbreeding is None:
        f = _inbreeding_of(pcrelate_pairs_raw_host(bits, words_per_sample, num_sites, x, beta,
                                                   lo, hi, _self_pairs(num_stored)))
    else:
        f = _host_inbreeding(inbreeding, num_stored)
    rows = pcrelate_pairs_raw_host(bits, words_per_sample, num_sites, x, beta, lo, hi, owner, f,
                                   count if stride == 24 else None)
    return PCRelatePairs(rows, f, beta, used, fit_mask, x)


def pairs_to_host(rows) -> np.ndarray:
    """The ``[P, 8]`` int32 device tensor of ``pcrelate_pairs_raw`` as ``PCRELATE_PAIR_DTYPE``
    rows on the host (waits for the copy)."""
    return np.ascontiguousarray(rows.cpu().numpy()).view(PCRELATE_PAIR_DTYPE).reshape(-1)


def _device_pairs(ctx, pairs, num_records=None):
    """(tensor that owns the memory, count, stride in bytes) of a pair list on the device: an
    int32 ``[*, 6]`` record tensor (the first ``num_records``), an int32 / int64 ``[P, 2]``
    tensor, or one of the host forms of ``_host_pairs``, uploaded."""
    import torch
    dev = f"cuda:{ctx.device}"
    if not isinstance(pairs, torch.Tensor):
        owner, _, count, stride = _host_pairs(pairs, num_records)
        flat = np.ascontiguousarray(owner).view(np.int32).reshape(owner.shape[0], stride // 4)
        return torch.from_numpy(flat).to(dev), count, stride
    if not pairs.is_cuda or pairs.device.index != ctx.device:
        raise ValueError("pairs must live on this context's GPU")
    if pairs.dim() == 2 and pairs.shape[1] == 6 and pairs.dtype == torch.int32:
        count = pairs.shape[0] if num_records is None else _count(num_records, "num_records")
        if count > pairs.shape[0]:
            raise ValueError(f"pairs holds {pairs.shape[0]} records, num_records is {count}")
        return pairs.contiguous(), count, 24
    if num_records is not None:
        raise ValueError("num_records goes with a record buffer, not with a [P, 2] tensor")
    if pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.dtype not in (torch.int32, torch.int64):
        raise ValueError("pairs must be an int32 [*, 6] record tensor or an int32 / int64 "
                         f"[P, 2] tensor, not {pairs.dtype} {tuple(pairs.shape)}")
    if pairs.dtype == torch.int64:
        if pairs.numel() and (int(pairs.min()) < 0 or int(pairs.max()) > 0xFFFFFFFF):
            raise ValueError("pairs must hold sample indices in [0, 2^32)")
        pairs = pairs.to(torch.int32)   # (wraps: the low 32 bits are the uint32)
    return pairs.contiguous(), pairs.shape[0], 8


def pcrelate_pairs_raw_device(ctx, bits, words_per_sample: int, num_sites: int, x, beta,
                              lo: float, hi: float, pairs, f=None, num_records=None, out=None,
                              stream=None):
    import torch
    from .api import _device_tensor, _stream_handle
    num_stored = ctx._rows_of(bits, words_per_sample)
    num_sites = _count(num_sites, "num_sites")
    x = ctx._geno_matrix(x, "x", num_stored)
    d = x.shape[1]
    beta = ctx._geno_matrix(beta, "beta", num_sites, d)
    if f is not None:
        _device_tensor(ctx.device, f, "f", torch.float32, shape=(num_stored,))
    owner, count, stride = _device_pairs(ctx, pairs, num_records)
    if out is None:
        out = torch.empty((count, 8), dtype=torch.int32, device=f"cuda:{ctx.device}")
    else:
        _device_tensor(ctx.device, out, "out", torch.int32, shape=(count, 8))
    check(ctx.lib.cuking_pcrelate_pairs(
        ctx.handle, bits.data_ptr(), num_stored, words_per_sample, num_sites, x.data_ptr(),
        max(x.stride(0), d), beta.data_ptr(), max(beta.stride(0), d), d, lo, hi,
        None if f is None else f.data_ptr(), owner.data_ptr() if count else None, count, stride,
        out.data_ptr() if count else None, _stream_handle(stream)))
    if stream is not None and owner is not pairs:  # (a converted copy is freed on return)
        owner.record_stream(stream)
    return out


def pcrelate_pairs_device(ctx, bits, words_per_sample: int, num_sites: int, pairs, scores=None,
                          model=None, fit=None, min_maf: float = 0.01, inbreeding=None,
                          num_records=None, stream=None) -> PCRelatePairs:
    import torch
    lo, hi = _bounds(min_maf)
    words_per_sample = _count(words_per_sample, "words_per_sample")
    num_sites = _count(num_sites, "num_sites")
    if (scores is None) == (model is None):
        raise ValueError("pcrelate pairs: give either scores or model")
    num_stored = ctx._rows_of(bits, words_per_sample)
    dev = f"cuda:{ctx.device}"
    if model is not None:
        x, beta, used, fit_mask = _model_of(model)
    else:
        op = DeviceIsafOperator(ctx, bits, words_per_sample, num_sites, fit)
        x, beta, used = isaf_fit(op, scores)
        fit_mask = op.fit
    owner, count, stride = _device_pairs(ctx, pairs, num_records)
    index = owner[:count, :2]
    if count and bool(((index < 0) | (index >= num_stored)).any()):   # (int32: < 0 is >= 2^31)
        _check_pair_range(index.cpu().numpy().view(np.uint32), num_stored)
    d_x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
    d_beta = torch.from_numpy(np.ascontiguousarray(beta, dtype=np.float32)).to(dev)
    # (the fit and the copies ran on the current stream: `stream` waits for them)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    args = (ctx, bits, words_per_sample, num_sites, d_x, d_beta, lo, hi)
    if inbreeding is None:
        selfs = pcrelate_pairs_raw_device(*args, _self_pairs(num_stored), stream=stream)
        if stream is not None:
            stream.synchronize()
        f = _inbreeding_of(pairs_to_host(selfs))
    else:
        f = _host_inbreeding(inbreeding, num_stored)
    d_f = torch.from_numpy(f).to(dev)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    rows = pcrelate_pairs_raw_device(*args, owner, d_f, count if stride == 24 else None,
                                     stream=stream)
    if stream is not None:
        stream.synchronize()
    return PCRelatePairs(pairs_to_host(rows), f, beta, used, fit_mask, x)


# ---- records: the pairs above a kinship threshold ----------------------------------------------

@dataclass
class PCRelateRecords:
    """What ``KingContext.pcrelate_records`` / ``pcrelate_records_host`` return: ``records``
    (the first ``num_records`` rows are the pairs with ``kin > min_kinship``, ``sample_i <
    sample_j``, in no particular order: the int32 ``[*, 6]`` device tensor ``unrelated_set`` and
    ``pcrelate_pairs`` take, or ``KING_RESULT_DTYPE`` rows from the host twin), ``num_records``,
    ``min_kinship``, ``block`` and the model: ``beta``, ``sites_used``, ``fit``, ``x`` as in
    ``PCRelateResult`` -- which makes the object the ``model`` argument of ``pcrelate_pairs``."""
    records: object
    num_records: int
    min_kinship: float
    block: Submatrix
    beta: np.ndarray
    sites_used: np.ndarray
    fit: np.ndarray
    x: np.ndarray

    def sorted(self) -> np.ndarray:
        """The records as ``KING_RESULT_DTYPE`` rows on the host, by ``(sample_i, sample_j)``
        (a copy; waits for it)."""
        return records_to_host(self.records, self.num_records)


def records_to_host(records, num_records: int) -> np.ndarray:
    """The first ``num_records`` rows of a record buffer (the ``[*, 6]`` int32 device tensor or
    host ``KING_RESULT_DTYPE`` rows) as sorted ``KING_RESULT_DTYPE`` rows on the host."""
    from .api import sort_results
    if isinstance(records, np.ndarray):
        rows = records[:num_records].copy()
    else:
        rows = np.ascontiguousarray(records[:num_records].cpu().numpy()) \
            .view(KING_RESULT_DTYPE).reshape(-1).copy()
    return sort_results(rows)


def _min_kin(min_kin) -> float:
    min_kin = float(np.float32(min_kin))
    if min_kin != min_kin:
        raise ValueError("pcrelate records: min_kin must not be NaN")
    return min_kin


def _default_records(block: Submatrix) -> int:
    """The buffer of a call without ``max_records``: 16 records per sample of the block, at
    most its pairs (the call is repeated once with the exact count if that overflows)."""
    rows, cols = max(block.i_end - block.i_begin, 0), max(block.j_end - block.j_begin, 0)
    pairs = rows * (rows - 1) // 2 if block.i_begin == block.j_begin else rows * cols
    return max(1, min(pairs, 16 * (rows + cols)))


def pcrelate_records_raw_host(bits: np.ndarray, words_per_sample: int, num_sites: int, x, beta,
                              lo: float, hi: float, min_kin: float, block=None,
                              max_records=None):
    """cuking_pcrelate_records_host, the bare call: the pairs of ``block`` (as
    ``pcrelate_matrix_host`` takes it) with ``kin > min_kin`` as ``(records, count)``,
    ``KING_RESULT_DTYPE`` rows in ascending ``(sample_i, sample_j)`` with the kinship bytes of
    ``pcrelate_matrix_host``.  The buffer rule is ``ld_edges_host``'s: without ``max_records`` a
    default buffer, grown once to the exact count; with it, an overflow raises
    ``ResourceExhaustedError`` whose ``num_records`` is the exact count."""
    assert bits.dtype == np.uint64 and bits.flags.c_contiguous
    words_per_sample = _count(words_per_sample, "words_per_sample")
    num_sites = _count(num_sites, "num_sites")
    num_stored = bits.size // words_per_sample if words_per_sample else 0
    x = _geno_host_matrix(x, "x", num_stored)
    beta = _geno_host_matrix(beta, "beta", num_sites, x.shape[1])
    block = _block(block, num_stored)
    min_kin = _min_kin(min_kin)
    d = x.shape[1]
    pad = np.zeros(4, dtype=np.float32)
    count = C.c_uint64(0)

    def call(capacity):
        recs = np.zeros(max(capacity, 1), dtype=KING_RESULT_DTYPE)
        status = _lib.load().cuking_pcrelate_records_host(
            (bits if bits.size else pad).ctypes.data, num_stored, words_per_sample, num_sites,
            (x if x.size else pad).ctypes.data, max(x.strides[0] // 4, d),
            (beta if beta.size else pad).ctypes.data, max(beta.strides[0] // 4, d), d, lo, hi,
            C.byref(block.c), min_kin, recs.ctypes.data, capacity, C.byref(count))
        return recs, status

    recs = _counted_buffer(call, _default_records(block), max_records, "max_records", count,
                           "num_records")
    return recs[:count.value].copy(), int(count.value)


def pcrelate_records_host(bits: np.ndarray, words_per_sample: int, num_sites: int, scores=None,
                          model=None, fit=None, min_maf: float = 0.01,
                          min_kinship: float = KING_CUTOFFS[0], block=None,
                          max_records=None) -> PCRelateRecords:
    """``KingContext.pcrelate_records`` on host memory and the host twins: no GPU."""
    lo, hi = _bounds(min_maf)
    words_per_sample = _count(words_per_sample, "words_per_sample")
    num_sites = _count(num_sites, "num_sites")
    if (scores is None) == (model is None):
        raise ValueError("pcrelate records: give either scores or model")
    if model is not None:
        x, beta, used, fit_mask = _model_of(model)
    else:
        op = HostIsafOperator(bits, words_per_sample, num_sites, fit)
        x, beta, used = isaf_fit(op, scores)
        fit_mask = op.fit
    block = _block(block, bits.size // words_per_sample if words_per_sample else 0)
    recs, count = pcrelate_records_raw_host(bits, words_per_sample, num_sites, x, beta, lo, hi,
                                            min_kinship, block, max_records)
    return PCRelateRecords(recs, count, _min_kin(min_kinship), block, beta, used, fit_mask, x)


def pcrelate_records_raw_device(ctx, bits, words_per_sample: int, num_sites: int, x, beta,
                                lo: float, hi: float, min_kin: float, block=None,
                                max_records=None, out=None, stream=None):
    import torch
    from .api import _device_tensor, _stream_handle
    num_stored = ctx._rows_of(bits, words_per_sample)
    num_sites = _count(num_sites, "num_sites")
    x = ctx._geno_matrix(x, "x", num_stored)
    d = x.shape[1]
    beta = ctx._geno_matrix(beta, "beta", num_sites, d)
    block = _block(block, num_stored)
    min_kin = _min_kin(min_kin)
    dev = f"cuda:{ctx.device}"
    if out is not None:
        _device_tensor(ctx.device, out, "out", torch.int32, cols=6)
        max_records = _out_capacity(out, max_records)
    count = C.c_uint64(0)

    def call(capacity):
        records = out if out is not None else torch.empty((max(capacity, 1), 6),
                                                          dtype=torch.int32, device=dev)
        return records, ctx.lib.cuking_pcrelate_records(
            ctx.handle, bits.data_ptr(), num_stored, words_per_sample, num_sites, x.data_ptr(),
            max(x.stride(0), d), beta.data_ptr(), max(beta.stride(0), d), d, lo, hi,
            C.byref(block.c), min_kin, records.data_ptr() if capacity else None, capacity,
            C.byref(count), _stream_handle(stream))

    records = _counted_buffer(call, _default_records(block), max_records, "max_records", count,
                              "num_records")
    return records, int(count.value)


def pcrelate_records_device(ctx, bits, words_per_sample: int, num_sites: int, scores=None,
                            model=None, fit=None, min_maf: float = 0.01,
                            min_kinship: float = KING_CUTOFFS[0], block=None,
                            max_records=None) -> PCRelateRecords:
    import torch
    lo, hi = _bounds(min_maf)
    words_per_sample = _count(words_per_sample, "words_per_sample")
    num_sites = _count(num_sites, "num_sites")
    if (scores is None) == (model is None):
        raise ValueError("pcrelate records: give either scores or model")
    dev = f"cuda:{ctx.device}"
    if model is not None:
        x, beta, used, fit_mask = _model_of(model)
    else:
        op = DeviceIsafOperator(ctx, bits, words_per_sample, num_sites, fit)
        x, beta, used = isaf_fit(op, scores)
        fit_mask = op.fit
    block = _block(block, ctx._rows_of(bits, words_per_sample))
    d_x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
    d_beta = torch.from_numpy(np.ascontiguousarray(beta, dtype=np.float32)).to(dev)
    records, count = pcrelate_records_raw_device(ctx, bits, words_per_sample, num_sites, d_x,
                                                 d_beta, lo, hi, min_kinship, block, max_records)
    return PCRelateRecords(records, count, _min_kin(min_kinship), block, beta, used, fit_mask, x)
