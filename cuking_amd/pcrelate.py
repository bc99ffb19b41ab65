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
from ._place import HOST, DevicePlace, tensor_to_host
from .api import (KING_CUTOFFS, KING_RESULT_DTYPE, Submatrix, _count, _counted_buffer,
                  _out_capacity, geno_matmul_host)
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


def _model_head(place, bits, words_per_sample, num_sites, x, beta):
    """What the argument list of every PC-Relate call begins with, up to ``d``, as ``(head,
    num_stored)``: the bitset, ``x`` float32 ``[num_stored, d]`` and ``beta`` float32 ``[>=
    num_sites, d]`` with their leading dimensions."""
    words_per_sample = _count(words_per_sample, "words_per_sample")
    num_sites = _count(num_sites, "num_sites")
    num_stored = place.bits(bits, words_per_sample)
    x, ldx = place.matrix(x, "x", num_stored)
    d = x.shape[1]
    beta, ldb = place.matrix(beta, "beta", num_sites, d)
    return (place.ptr(bits, pad=True), num_stored, words_per_sample, num_sites,
            place.ptr(x, pad=True), ldx, place.ptr(beta, pad=True), ldb, d), num_stored


def _fit_model(place, bits, words_per_sample, num_sites, scores, model, fit, what: str):
    """``(x, beta, used, fit)`` of ``model``, or fitted on ``scores`` and ``fit``."""
    if (scores is None) == (model is None):
        raise ValueError(f"pcrelate {what}: give either scores or model")
    if model is not None:
        return _model_of(model)
    op = place.isaf_operator(bits, words_per_sample, num_sites, fit)
    return (*isaf_fit(op, scores), op.fit)


def _pcrelate_matrix(place, bits, words_per_sample, num_sites, x, beta, lo, hi, block, out):
    head, num_stored = _model_head(place, bits, words_per_sample, num_sites, x, beta)
    block = _block(block, num_stored)
    rows, cols = block.i_end - block.i_begin, block.j_end - block.j_begin
    if out is None:
        out = place.alloc((max(rows, 0), max(cols, 0)), np.float32)
    out, ldo = place.matrix(out, "out", rows, cols)
    check(place.fn("pcrelate_matrix")(*head, lo, hi, C.byref(block.c), place.ptr(out, pad=True),
                                      ldo))
    return out


def _pcrelate(place, bits, words_per_sample, num_sites, scores, fit, min_maf, block, out):
    lo, hi = _bounds(min_maf)
    op = place.isaf_operator(bits, _count(words_per_sample, "words_per_sample"),
                             _count(num_sites, "num_sites"), fit)
    x, beta, used = isaf_fit(op, scores)
    block = _block(block, op.bits.shape[0])
    # (the fit ran on the current stream: `stream` waits for it and for the two copies, which
    # are freed when this returns)
    there = place.from_host(x), place.from_host(beta)
    place.uploads_done()
    kin = _pcrelate_matrix(place, bits, words_per_sample, num_sites, *there, lo, hi, block, out)
    place.keep()
    return PCRelateResult(kin, beta, used, op.fit, x, block)


def pcrelate_matrix_host(bits: np.ndarray, words_per_sample: int, num_sites: int, x, beta,
                         lo: float, hi: float, block=None, out=None) -> np.ndarray:
    """cuking_pcrelate_matrix_host: the kinship of every pair of ``block`` (a ``Submatrix`` or
    ``(i_begin, i_end, j_begin, j_end)`` over the stored samples; None = all) from the host
    bitset, ``x`` float32 ``[num_stored, d]`` and ``beta`` float32 ``[>= num_sites, d]``; sums in
    double, rounded once, divided in float32: the specification of
    ``KingContext.pcrelate_matrix`` in executable form.  ``out``: float32 ``[rows, cols]`` to
    write into (may be a column slice of a wider array)."""
    return _pcrelate_matrix(HOST, bits, words_per_sample, num_sites, x, beta, lo, hi, block, out)


def pcrelate_host(bits: np.ndarray, words_per_sample: int, num_sites: int, scores, fit=None,
                  min_maf: float = 0.01, block=None, out=None) -> PCRelateResult:
    """``KingContext.pcrelate`` on host memory and the host twins: no GPU."""
    return _pcrelate(HOST, bits, words_per_sample, num_sites, scores, fit, min_maf, block, out)


def pcrelate_matrix_device(ctx, bits, words_per_sample: int, num_sites: int, x, beta, lo: float,
                           hi: float, block=None, out=None, stream=None):
    return _pcrelate_matrix(DevicePlace(ctx, stream), bits, words_per_sample, num_sites, x, beta,
                            lo, hi, block, out)


def pcrelate_device(ctx, bits, words_per_sample: int, num_sites: int, scores, fit=None,
                    min_maf: float = 0.01, block=None, out=None, stream=None) -> PCRelateResult:
    return _pcrelate(DevicePlace(ctx, stream), bits, words_per_sample, num_sites, scores, fit,
                     min_maf, block, out)


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


def _check_pair_range(indices, num_stored: int):
    if indices.size and int(indices.max()) >= num_stored:
        bad = int(np.argmax((indices >= num_stored).any(axis=1)))
        raise ValueError(f"pcrelate pairs: pair {bad} = ({int(indices[bad, 0])}, "
                         f"{int(indices[bad, 1])}) is outside the {num_stored} stored samples")


def _pcrelate_pairs_raw(place, bits, words_per_sample, num_sites, x, beta, lo, hi, pairs, f,
                        num_records, out=None):
    head, num_stored = _model_head(place, bits, words_per_sample, num_sites, x, beta)
    if f is not None:
        f = place.vector(f, "inbreeding", np.float32, num_stored)
    owner, count, stride = place.pairs(pairs, num_records)
    out = place.alloc(count, PCRELATE_PAIR_DTYPE) if out is None else \
        place.out(out, "out", PCRELATE_PAIR_DTYPE, count)
    place.uploads_done()
    check(place.fn("pcrelate_pairs")(*head, lo, hi, place.ptr(f, pad=True),
                                     place.ptr(owner) if count else None, count, stride,
                                     place.ptr(out)))
    place.keep()
    return out


def pcrelate_pairs_raw_host(bits: np.ndarray, words_per_sample: int, num_sites: int, x, beta,
                            lo: float, hi: float, pairs, f=None, num_records=None) -> np.ndarray:
    """cuking_pcrelate_pairs_host, the bare call: one ``PCRELATE_PAIR_DTYPE`` row per pair of
    ``pairs`` (records with ``num_records``, or an integer ``[P, 2]`` array), from the host
    bitset, ``x`` float32 ``[num_stored, d]``, ``beta`` float32 ``[>= num_sites, d]`` and ``f``
    float32 ``[num_stored]`` (None = all zero).  The same float32 chains as the kernel: bit for
    bit what ``KingContext.pcrelate_pairs_raw`` gives.  An index outside the stored samples is
    not an error here: its row holds NaN."""
    return _pcrelate_pairs_raw(HOST, bits, words_per_sample, num_sites, x, beta, lo, hi, pairs, f,
                               num_records)


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


def _pcrelate_pairs(place, bits, words_per_sample, num_sites, pairs, scores, model, fit, min_maf,
                    inbreeding, num_records) -> PCRelatePairs:
    lo, hi = _bounds(min_maf)
    words_per_sample = _count(words_per_sample, "words_per_sample")
    num_sites = _count(num_sites, "num_sites")
    x, beta, used, fit_mask = _fit_model(place, bits, words_per_sample, num_sites, scores, model,
                                         fit, "pairs")
    num_stored = place.bits(bits, words_per_sample)
    owner, count, stride = place.pairs(pairs, num_records)
    _check_pair_range(place.pair_indices(owner, count, stride, num_stored), num_stored)
    args = (place, bits, words_per_sample, num_sites, place.from_host(x), place.from_host(beta),
            lo, hi)
    if inbreeding is None:
        selfs = _pcrelate_pairs_raw(*args, _self_pairs(num_stored), None, None)
        place.finish()
        f = _inbreeding_of(place.to_host(selfs, PCRELATE_PAIR_DTYPE))
    else:
        f = HOST.vector(inbreeding, "inbreeding", np.float32, num_stored)
    rows = _pcrelate_pairs_raw(*args, owner, place.from_host(f), count if stride == 24 else None)
    place.finish()
    return PCRelatePairs(place.to_host(rows, PCRELATE_PAIR_DTYPE), f, beta, used, fit_mask, x)


def pcrelate_pairs_host(bits: np.ndarray, words_per_sample: int, num_sites: int, pairs,
                        scores=None, model=None, fit=None, min_maf: float = 0.01,
                        inbreeding=None, num_records=None) -> PCRelatePairs:
    """``KingContext.pcrelate_pairs`` on host memory and the host twins: no GPU."""
    return _pcrelate_pairs(HOST, bits, words_per_sample, num_sites, pairs, scores, model, fit,
                           min_maf, inbreeding, num_records)


def pairs_to_host(rows) -> np.ndarray:
    """The ``[P, 8]`` int32 device tensor of ``pcrelate_pairs_raw`` as ``PCRELATE_PAIR_DTYPE``
    rows on the host (waits for the copy)."""
    return tensor_to_host(rows, PCRELATE_PAIR_DTYPE)


def pcrelate_pairs_raw_device(ctx, bits, words_per_sample: int, num_sites: int, x, beta,
                              lo: float, hi: float, pairs, f=None, num_records=None, out=None,
                              stream=None):
    return _pcrelate_pairs_raw(DevicePlace(ctx, stream), bits, words_per_sample, num_sites, x,
                               beta, lo, hi, pairs, f, num_records, out)


def pcrelate_pairs_device(ctx, bits, words_per_sample: int, num_sites: int, pairs, scores=None,
                          model=None, fit=None, min_maf: float = 0.01, inbreeding=None,
                          num_records=None, stream=None) -> PCRelatePairs:
    return _pcrelate_pairs(DevicePlace(ctx, stream), bits, words_per_sample, num_sites, pairs,
                           scores, model, fit, min_maf, inbreeding, num_records)


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
        rows = tensor_to_host(records[:num_records], KING_RESULT_DTYPE).copy()
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


def _pcrelate_records_raw(place, bits, words_per_sample, num_sites, x, beta, lo, hi, min_kin,
                          block, max_records, out=None):
    head, num_stored = _model_head(place, bits, words_per_sample, num_sites, x, beta)
    block = _block(block, num_stored)
    min_kin = _min_kin(min_kin)
    if out is not None:
        place.out(out, "out", KING_RESULT_DTYPE)
        max_records = _out_capacity(out, max_records)
    count = C.c_uint64(0)

    def call(capacity):
        recs = out if out is not None else place.alloc(max(capacity, 1), KING_RESULT_DTYPE)
        return recs, place.fn("pcrelate_records")(*head, lo, hi, C.byref(block.c), min_kin,
                                                  place.ptr(recs) if capacity else None,
                                                  capacity, C.byref(count))

    recs = _counted_buffer(call, _default_records(block), max_records, "max_records", count,
                           "num_records")
    return place.trim(recs, count.value), int(count.value)


def _pcrelate_records(place, bits, words_per_sample, num_sites, scores, model, fit, min_maf,
                      min_kinship, block, max_records) -> PCRelateRecords:
    lo, hi = _bounds(min_maf)
    words_per_sample = _count(words_per_sample, "words_per_sample")
    num_sites = _count(num_sites, "num_sites")
    x, beta, used, fit_mask = _fit_model(place, bits, words_per_sample, num_sites, scores, model,
                                         fit, "records")
    block = _block(block, place.bits(bits, words_per_sample))
    recs, count = _pcrelate_records_raw(place, bits, words_per_sample, num_sites,
                                        place.from_host(x), place.from_host(beta), lo, hi,
                                        min_kinship, block, max_records)
    return PCRelateRecords(recs, count, _min_kin(min_kinship), block, beta, used, fit_mask, x)


def pcrelate_records_raw_host(bits: np.ndarray, words_per_sample: int, num_sites: int, x, beta,
                              lo: float, hi: float, min_kin: float, block=None,
                              max_records=None):
    """cuking_pcrelate_records_host, the bare call: the pairs of ``block`` (as
    ``pcrelate_matrix_host`` takes it) with ``kin > min_kin`` as ``(records, count)``,
    ``KING_RESULT_DTYPE`` rows in ascending ``(sample_i, sample_j)`` with the kinship bytes of
    ``pcrelate_matrix_host``.  The buffer rule is ``ld_edges_host``'s: without ``max_records`` a
    default buffer, grown once to the exact count; with it, an overflow raises
    ``ResourceExhaustedError`` whose ``num_records`` is the exact count."""
    return _pcrelate_records_raw(HOST, bits, words_per_sample, num_sites, x, beta, lo, hi, min_kin,
                                 block, max_records)


def pcrelate_records_host(bits: np.ndarray, words_per_sample: int, num_sites: int, scores=None,
                          model=None, fit=None, min_maf: float = 0.01,
                          min_kinship: float = KING_CUTOFFS[0], block=None,
                          max_records=None) -> PCRelateRecords:
    """``KingContext.pcrelate_records`` on host memory and the host twins: no GPU."""
    return _pcrelate_records(HOST, bits, words_per_sample, num_sites, scores, model, fit, min_maf,
                             min_kinship, block, max_records)


def pcrelate_records_raw_device(ctx, bits, words_per_sample: int, num_sites: int, x, beta,
                                lo: float, hi: float, min_kin: float, block=None,
                                max_records=None, out=None, stream=None):
    return _pcrelate_records_raw(DevicePlace(ctx, stream), bits, words_per_sample, num_sites, x,
                                 beta, lo, hi, min_kin, block, max_records, out)


def pcrelate_records_device(ctx, bits, words_per_sample: int, num_sites: int, scores=None,
                            model=None, fit=None, min_maf: float = 0.01,
                            min_kinship: float = KING_CUTOFFS[0], block=None,
                            max_records=None) -> PCRelateRecords:
    return _pcrelate_records(DevicePlace(ctx), bits, words_per_sample, num_sites, scores, model,
                             fit, min_maf, min_kinship, block, max_records)
