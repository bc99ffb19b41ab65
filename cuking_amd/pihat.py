"""PI_HAT: the method-of-moments IBD estimate of PLINK ``--genome`` and
``hl.identity_by_descent`` (include/cuking_amd.h "PI_HAT (PLINK --genome)" holds the definition,
csrc/king_pihat.h the code host, device and tests share).

Model (``pi_hat_model_host``): the five expected IBS-state proportions from the genotype counts of
the rows the allele frequencies come from -- founders, an unrelated set, or the cohort itself.
Pair (``pi_hat_of_records``): ``z0, z1, z2, pi_hat`` from a record's ``ibs0, ibs1, ibs2``, for
ANY record buffer, ``KingContext.run``'s included.  Scan (``KingContext.pi_hat_records`` /
``pi_hat_records_host``): every pair of a block with ``(float32)pi_hat > min_pi_hat`` as the
24-byte records ``unrelated_set``, ``pcrelate_pairs`` and ``ibd_segments`` take, ``kin`` holding
the float32 PI_HAT.  One body over a place (``_place``) serves host twin and device call.

PI_HAT assumes ONE homogeneous population: it reads shared ancestry as relatedness (within a
population of an admixed cohort it is inflated; that is what PC-Relate is for).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import CPihatModel, check
from ._place import HOST, DevicePlace, tensor_to_host
from .api import (KING_CUTOFFS, KING_RESULT_DTYPE, ResourceExhaustedError, Submatrix, _count,
                  _counted_buffer, _stream_handle, sort_results)

PIHAT_MAX_PEOPLE = 1 << 24
DEFAULT_MIN_PI_HAT = 2 * KING_CUTOFFS[0]   # the third-degree cut-off doubled: a convention


@dataclass(frozen=True)
class PiHatModel:
    """cuking_pihat_model: the expected proportions ``e00, e01, e02, e11, e12`` (E_uv: IBS state
    v given IBD state u) and the sites they average over."""
    e00: float
    e01: float
    e02: float
    e11: float
    e12: float
    sites_used: int

    @property
    def c(self) -> CPihatModel:
        return CPihatModel(self.e00, self.e01, self.e02, self.e11, self.e12, self.sites_used)

    def as_tuple(self) -> tuple:
        return (self.e00, self.e01, self.e02, self.e11, self.e12, self.sites_used)


def pi_hat_model_host(counts, num_sites: int) -> PiHatModel:
    """cuking_pihat_model_host: the model from the first ``num_sites`` rows of a ``site_counts``
    array (uint32 / int32 ``[>= num_sites, 4]``: hom_ref, het, hom_var, missing -- ignored).  A
    site counts iff it has two people or more; without one the model holds NaNs and no pair
    qualifies.  A row of more than 2^24 people is refused."""
    num_sites = _count(num_sites, "num_sites")
    counts = np.asarray(counts)
    if counts.ndim != 2 or counts.shape[1] != 4 or counts.dtype not in (np.uint32, np.int32) or \
            counts.shape[0] < num_sites:
        raise ValueError(f"counts must be a uint32 [>= {num_sites}, 4] array (site_counts), not "
                         f"{counts.dtype} {counts.shape}")
    counts = np.ascontiguousarray(counts).view(np.uint32)
    m = CPihatModel()
    check(_lib.load().cuking_pihat_model_host(counts.ctypes.data if num_sites else None,
                                              num_sites, C.byref(m)))
    return PiHatModel(m.e00, m.e01, m.e02, m.e11, m.e12, int(m.sites_used))


def _flags(bounded: bool) -> int:
    return 0 if bounded else _lib.PIHAT_UNBOUNDED


def _host_records(records, num_records=None) -> np.ndarray:
    """A record buffer (host ``KING_RESULT_DTYPE`` rows or the int32 ``[*, 6]`` device tensor) as
    contiguous host rows, the first ``num_records``."""
    if not isinstance(records, np.ndarray):
        records = tensor_to_host(records if num_records is None else records[:num_records],
                                 KING_RESULT_DTYPE)
    if records.dtype != KING_RESULT_DTYPE or records.ndim != 1:
        raise ValueError("records must be KING_RESULT_DTYPE rows or an int32 [*, 6] device tensor")
    if num_records is not None:
        if _count(num_records, "num_records") > records.shape[0]:
            raise ValueError(f"records holds {records.shape[0]} rows, num_records is "
                             f"{num_records}")
        records = records[:num_records]
    return np.ascontiguousarray(records)


def pi_hat_of_records(records, model: PiHatModel, bounded: bool = True,
                      num_records=None) -> np.ndarray:
    """cuking_pihat_records_host: float64 ``[n, 4]`` = ``z0, z1, z2, pi_hat`` of every record's
    ``ibs0, ibs1, ibs2`` under ``model`` -- what PLINK ``--genome`` prints for those pairs.  Any
    record buffer: ``KingContext.run``'s, ``pi_hat_records``', host rows or the device tensor
    (copied to the host)."""
    rows = _host_records(records, num_records)
    out = np.empty((rows.shape[0], 4), dtype=np.float64)
    check(_lib.load().cuking_pihat_records_host(
        rows.ctypes.data if rows.size else None, rows.shape[0], C.byref(model.c),
        _flags(bounded), out.ctypes.data if rows.size else None))
    return out


@dataclass
class PiHatRecords:
    """What ``KingContext.pi_hat_records`` / ``pi_hat_records_host`` return: ``records`` (the
    first ``num_records`` rows are the pairs with ``(float32)pi_hat > min_pi_hat``, ``sample_i <
    sample_j``, ``kin`` = the float32 PI_HAT, ``ibs0/1/2`` those of a KING record: the int32
    ``[*, 6]`` device tensor in no particular order, or ``KING_RESULT_DTYPE`` rows in ascending
    order from the host twin), ``num_records``, the ``model``, ``min_pi_hat``, ``bounded`` and
    the ``block``."""
    records: object
    num_records: int
    model: PiHatModel
    min_pi_hat: float
    bounded: bool
    block: Submatrix

    def sorted(self) -> np.ndarray:
        """The records as ``KING_RESULT_DTYPE`` rows on the host by ``(sample_i, sample_j)`` (a
        copy; waits for it)."""
        return sort_results(_host_records(self.records, self.num_records).copy())

    def z(self) -> np.ndarray:
        """float64 ``[num_records, 4]``: ``z0, z1, z2, pi_hat`` of ``sorted()``'s rows."""
        return pi_hat_of_records(self.sorted(), self.model, self.bounded)

    def pairs(self) -> np.ndarray:
        """uint32 ``[num_records, 2]`` of ``sorted()``'s rows: the list ``pcrelate_pairs`` and
        ``ibd_segments`` take."""
        rows = self.sorted()
        return np.stack([rows["sample_i"], rows["sample_j"]], axis=1).astype(np.uint32)


def site_counts_of_host_bits(bits: np.ndarray, words_per_sample: int) -> np.ndarray:
    """``KingContext.site_counts`` of a host bitset ``[rows, words_per_sample]`` (a row is its
    het words, then its hom_var words; both bits = missing): uint32 ``[64 P, 4]``."""
    rows = np.ascontiguousarray(bits, dtype=np.uint64).reshape(-1, words_per_sample)
    planes = words_per_sample // 2
    flat = np.unpackbits(rows.view(np.uint8), axis=1, bitorder="little").astype(bool)
    het, hom = flat[:, :64 * planes], flat[:, 64 * planes:]
    out = np.empty((64 * planes, 4), dtype=np.uint32)
    out[:, 0] = (~het & ~hom).sum(axis=0)
    out[:, 1] = (het & ~hom).sum(axis=0)
    out[:, 2] = (~het & hom).sum(axis=0)
    out[:, 3] = (het & hom).sum(axis=0)
    return out


def _default_records(sm: Submatrix) -> int:
    """The buffer rule of ``pcrelate_records``: 16 records per sample of the block, at most its
    pairs."""
    return max(1, min(sm.NumPairs(), 16 * (sm.NumRows() + sm.NumCols())))


def _scan(place, sm, words_per_sample, bits, model, min_pi_hat, flags, capacity, tile_range):
    """One library call into a fresh buffer of ``capacity`` records: ``(buffer, status, count)``.
    The host twin counts into a word of the caller's; the device call counts into device words
    (the counter and overflow flag of ``compute_king``), read back after a wait."""
    recs = place.zeros(max(capacity, 1), KING_RESULT_DTYPE)
    if not isinstance(place, DevicePlace):
        if tile_range is not None:
            raise ValueError("tile_range goes with the device call")
        count = C.c_uint32(0)
        status = place.fn("compute_pihat")(C.byref(sm.c), words_per_sample,
                                           place.ptr(bits, pad=True), C.byref(model.c),
                                           min_pi_hat, flags, capacity,
                                           place.ptr(recs) if capacity else None, C.byref(count))
        return recs, status, int(count.value)
    ctx = place.ctx
    words = place.zeros(2, np.uint32)
    # (the zero-fills above and whatever made `bits` ran on the current stream: the call's
    #  stream waits for them)
    place.uploads_done()
    head = (ctx.handle, C.byref(sm.c), words_per_sample, bits.data_ptr())
    tail = (C.byref(model.c), min_pi_hat, flags, capacity, recs.data_ptr() if capacity else None,
            words[0:1].data_ptr(), words[1:2].data_ptr(), _stream_handle(place.stream))
    if tile_range is None:
        status = ctx.lib.cuking_compute_pihat(*head, *tail)
    else:
        status = ctx.lib.cuking_compute_pihat_tiles(*head, int(tile_range[0]), int(tile_range[1]),
                                                    *tail)
    if status != _lib.OK:
        return recs, status, 0
    place.keep(recs, words)
    place.finish()
    import torch
    if place.stream is None:
        torch.cuda.current_stream(ctx.device).synchronize()
    count, overflow = (int(x) & 0xFFFFFFFF for x in words.tolist())
    if overflow or count > capacity:
        return recs, _lib.ERR_RESOURCE_EXHAUSTED, count
    return recs, _lib.OK, count


def _pi_hat_records(place, sm, words_per_sample, bits, num_sites, min_pi_hat, counts, model,
                    bounded, max_results, tile_range=None) -> PiHatRecords:
    words_per_sample = _count(words_per_sample, "words_per_sample")
    num_sites = _count(num_sites, "num_sites")
    if num_sites > 32 * words_per_sample:
        raise ValueError(f"{num_sites} sites do not fit {words_per_sample} words per sample")
    stored = place.bits(bits, words_per_sample)
    if stored < sm.NumSamples():
        raise ValueError(f"bits holds {stored} samples, the block stores {sm.NumSamples()}")
    if model is not None and counts is not None:
        raise ValueError("pass counts or model, not both")
    if model is None:
        if counts is None:
            # the call's own stored samples
            if isinstance(place, DevicePlace):
                # (site_counts accumulates: zeroed on the current stream, which the call's
                #  stream then waits for)
                out = place.zeros((words_per_sample // 2 * 64, 4), np.uint32)
                place.uploads_done()
                counts = place.ctx.site_counts(bits[:sm.NumSamples() * words_per_sample]
                                               if bits.dim() == 1 else bits[:sm.NumSamples()],
                                               words_per_sample, out=out, stream=place.stream)
                place.keep(out)
            else:
                counts = site_counts_of_host_bits(
                    bits.reshape(-1)[:sm.NumSamples() * words_per_sample], words_per_sample)
        if not isinstance(counts, np.ndarray):
            place.finish()
            counts = tensor_to_host(counts, np.uint32)
        model = pi_hat_model_host(counts, num_sites)
    elif not isinstance(model, PiHatModel):
        raise ValueError("model must be a PiHatModel (pi_hat_model_host, or an earlier call's)")
    min_pi_hat = float(np.float32(min_pi_hat))
    found = C.c_uint64(0)

    def call(capacity):
        recs, status, count = _scan(place, sm, words_per_sample, bits, model, min_pi_hat,
                                    _flags(bounded), capacity, tile_range)
        found.value = count
        return recs, status

    try:
        recs = _counted_buffer(call, _default_records(sm), max_results, "max_results", found,
                               "num_records")
    except ResourceExhaustedError as e:
        if not e.args or not e.args[0] or "pi_hat" not in e.args[0]:
            e.args = (f"pi_hat: {found.value} records do not fit max_results: retry with that "
                      "many",)
        raise
    count = int(found.value)
    return PiHatRecords(place.trim(recs, count), count, model, min_pi_hat, bool(bounded), sm)


def pi_hat_records_host(sm: Submatrix, words_per_sample: int, bits: np.ndarray, num_sites: int,
                        min_pi_hat: float = DEFAULT_MIN_PI_HAT, counts=None, model=None,
                        bounded: bool = True, max_results=None) -> PiHatRecords:
    """``KingContext.pi_hat_records`` on host memory and the host twin (plain popcounts per
    pair, records in ascending ``(i, j)``): no GPU."""
    bits = np.ascontiguousarray(bits)
    if bits.dtype != np.uint64:
        raise ValueError(f"bits must be uint64, not {bits.dtype}")
    return _pi_hat_records(HOST, sm, words_per_sample, bits, num_sites, min_pi_hat, counts, model,
                           bounded, max_results)


def pi_hat_records_device(ctx, sm: Submatrix, words_per_sample: int, bits, num_sites: int,
                          min_pi_hat: float = DEFAULT_MIN_PI_HAT, counts=None, model=None,
                          bounded: bool = True, max_results=None, stream=None,
                          tile_range=None) -> PiHatRecords:
    return _pi_hat_records(DevicePlace(ctx, stream), sm, words_per_sample, bits, num_sites,
                           min_pi_hat, counts, model, bounded, max_results, tile_range)
