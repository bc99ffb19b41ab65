"""IBD segments for listed pairs: the long runs of sites in which two samples never carry
opposite homozygotes (kind 1, IBD1) or never differ (kind 2, IBD2) -- KING ``--ibdseg``, IBIS and
TRUFFLE on unphased data.  include/cuking_amd.h "IBD segments for listed pairs" holds the
definition, csrc/king_ibd.h the word masks; this module wraps the call and derives the shared
proportions, a kinship and the relationship from the lengths.  No allele frequency, no principal
component and no ``min_maf`` enters, so the answer does not depend on a model of ancestry.

``bridge_sites`` (0, or at least 64) forgives isolated genotyping errors: two runs of at least
that many sites on either side of one break site of a group are linked, and a segment is a
chain of linked runs (the header's "IBD segments with bridged breaks").  0 is the strict call.

``ibd_scan`` needs no list: it scans every pair of a block and keeps the pairs with a kind-1
segment (the header's "IBD scan of a block"), as ``pcrelate_records`` does for PC-Relate.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import check
from .api import KING_CUTOFFS, _count, _counted_buffer, _out_capacity
from .pcrelate import (DUPLICATE, FULL_SIBLING, PARENT_CHILD, SECOND_DEGREE, THIRD_DEGREE,
                       UNRELATED, _block, _default_records, _device_pairs, _host_pairs)

MIN_SITES = _lib.IBD_MIN_SITES
# cuking_ibd_pair, cuking_ibd_segment
IBD_PAIR_DTYPE = np.dtype(
    [("sample_i", "<u4"), ("sample_j", "<u4"), ("segments1", "<u4"), ("segments2", "<u4"),
     ("length1", "<u8"), ("length2", "<u8"), ("longest1", "<u4"), ("longest2", "<u4")])
IBD_SEGMENT_DTYPE = np.dtype(
    [("pair", "<u4"), ("kind", "<u4"), ("first_site", "<u4"), ("last_site", "<u4")])
assert IBD_PAIR_DTYPE.itemsize == 40 and IBD_SEGMENT_DTYPE.itemsize == 16


def sort_segments(segments: np.ndarray) -> np.ndarray:
    """``IBD_SEGMENT_DTYPE`` rows by ``(pair, kind, first_site)`` (a copy)."""
    return np.sort(segments, order=["pair", "kind", "first_site"])


@dataclass
class IBDPairs:
    """What ``KingContext.ibd_segments`` / ``ibd_segments_host`` return, as host arrays:
    ``rows`` (``IBD_PAIR_DTYPE`` ``[P]``, the output rows in input order) and its fields
    ``sample_i``, ``sample_j`` (uint32, as given), ``segments1``, ``segments2`` (uint32: the
    number of segments of kind 1 / 2), ``length1``, ``length2`` (uint64: the sum of their
    lengths), ``longest1``, ``longest2`` (uint32); ``total_length`` (``genome_length`` of the
    call); ``segments`` (``IBD_SEGMENT_DTYPE`` rows in no particular order, or None when they
    were not asked for); ``min_sites``, ``min_length`` and ``bridge_sites`` of the call;
    ``bridged`` (uint32 ``[P, 2]`` when ``bridge_sites`` is not 0, else None): the bridged breaks
    inside the counted segments of kind 1 and of kind 2 -- the errors that were forgiven.
    From ``KingContext.ibd_scan`` / ``ibd_scan_host`` the rows are the records of the scan by
    ``(sample_i, sample_j)``, ``min_total`` its threshold (else None) and ``block`` its block;
    ``num_records`` is the number of rows either way."""
    rows: np.ndarray
    total_length: int
    segments: object
    min_sites: int
    min_length: int
    bridge_sites: int = 0
    bridged: object = None
    min_total: object = None
    block: object = None

    num_records = property(lambda self: int(self.rows.shape[0]))

    sample_i = property(lambda self: self.rows["sample_i"])
    sample_j = property(lambda self: self.rows["sample_j"])
    segments1 = property(lambda self: self.rows["segments1"])
    segments2 = property(lambda self: self.rows["segments2"])
    length1 = property(lambda self: self.rows["length1"])
    length2 = property(lambda self: self.rows["length2"])
    longest1 = property(lambda self: self.rows["longest1"])
    longest2 = property(lambda self: self.rows["longest2"])

    def pairs(self) -> np.ndarray:
        """``(sample_i, sample_j)`` of the rows as the uint32 ``[P, 2]`` array ``ibd_segments``
        and ``pcrelate_pairs`` take as their list."""
        return np.stack([self.sample_i, self.sample_j], axis=1).astype(np.uint32)

    def sorted(self) -> np.ndarray:
        """The segments by ``(pair, kind, first_site)`` (a copy); ValueError without a list."""
        if self.segments is None:
            raise ValueError("the call did not ask for the segment list (segments=True)")
        return sort_segments(self.segments)

    def proportions(self):
        """``(pi1, pi2, kin)`` in float64 on the host: ``pi1 = (length1 - length2) / total``
        (the share of the genome that is IBD1 only), ``pi2 = length2 / total`` and ``kin = pi1
        / 4 + pi2 / 2``.  A ``total_length`` of zero gives NaN."""
        total = np.float64(self.total_length)
        with np.errstate(invalid="ignore", divide="ignore"):
            pi2 = self.length2.astype(np.float64) / total
            pi1 = (self.length1 - self.length2).astype(np.float64) / total
        return pi1, pi2, pi1 / 4.0 + pi2 / 2.0

    def relationship(self, thresholds=KING_CUTOFFS, sibling_ibd2: float = 0.08) -> np.ndarray:
        """One code per pair (uint8; ``pcrelate.RELATIONSHIP_NAMES[code]``), the codes of
        ``PCRelatePairs.relationship``.  The degree is the number of the four ascending
        ``thresholds`` that ``kin`` of ``proportions()`` exceeds, in the strict float32
        comparison ``kin > t`` (a NaN exceeds none: unrelated); first degree is full siblings
        where ``pi2 > sibling_ibd2`` (strict; false for a NaN) and parent-child otherwise.  The
        0.08 is a convention -- a parent and a child share no IBD2, siblings a quarter of the
        genome --, an argument and not a measured value."""
        thr = np.asarray(thresholds, dtype=np.float32)
        if thr.shape != (4,) or not (np.diff(thr) > 0).all():
            raise ValueError(f"thresholds must be four ascending values, not {thresholds!r}")
        _, pi2, kin = self.proportions()
        with np.errstate(invalid="ignore"):
            degree = (kin.astype(np.float32)[:, None] > thr[None, :]).sum(axis=1)
            sibling = pi2 > float(sibling_ibd2)
        code = np.array([UNRELATED, THIRD_DEGREE, SECOND_DEGREE, PARENT_CHILD, DUPLICATE],
                        dtype=np.uint8)[degree]
        code[(degree == 3) & sibling] = FULL_SIBLING
        return code


def _site_array(values, name: str, num_sites: int, dtype):
    """None, or ``values`` as a contiguous ``dtype`` ``[num_sites]`` host array."""
    if values is None:
        return None
    values = np.asarray(values)
    if values.ndim != 1 or values.shape[0] != num_sites or values.dtype.kind not in "iu":
        raise ValueError(f"{name} must be an integer [{num_sites}] array, not {values.dtype} "
                         f"{values.shape}")
    info = np.iinfo(dtype)
    if values.size and (int(values.min()) < info.min or int(values.max()) > info.max):
        raise ValueError(f"{name} must fit {np.dtype(dtype).name}")
    return np.ascontiguousarray(values, dtype=dtype)


def genome_length(group, pos, num_sites: int) -> int:
    """The length a pair that shares everything would have: the sum over the groups of
    ``pos[last] - pos[first]`` (``pos`` None: the site index; ``group`` None: one group), on
    the host."""
    num_sites = _count(num_sites, "num_sites")
    if num_sites == 0:
        return 0
    group = _site_array(group, "group", num_sites, np.int32)
    pos = np.arange(num_sites, dtype=np.int64) if pos is None else \
        _site_array(pos, "pos", num_sites, np.uint32).astype(np.int64)
    first = np.ones(num_sites, dtype=bool)
    if group is not None:
        first[1:] = group[1:] != group[:-1]
    else:
        first[1:] = False
    last = np.roll(first, -1)
    return int(pos[last].sum() - pos[first].sum())


def _thresholds(min_sites, min_length):
    return _count(min_sites, "min_sites"), _count(min_length, "min_length")


def _bridge(bridge_sites) -> int:
    return _count(bridge_sites, "bridge_sites")


def _default_segments(count: int) -> int:
    """The buffer of a call without ``max_segments``: four segments per pair (the call is
    repeated once with the exact count if that overflows)."""
    return max(1, 4 * count)


def _segment_buffer(call, count: int, want: bool, max_segments, found):
    """The buffer rule (``_counted_buffer``) of a segment list, for every call that has one:
    ``_default_segments(count)`` by default, and a list that is not wanted (then
    ``max_segments`` is None) has capacity 0 and is not counted."""
    return _counted_buffer(call, _default_segments(count) if want else 0, max_segments,
                           "max_segments", found, "num_segments")


def ibd_segments_raw_host(bits: np.ndarray, words_per_sample: int, num_sites: int, pairs,
                          group=None, pos=None, min_sites: int = 512, min_length: int = 0,
                          segments: bool = False, max_segments=None, num_records=None,
                          bridge_sites: int = 0):
    """cuking_ibd_pairs_host, the bare call: ``(rows, segments)`` -- one ``IBD_PAIR_DTYPE`` row
    per pair of ``pairs`` (records with ``num_records``, or an integer ``[P, 2]`` array) and,
    with ``segments`` (or a ``max_segments``), the ``IBD_SEGMENT_DTYPE`` rows, else None.  Bit
    for bit what ``KingContext.ibd_segments_raw`` gives.  The buffer rule is ``ld_edges_host``'s:
    without ``max_segments`` a default buffer, grown once to the exact count; with it, an
    overflow raises ``ResourceExhaustedError`` whose ``num_segments`` is the exact count.
    With ``bridge_sites`` not 0 it is cuking_ibd_pairs_bridged_host and returns ``(rows,
    segments, bridged)``, ``bridged`` uint32 ``[P, 2]``."""
    assert bits.dtype == np.uint64 and bits.flags.c_contiguous
    words_per_sample = _count(words_per_sample, "words_per_sample")
    num_sites = _count(num_sites, "num_sites")
    min_sites, min_length = _thresholds(min_sites, min_length)
    bridge_sites = _bridge(bridge_sites)
    num_stored = bits.size // words_per_sample if words_per_sample else 0
    group = _site_array(group, "group", num_sites, np.int32)
    pos = _site_array(pos, "pos", num_sites, np.uint32)
    owner, ptr, count, stride = _host_pairs(pairs, num_records)   # (owner keeps ptr alive)
    out = np.zeros(count, dtype=IBD_PAIR_DTYPE)
    bridged = np.zeros((count, 2), dtype=np.uint32)
    pad = np.zeros(4, dtype=np.uint64)
    found = C.c_uint64(0)
    want = segments or max_segments is not None

    def call(capacity):
        segs = np.zeros(max(capacity, 1), dtype=IBD_SEGMENT_DTYPE)
        head = ((bits if bits.size else pad).ctypes.data, num_stored, words_per_sample, num_sites,
                None if group is None or not group.size else group.ctypes.data,
                None if pos is None or not pos.size else pos.ctypes.data, min_sites, min_length)
        pair = (ptr if count else None, count, stride, out.ctypes.data if count else None)
        tail = (segs.ctypes.data if want and capacity else None, capacity if want else 0,
                C.byref(found) if want else None)
        if bridge_sites == 0:
            status = _lib.load().cuking_ibd_pairs_host(*head, *pair, *tail)
        else:
            status = _lib.load().cuking_ibd_pairs_bridged_host(
                *head, bridge_sites, *pair, bridged.ctypes.data if count else None, *tail)
        return segs, status

    segs = _segment_buffer(call, count, want, max_segments, found)
    segs = segs[:found.value].copy() if want else None
    return (out, segs) if bridge_sites == 0 else (out, segs, bridged)


def ibd_segments_host(bits: np.ndarray, words_per_sample: int, num_sites: int, pairs,
                      group=None, pos=None, min_sites: int = 512, min_length: int = 0,
                      segments: bool = False, max_segments=None, num_records=None,
                      bridge_sites: int = 0) -> IBDPairs:
    """``KingContext.ibd_segments`` on host memory and the host twin: no GPU."""
    rows, segs, *bridged = ibd_segments_raw_host(bits, words_per_sample, num_sites, pairs, group,
                                                 pos, min_sites, min_length, segments,
                                                 max_segments, num_records, bridge_sites)
    return IBDPairs(rows, genome_length(group, pos, num_sites), segs, int(min_sites),
                    int(min_length), int(bridge_sites), *bridged)


def rows_to_host(rows) -> np.ndarray:
    """The ``[P, 10]`` int32 device tensor of ``ibd_segments_raw`` as ``IBD_PAIR_DTYPE`` rows on
    the host (waits for the copy)."""
    return np.ascontiguousarray(rows.cpu().numpy()).view(IBD_PAIR_DTYPE).reshape(-1)


def segments_to_host(segments, num_segments: int) -> np.ndarray:
    """The first ``num_segments`` rows of the ``[*, 4]`` int32 device tensor of
    ``ibd_segments_raw`` as ``IBD_SEGMENT_DTYPE`` rows on the host (waits for the copy)."""
    return np.ascontiguousarray(segments[:num_segments].cpu().numpy()) \
        .view(IBD_SEGMENT_DTYPE).reshape(-1)


def bridged_to_host(bridged) -> np.ndarray:
    """The ``[P, 2]`` int32 device tensor of ``ibd_segments_raw`` as uint32 on the host (waits for
    the copy)."""
    return np.ascontiguousarray(bridged.cpu().numpy()).view(np.uint32)


def _device_sites(ctx, values, name: str, num_sites: int, dtype):
    """None, or ``values`` (a host array, or an int32 device tensor of ``num_sites``) on the
    device; uint32 travels as its int32 bit pattern."""
    import torch
    from .api import _device_tensor
    if values is None:
        return None
    if isinstance(values, torch.Tensor):
        return _device_tensor(ctx.device, values, name, torch.int32, shape=(num_sites,))
    host = _site_array(values, name, num_sites, dtype)
    return torch.from_numpy(host.view(np.int32)).to(f"cuda:{ctx.device}")


def ibd_segments_raw_device(ctx, bits, words_per_sample: int, num_sites: int, pairs, group=None,
                            pos=None, min_sites: int = 512, min_length: int = 0,
                            segments: bool = False, max_segments=None, num_records=None,
                            out=None, stream=None, bridge_sites: int = 0):
    import torch
    from .api import _device_tensor, _stream_handle
    words_per_sample = _count(words_per_sample, "words_per_sample")
    num_sites = _count(num_sites, "num_sites")
    min_sites, min_length = _thresholds(min_sites, min_length)
    bridge_sites = _bridge(bridge_sites)
    num_stored = ctx._rows_of(bits, words_per_sample)
    dev = f"cuda:{ctx.device}"
    d_group = _device_sites(ctx, group, "group", num_sites, np.int32)
    d_pos = _device_sites(ctx, pos, "pos", num_sites, np.uint32)
    owner, count, stride = _device_pairs(ctx, pairs, num_records)
    if out is None:
        out = torch.empty((count, 10), dtype=torch.int32, device=dev)
    else:
        _device_tensor(ctx.device, out, "out", torch.int32, shape=(count, 10))
    bridged = None
    if bridge_sites != 0:   # (uint32 travels as its int32 bit pattern)
        bridged = torch.empty((count, 2), dtype=torch.int32, device=dev)
    want = segments or max_segments is not None
    found = C.c_uint64(0)
    # (uploads ran on the current stream: `stream` waits for them)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())

    def call(capacity):
        segs = torch.empty((max(capacity, 1), 4), dtype=torch.int32, device=dev)
        head = (ctx.handle, bits.data_ptr(), num_stored, words_per_sample, num_sites,
                None if d_group is None or not num_sites else d_group.data_ptr(),
                None if d_pos is None or not num_sites else d_pos.data_ptr(), min_sites,
                min_length)
        pair = (owner.data_ptr() if count else None, count, stride,
                out.data_ptr() if count else None)
        tail = (segs.data_ptr() if want and capacity else None, capacity if want else 0,
                C.byref(found) if want else None, _stream_handle(stream))
        if bridge_sites == 0:
            return segs, ctx.lib.cuking_ibd_pairs(*head, *pair, *tail)
        return segs, ctx.lib.cuking_ibd_pairs_bridged(
            *head, bridge_sites, *pair, bridged.data_ptr() if count else None, *tail)

    segs = _segment_buffer(call, count, want, max_segments, found)
    if stream is not None:  # (converted copies are freed on return)
        for t in (owner, d_group, d_pos, segs):
            if t is not None:
                t.record_stream(stream)
    got = (out, (segs if want else None), int(found.value))
    return got if bridge_sites == 0 else got + (bridged,)


def ibd_segments_device(ctx, bits, words_per_sample: int, num_sites: int, pairs, group=None,
                        pos=None, min_sites: int = 512, min_length: int = 0,
                        segments: bool = False, max_segments=None, num_records=None,
                        stream=None, bridge_sites: int = 0) -> IBDPairs:
    import torch
    host_group = group.cpu().numpy() if isinstance(group, torch.Tensor) else group
    host_pos = pos.cpu().numpy().view(np.uint32) if isinstance(pos, torch.Tensor) else pos
    total = genome_length(host_group, host_pos, num_sites)
    rows, segs, found, *bridged = ibd_segments_raw_device(
        ctx, bits, words_per_sample, num_sites, pairs, group, pos, min_sites, min_length, segments,
        max_segments, num_records, stream=stream, bridge_sites=bridge_sites)
    if stream is not None:
        stream.synchronize()
    return IBDPairs(rows_to_host(rows), total,
                    None if segs is None else segments_to_host(segs, found), int(min_sites),
                    int(min_length), int(bridge_sites), *map(bridged_to_host, bridged))


# ---- the scan of a block: every pair, no list --------------------------------------------------

def sort_records(rows: np.ndarray) -> np.ndarray:
    """``IBD_PAIR_DTYPE`` rows by ``(sample_i, sample_j)`` (a copy)."""
    return np.sort(rows, order=["sample_i", "sample_j"])


def _min_total(min_total) -> int:
    min_total = int(min_total)
    if not 0 <= min_total < 1 << 64:
        raise ValueError(f"min_total must be in [0, 2^64), not {min_total}")
    return min_total


def _record_buffer(call, block, max_records, found):
    """The buffer rule (``_counted_buffer``) of the scan's records, with the default of
    ``pcrelate_records``: 16 records per sample of the block."""
    return _counted_buffer(call, _default_records(block), max_records, "max_records", found,
                           "num_records")


def ibd_scan_raw_host(bits: np.ndarray, words_per_sample: int, num_sites: int, group=None,
                      pos=None, min_sites: int = 512, min_length: int = 0, min_total: int = 0,
                      block=None, max_records=None):
    """cuking_ibd_scan_host, the bare call: ``(records, count)`` -- the pairs of ``block`` (a
    ``Submatrix`` or ``(i_begin, i_end, j_begin, j_end)`` over the stored samples; None = all)
    with a kind-1 segment and ``length1 >= min_total`` as ``IBD_PAIR_DTYPE`` rows in ascending
    ``(sample_i, sample_j)``, each the bytes ``ibd_segments_raw_host`` gives for that pair.  The
    buffer rule is ``pcrelate_records_raw_host``'s."""
    assert bits.dtype == np.uint64 and bits.flags.c_contiguous
    words_per_sample = _count(words_per_sample, "words_per_sample")
    num_sites = _count(num_sites, "num_sites")
    min_sites, min_length = _thresholds(min_sites, min_length)
    min_total = _min_total(min_total)
    num_stored = bits.size // words_per_sample if words_per_sample else 0
    group = _site_array(group, "group", num_sites, np.int32)
    pos = _site_array(pos, "pos", num_sites, np.uint32)
    block = _block(block, num_stored)
    pad = np.zeros(4, dtype=np.uint64)
    found = C.c_uint64(0)

    def call(capacity):
        recs = np.zeros(max(capacity, 1), dtype=IBD_PAIR_DTYPE)
        status = _lib.load().cuking_ibd_scan_host(
            (bits if bits.size else pad).ctypes.data, num_stored, words_per_sample, num_sites,
            None if group is None or not group.size else group.ctypes.data,
            None if pos is None or not pos.size else pos.ctypes.data, min_sites, min_length,
            C.byref(block.c), min_total, recs.ctypes.data if capacity else None, capacity,
            C.byref(found))
        return recs, status

    recs = _record_buffer(call, block, max_records, found)
    return recs[:found.value].copy(), int(found.value)


def ibd_scan_host(bits: np.ndarray, words_per_sample: int, num_sites: int, group=None, pos=None,
                  min_sites: int = 512, min_length: int = 0, min_total: int = 0, block=None,
                  max_records=None) -> IBDPairs:
    """``KingContext.ibd_scan`` on host memory and the host twin: no GPU."""
    recs, _ = ibd_scan_raw_host(bits, words_per_sample, num_sites, group, pos, min_sites,
                                min_length, min_total, block, max_records)
    num_stored = bits.size // words_per_sample if words_per_sample else 0
    return IBDPairs(recs, genome_length(group, pos, num_sites), None, int(min_sites),
                    int(min_length), min_total=int(min_total), block=_block(block, num_stored))


def records_to_host(records, num_records: int) -> np.ndarray:
    """The first ``num_records`` rows of the ``[*, 10]`` int32 device tensor of ``ibd_scan_raw``
    as ``IBD_PAIR_DTYPE`` rows on the host by ``(sample_i, sample_j)`` (waits for the copy)."""
    return sort_records(rows_to_host(records[:num_records]))


def ibd_scan_raw_device(ctx, bits, words_per_sample: int, num_sites: int, group=None, pos=None,
                        min_sites: int = 512, min_length: int = 0, min_total: int = 0,
                        block=None, max_records=None, out=None, stream=None):
    import torch
    from .api import _device_tensor, _stream_handle
    words_per_sample = _count(words_per_sample, "words_per_sample")
    num_sites = _count(num_sites, "num_sites")
    min_sites, min_length = _thresholds(min_sites, min_length)
    min_total = _min_total(min_total)
    num_stored = ctx._rows_of(bits, words_per_sample)
    dev = f"cuda:{ctx.device}"
    d_group = _device_sites(ctx, group, "group", num_sites, np.int32)
    d_pos = _device_sites(ctx, pos, "pos", num_sites, np.uint32)
    block = _block(block, num_stored)
    if out is not None:
        _device_tensor(ctx.device, out, "out", torch.int32, cols=10)
        max_records = _out_capacity(out, max_records)
    found = C.c_uint64(0)
    # (uploads ran on the current stream: `stream` waits for them)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())

    def call(capacity):
        recs = out if out is not None else \
            torch.empty((max(capacity, 1), 10), dtype=torch.int32, device=dev)
        status = ctx.lib.cuking_ibd_scan(
            ctx.handle, bits.data_ptr(), num_stored, words_per_sample, num_sites,
            None if d_group is None or not num_sites else d_group.data_ptr(),
            None if d_pos is None or not num_sites else d_pos.data_ptr(), min_sites, min_length,
            C.byref(block.c), min_total, recs.data_ptr() if capacity else None, capacity,
            C.byref(found), _stream_handle(stream))
        return recs, status

    recs = _record_buffer(call, block, max_records, found)
    if stream is not None:  # (converted copies are freed on return)
        for t in (d_group, d_pos, recs):
            if t is not None:
                t.record_stream(stream)
    return recs, int(found.value)


def ibd_scan_device(ctx, bits, words_per_sample: int, num_sites: int, group=None, pos=None,
                    min_sites: int = 512, min_length: int = 0, min_total: int = 0, block=None,
                    max_records=None, stream=None) -> IBDPairs:
    import torch
    host_group = group.cpu().numpy() if isinstance(group, torch.Tensor) else group
    host_pos = pos.cpu().numpy().view(np.uint32) if isinstance(pos, torch.Tensor) else pos
    total = genome_length(host_group, host_pos, num_sites)
    recs, count = ibd_scan_raw_device(ctx, bits, words_per_sample, num_sites, group, pos,
                                      min_sites, min_length, min_total, block, max_records,
                                      stream=stream)
    return IBDPairs(records_to_host(recs, count), total, None, int(min_sites), int(min_length),
                    min_total=int(min_total),
                    block=_block(block, ctx._rows_of(bits, words_per_sample)))
