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
from ._place import HOST, DevicePlace, site_array, tensor_to_host
from .api import KING_CUTOFFS, _count, _counted_buffer, _out_capacity
from .pcrelate import (DUPLICATE, FULL_SIBLING, PARENT_CHILD, SECOND_DEGREE, THIRD_DEGREE,
                       UNRELATED, _block, _default_records)

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


def genome_length(group, pos, num_sites: int) -> int:
    """The length a pair that shares everything would have: the sum over the groups of
    ``pos[last] - pos[first]`` (``pos`` None: the site index; ``group`` None: one group), on
    the host."""
    num_sites = _count(num_sites, "num_sites")
    if num_sites == 0:
        return 0
    group = site_array(group, "group", num_sites, np.int32)
    pos = np.arange(num_sites, dtype=np.int64) if pos is None else \
        site_array(pos, "pos", num_sites, np.uint32).astype(np.int64)
    first = np.ones(num_sites, dtype=bool)
    if group is not None:
        first[1:] = group[1:] != group[:-1]
    else:
        first[1:] = False
    last = np.roll(first, -1)
    return int(pos[last].sum() - pos[first].sum())


def _place_genome_length(place, group, pos, num_sites: int) -> int:
    return genome_length(place.host_sites(group, np.int32), place.host_sites(pos, np.uint32),
                         num_sites)


def _scan_head(place, bits, words_per_sample, num_sites, group, pos, min_sites, min_length):
    """What the argument list of every run walk (IBD pairs, IBD scan, ROH) begins with, as
    ``(head, num_stored, owners)``; ``owners`` keeps the site arrays behind ``head`` alive."""
    words_per_sample = _count(words_per_sample, "words_per_sample")
    num_sites = _count(num_sites, "num_sites")
    min_sites, min_length = _count(min_sites, "min_sites"), _count(min_length, "min_length")
    num_stored = place.bits(bits, words_per_sample)
    group = place.sites(group, "group", num_sites, np.int32)
    pos = place.sites(pos, "pos", num_sites, np.uint32)
    return (place.ptr(bits, pad=True), num_stored, words_per_sample, num_sites, place.ptr(group),
            place.ptr(pos), min_sites, min_length), num_stored, (group, pos)


def _default_segments(count: int) -> int:
    """The buffer of a call without ``max_segments``: four segments per pair (the call is
    repeated once with the exact count if that overflows)."""
    return max(1, 4 * count)


def _segment_list(place, call, count: int, want: bool, max_segments):
    """The segment list of a call that has one, as ``(segments or None, num_segments)``:
    ``call(pointer, capacity, counter)`` is the library call with the list's three arguments.
    The buffer rule is ``_counted_buffer``'s with ``_default_segments(count)`` by default; a
    list that is not wanted (then ``max_segments`` is None) has no buffer, capacity 0 and no
    counter."""
    found = C.c_uint64(0)

    def sized(capacity):
        segs = place.alloc(max(capacity, 1), IBD_SEGMENT_DTYPE)
        return segs, call(place.ptr(segs) if want and capacity else None,
                          capacity if want else 0, C.byref(found) if want else None)

    segs = _counted_buffer(sized, _default_segments(count) if want else 0, max_segments,
                           "max_segments", found, "num_segments")
    place.keep(segs)
    return (place.trim(segs, found.value) if want else None), int(found.value)


def _ibd_segments_raw(place, bits, words_per_sample, num_sites, pairs, group, pos, min_sites,
                      min_length, segments, max_segments, num_records, bridge_sites, out=None):
    head, _, owners = _scan_head(place, bits, words_per_sample, num_sites, group, pos, min_sites,
                                 min_length)
    bridge_sites = _count(bridge_sites, "bridge_sites")
    owner, count, stride = place.pairs(pairs, num_records)
    out = place.alloc(count, IBD_PAIR_DTYPE) if out is None else \
        place.out(out, "out", IBD_PAIR_DTYPE, count)
    pair = (place.ptr(owner) if count else None, count, stride, place.ptr(out))
    # (uint32 travels as its int32 bit pattern)
    bridged = place.alloc((count, 2), np.uint32) if bridge_sites else None
    place.uploads_done()

    def call(*tail):
        if bridge_sites == 0:
            return place.fn("ibd_pairs")(*head, *pair, *tail)
        return place.fn("ibd_pairs_bridged")(*head, bridge_sites, *pair, place.ptr(bridged),
                                             *tail)

    got = (out, *_segment_list(place, call, count, segments or max_segments is not None,
                               max_segments))
    return got if bridge_sites == 0 else got + (bridged,)


def _ibd_segments(place, bits, words_per_sample, num_sites, pairs, group, pos, min_sites,
                  min_length, segments, max_segments, num_records, bridge_sites) -> IBDPairs:
    total = _place_genome_length(place, group, pos, num_sites)
    rows, segs, found, *bridged = _ibd_segments_raw(
        place, bits, words_per_sample, num_sites, pairs, group, pos, min_sites, min_length,
        segments, max_segments, num_records, bridge_sites)
    place.finish()
    return IBDPairs(place.to_host(rows, IBD_PAIR_DTYPE), total,
                    None if segs is None else place.to_host(segs, IBD_SEGMENT_DTYPE, found),
                    int(min_sites), int(min_length), int(bridge_sites),
                    *(place.to_host(b, np.uint32) for b in bridged))


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
    rows, segs, _, *bridged = _ibd_segments_raw(
        HOST, bits, words_per_sample, num_sites, pairs, group, pos, min_sites, min_length,
        segments, max_segments, num_records, bridge_sites)
    return (rows, segs, *bridged)


def ibd_segments_host(bits: np.ndarray, words_per_sample: int, num_sites: int, pairs,
                      group=None, pos=None, min_sites: int = 512, min_length: int = 0,
                      segments: bool = False, max_segments=None, num_records=None,
                      bridge_sites: int = 0) -> IBDPairs:
    """``KingContext.ibd_segments`` on host memory and the host twin: no GPU."""
    return _ibd_segments(HOST, bits, words_per_sample, num_sites, pairs, group, pos, min_sites,
                         min_length, segments, max_segments, num_records, bridge_sites)


def rows_to_host(rows) -> np.ndarray:
    """The ``[P, 10]`` int32 device tensor of ``ibd_segments_raw`` as ``IBD_PAIR_DTYPE`` rows on
    the host (waits for the copy)."""
    return tensor_to_host(rows, IBD_PAIR_DTYPE)


def segments_to_host(segments, num_segments: int) -> np.ndarray:
    """The first ``num_segments`` rows of the ``[*, 4]`` int32 device tensor of
    ``ibd_segments_raw`` as ``IBD_SEGMENT_DTYPE`` rows on the host (waits for the copy)."""
    return tensor_to_host(segments[:num_segments], IBD_SEGMENT_DTYPE)


def bridged_to_host(bridged) -> np.ndarray:
    """The ``[P, 2]`` int32 device tensor of ``ibd_segments_raw`` as uint32 on the host (waits for
    the copy)."""
    return tensor_to_host(bridged, np.uint32)


def ibd_segments_raw_device(ctx, bits, words_per_sample: int, num_sites: int, pairs, group=None,
                            pos=None, min_sites: int = 512, min_length: int = 0,
                            segments: bool = False, max_segments=None, num_records=None,
                            out=None, stream=None, bridge_sites: int = 0):
    return _ibd_segments_raw(DevicePlace(ctx, stream), bits, words_per_sample, num_sites, pairs,
                             group, pos, min_sites, min_length, segments, max_segments,
                             num_records, bridge_sites, out)


def ibd_segments_device(ctx, bits, words_per_sample: int, num_sites: int, pairs, group=None,
                        pos=None, min_sites: int = 512, min_length: int = 0,
                        segments: bool = False, max_segments=None, num_records=None,
                        stream=None, bridge_sites: int = 0) -> IBDPairs:
    return _ibd_segments(DevicePlace(ctx, stream), bits, words_per_sample, num_sites, pairs,
                         group, pos, min_sites, min_length, segments, max_segments, num_records,
                         bridge_sites)


# ---- the scan of a block: every pair, no list --------------------------------------------------

def sort_records(rows: np.ndarray) -> np.ndarray:
    """``IBD_PAIR_DTYPE`` rows by ``(sample_i, sample_j)`` (a copy)."""
    return np.sort(rows, order=["sample_i", "sample_j"])


def _ibd_scan_raw(place, bits, words_per_sample, num_sites, group, pos, min_sites, min_length,
                  min_total, block, max_records, out=None):
    head, num_stored, owners = _scan_head(place, bits, words_per_sample, num_sites, group, pos,
                                          min_sites, min_length)
    min_total = int(min_total)
    if not 0 <= min_total < 1 << 64:
        raise ValueError(f"min_total must be in [0, 2^64), not {min_total}")
    block = _block(block, num_stored)
    if out is not None:
        place.out(out, "out", IBD_PAIR_DTYPE)
        max_records = _out_capacity(out, max_records)
    found = C.c_uint64(0)
    place.uploads_done()

    def call(capacity):
        recs = out if out is not None else place.alloc(max(capacity, 1), IBD_PAIR_DTYPE)
        return recs, place.fn("ibd_scan")(*head, C.byref(block.c), min_total,
                                          place.ptr(recs) if capacity else None, capacity,
                                          C.byref(found))

    # (the buffer rule and the default of ``pcrelate_records``: 16 records per sample of the block)
    recs = _counted_buffer(call, _default_records(block), max_records, "max_records", found,
                           "num_records")
    place.keep(recs)
    return place.trim(recs, found.value), int(found.value), block


def _ibd_scan(place, bits, words_per_sample, num_sites, group, pos, min_sites, min_length,
              min_total, block, max_records) -> IBDPairs:
    total = _place_genome_length(place, group, pos, num_sites)
    recs, count, block = _ibd_scan_raw(place, bits, words_per_sample, num_sites, group, pos,
                                       min_sites, min_length, min_total, block, max_records)
    return IBDPairs(sort_records(place.to_host(recs, IBD_PAIR_DTYPE, count)), total, None,
                    int(min_sites), int(min_length), min_total=int(min_total), block=block)


def ibd_scan_raw_host(bits: np.ndarray, words_per_sample: int, num_sites: int, group=None,
                      pos=None, min_sites: int = 512, min_length: int = 0, min_total: int = 0,
                      block=None, max_records=None):
    """cuking_ibd_scan_host, the bare call: ``(records, count)`` -- the pairs of ``block`` (a
    ``Submatrix`` or ``(i_begin, i_end, j_begin, j_end)`` over the stored samples; None = all)
    with a kind-1 segment and ``length1 >= min_total`` as ``IBD_PAIR_DTYPE`` rows in ascending
    ``(sample_i, sample_j)``, each the bytes ``ibd_segments_raw_host`` gives for that pair.  The
    buffer rule is ``pcrelate_records_raw_host``'s."""
    return _ibd_scan_raw(HOST, bits, words_per_sample, num_sites, group, pos, min_sites,
                         min_length, min_total, block, max_records)[:2]


def ibd_scan_host(bits: np.ndarray, words_per_sample: int, num_sites: int, group=None, pos=None,
                  min_sites: int = 512, min_length: int = 0, min_total: int = 0, block=None,
                  max_records=None) -> IBDPairs:
    """``KingContext.ibd_scan`` on host memory and the host twin: no GPU."""
    return _ibd_scan(HOST, bits, words_per_sample, num_sites, group, pos, min_sites, min_length,
                     min_total, block, max_records)


def records_to_host(records, num_records: int) -> np.ndarray:
    """The first ``num_records`` rows of the ``[*, 10]`` int32 device tensor of ``ibd_scan_raw``
    as ``IBD_PAIR_DTYPE`` rows on the host by ``(sample_i, sample_j)`` (waits for the copy)."""
    return sort_records(rows_to_host(records[:num_records]))


def ibd_scan_raw_device(ctx, bits, words_per_sample: int, num_sites: int, group=None, pos=None,
                        min_sites: int = 512, min_length: int = 0, min_total: int = 0,
                        block=None, max_records=None, out=None, stream=None):
    return _ibd_scan_raw(DevicePlace(ctx, stream), bits, words_per_sample, num_sites, group, pos,
                         min_sites, min_length, min_total, block, max_records, out)[:2]


def ibd_scan_device(ctx, bits, words_per_sample: int, num_sites: int, group=None, pos=None,
                    min_sites: int = 512, min_length: int = 0, min_total: int = 0, block=None,
                    max_records=None, stream=None) -> IBDPairs:
    return _ibd_scan(DevicePlace(ctx, stream), bits, words_per_sample, num_sites, group, pos,
                     min_sites, min_length, min_total, block, max_records)
