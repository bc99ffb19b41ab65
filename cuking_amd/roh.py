"""Runs of homozygosity per sample: the long runs of sites in which one sample carries no
heterozygous call -- ``king --roh``, ``plink --homozyg``, ``bcftools roh`` -- and F_ROH, their
summed length over the genome's length: the inbreeding estimate that needs no allele frequency,
no principal component and no ``min_maf``, and that says WHERE the autozygosity lies.
include/cuking_amd.h "Runs of homozygosity" holds the definition: it is the scan of ``ibd.py``
of a sample with itself, with a het as the break site and one kind.

``bridge_sites`` (0, or at least 64) forgives isolated hets (genotyping errors, ``plink
--homozyg-window-het 1``): two runs of at least that many sites on either side of one het of a
group are linked, and a segment is a chain of linked runs.  0 is the strict call.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ._place import HOST, DevicePlace, tensor_to_host
from .api import _count
from .ibd import (IBD_SEGMENT_DTYPE, _place_genome_length, _scan_head, _segment_list,
                  sort_segments)

ROH_KIND = 0
# cuking_roh_sample
ROH_SAMPLE_DTYPE = np.dtype([("length", "<u8"), ("sample", "<u4"), ("segments", "<u4"),
                             ("longest", "<u4"), ("bridged", "<u4")])
assert ROH_SAMPLE_DTYPE.itemsize == 24


@dataclass
class ROHSamples:
    """What ``KingContext.roh_segments`` / ``roh_segments_host`` return, as host arrays: ``rows``
    (``ROH_SAMPLE_DTYPE`` ``[S]``, one per listed sample in list order) and its fields ``sample``
    (uint32, as listed), ``segments`` (uint32: the number of segments), ``length`` (uint64: the
    sum of their lengths), ``longest`` (uint32), ``bridged`` (uint32: the bridged hets inside
    the counted segments, 0 at ``bridge_sites = 0``); ``total_length`` (``ibd.genome_length`` of
    the call); ``segment_list`` (``IBD_SEGMENT_DTYPE`` rows in no particular order -- ``pair`` is
    the row index, ``kind`` 0 -- or None when they were not asked for); ``min_sites``,
    ``min_length`` and ``bridge_sites`` of the call."""
    rows: np.ndarray
    total_length: int
    segment_list: object
    min_sites: int
    min_length: int
    bridge_sites: int = 0

    sample = property(lambda self: self.rows["sample"])
    segments = property(lambda self: self.rows["segments"])
    length = property(lambda self: self.rows["length"])
    longest = property(lambda self: self.rows["longest"])
    bridged = property(lambda self: self.rows["bridged"])

    def froh(self) -> np.ndarray:
        """F_ROH per listed sample: ``length / total_length`` in float64 on the host; NaN when
        ``total_length`` is zero."""
        if self.total_length == 0:
            return np.full(len(self.rows), np.nan, dtype=np.float64)
        return self.length.astype(np.float64) / np.float64(self.total_length)

    def sorted(self) -> np.ndarray:
        """The segments by ``(pair, kind, first_site)`` (a copy); ValueError without a list."""
        if self.segment_list is None:
            raise ValueError("the call did not ask for the segment list (segments=True)")
        return sort_segments(self.segment_list)


def _sample_list(samples) -> np.ndarray:
    """``samples`` as a contiguous uint32 ``[S]`` host array."""
    samples = np.asarray(samples)
    if samples.ndim != 1 or (samples.size and samples.dtype.kind not in "iu"):
        raise ValueError(f"samples must be an integer [S] array, not {samples.dtype} "
                         f"{samples.shape}")
    if samples.size and (int(samples.min()) < 0 or int(samples.max()) > 0xFFFFFFFF):
        raise ValueError("samples must fit uint32")
    return np.ascontiguousarray(samples, dtype=np.uint32)


def _roh_segments_raw(place, bits, words_per_sample, num_sites, samples, group, pos, min_sites,
                      min_length, bridge_sites, segments, max_segments, out=None):
    head, num_stored, owners = _scan_head(place, bits, words_per_sample, num_sites, group, pos,
                                          min_sites, min_length)
    bridge_sites = _count(bridge_sites, "bridge_sites")
    # (None is the samples 0 .. num_stored - 1: the library's null list)
    listed = None if samples is None else place.index_list(samples, "samples", None, _sample_list)
    count = num_stored if listed is None else listed.shape[0]
    out = place.alloc(count, ROH_SAMPLE_DTYPE) if out is None else \
        place.out(out, "out", ROH_SAMPLE_DTYPE, count)
    place.uploads_done()

    def call(*tail):
        return place.fn("roh_samples")(*head, bridge_sites, place.ptr(listed), count,
                                       place.ptr(out), *tail)

    return (out, *_segment_list(place, call, count, segments or max_segments is not None,
                                max_segments))


def _roh_segments(place, bits, words_per_sample, num_sites, samples, group, pos, min_sites,
                  min_length, bridge_sites, segments, max_segments) -> ROHSamples:
    total = _place_genome_length(place, group, pos, num_sites)
    rows, segs, found = _roh_segments_raw(place, bits, words_per_sample, num_sites, samples,
                                          group, pos, min_sites, min_length, bridge_sites,
                                          segments, max_segments)
    place.finish()
    return ROHSamples(place.to_host(rows, ROH_SAMPLE_DTYPE), total,
                      None if segs is None else place.to_host(segs, IBD_SEGMENT_DTYPE, found),
                      int(min_sites), int(min_length), int(bridge_sites))


def roh_segments_raw_host(bits: np.ndarray, words_per_sample: int, num_sites: int, samples=None,
                          group=None, pos=None, min_sites: int = 512, min_length: int = 0,
                          bridge_sites: int = 0, segments: bool = False, max_segments=None):
    """cuking_roh_samples_host, the bare call: ``(rows, segments)`` -- one ``ROH_SAMPLE_DTYPE``
    row per entry of ``samples`` (an integer ``[S]`` array; None: every stored sample) and, with
    ``segments`` (or a ``max_segments``), the ``IBD_SEGMENT_DTYPE`` rows, else None.  Bit for bit
    what ``KingContext.roh_segments_raw`` gives.  The buffer rule is ``ibd_segments_raw_host``'s,
    four segments per sample by default."""
    return _roh_segments_raw(HOST, bits, words_per_sample, num_sites, samples, group, pos,
                             min_sites, min_length, bridge_sites, segments, max_segments)[:2]


def roh_segments_host(bits: np.ndarray, words_per_sample: int, num_sites: int, samples=None,
                      group=None, pos=None, min_sites: int = 512, min_length: int = 0,
                      bridge_sites: int = 0, segments: bool = False,
                      max_segments=None) -> ROHSamples:
    """``KingContext.roh_segments`` on host memory and the host twin: no GPU."""
    return _roh_segments(HOST, bits, words_per_sample, num_sites, samples, group, pos, min_sites,
                         min_length, bridge_sites, segments, max_segments)


def rows_to_host(rows) -> np.ndarray:
    """The ``[S, 6]`` int32 device tensor of ``roh_segments_raw`` as ``ROH_SAMPLE_DTYPE`` rows on
    the host (waits for the copy)."""
    return tensor_to_host(rows, ROH_SAMPLE_DTYPE)


def roh_segments_raw_device(ctx, bits, words_per_sample: int, num_sites: int, samples=None,
                            group=None, pos=None, min_sites: int = 512, min_length: int = 0,
                            bridge_sites: int = 0, segments: bool = False, max_segments=None,
                            out=None, stream=None):
    return _roh_segments_raw(DevicePlace(ctx, stream), bits, words_per_sample, num_sites, samples,
                             group, pos, min_sites, min_length, bridge_sites, segments,
                             max_segments, out)


def roh_segments_device(ctx, bits, words_per_sample: int, num_sites: int, samples=None,
                        group=None, pos=None, min_sites: int = 512, min_length: int = 0,
                        bridge_sites: int = 0, segments: bool = False, max_segments=None,
                        stream=None) -> ROHSamples:
    return _roh_segments(DevicePlace(ctx, stream), bits, words_per_sample, num_sites, samples,
                         group, pos, min_sites, min_length, bridge_sites, segments, max_segments)
