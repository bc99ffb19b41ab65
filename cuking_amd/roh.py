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

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from .api import _count
from .ibd import (IBD_SEGMENT_DTYPE, _bridge, _device_sites, _segment_buffer, _site_array,
                  _thresholds, genome_length, segments_to_host, sort_segments)

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


def _sample_list(samples, num_stored: int):
    """``(list or None, count)``: ``samples`` as a contiguous uint32 host array; None is the
    samples ``0 .. num_stored - 1`` (the library's null list)."""
    if samples is None:
        return None, num_stored
    samples = np.asarray(samples)
    if samples.ndim != 1 or (samples.size and samples.dtype.kind not in "iu"):
        raise ValueError(f"samples must be an integer [S] array, not {samples.dtype} "
                         f"{samples.shape}")
    if samples.size and (int(samples.min()) < 0 or int(samples.max()) > 0xFFFFFFFF):
        raise ValueError("samples must fit uint32")
    return np.ascontiguousarray(samples, dtype=np.uint32), len(samples)


def roh_segments_raw_host(bits: np.ndarray, words_per_sample: int, num_sites: int, samples=None,
                          group=None, pos=None, min_sites: int = 512, min_length: int = 0,
                          bridge_sites: int = 0, segments: bool = False, max_segments=None):
    """cuking_roh_samples_host, the bare call: ``(rows, segments)`` -- one ``ROH_SAMPLE_DTYPE``
    row per entry of ``samples`` (an integer ``[S]`` array; None: every stored sample) and, with
    ``segments`` (or a ``max_segments``), the ``IBD_SEGMENT_DTYPE`` rows, else None.  Bit for bit
    what ``KingContext.roh_segments_raw`` gives.  The buffer rule is ``ibd_segments_raw_host``'s,
    four segments per sample by default."""
    assert bits.dtype == np.uint64 and bits.flags.c_contiguous
    words_per_sample = _count(words_per_sample, "words_per_sample")
    num_sites = _count(num_sites, "num_sites")
    min_sites, min_length = _thresholds(min_sites, min_length)
    bridge_sites = _bridge(bridge_sites)
    num_stored = bits.size // words_per_sample if words_per_sample else 0
    group = _site_array(group, "group", num_sites, np.int32)
    pos = _site_array(pos, "pos", num_sites, np.uint32)
    listed, count = _sample_list(samples, num_stored)
    out = np.zeros(count, dtype=ROH_SAMPLE_DTYPE)
    pad = np.zeros(4, dtype=np.uint64)
    found = C.c_uint64(0)
    want = segments or max_segments is not None

    def call(capacity):
        segs = np.zeros(max(capacity, 1), dtype=IBD_SEGMENT_DTYPE)
        return segs, _lib.load().cuking_roh_samples_host(
            (bits if bits.size else pad).ctypes.data, num_stored, words_per_sample, num_sites,
            None if group is None or not group.size else group.ctypes.data,
            None if pos is None or not pos.size else pos.ctypes.data, min_sites, min_length,
            bridge_sites, None if listed is None or not count else listed.ctypes.data, count,
            out.ctypes.data if count else None, segs.ctypes.data if want and capacity else None,
            capacity if want else 0, C.byref(found) if want else None)

    segs = _segment_buffer(call, count, want, max_segments, found)
    return out, (segs[:found.value].copy() if want else None)


def roh_segments_host(bits: np.ndarray, words_per_sample: int, num_sites: int, samples=None,
                      group=None, pos=None, min_sites: int = 512, min_length: int = 0,
                      bridge_sites: int = 0, segments: bool = False,
                      max_segments=None) -> ROHSamples:
    """``KingContext.roh_segments`` on host memory and the host twin: no GPU."""
    rows, segs = roh_segments_raw_host(bits, words_per_sample, num_sites, samples, group, pos,
                                       min_sites, min_length, bridge_sites, segments,
                                       max_segments)
    return ROHSamples(rows, genome_length(group, pos, num_sites), segs, int(min_sites),
                      int(min_length), int(bridge_sites))


def rows_to_host(rows) -> np.ndarray:
    """The ``[S, 6]`` int32 device tensor of ``roh_segments_raw`` as ``ROH_SAMPLE_DTYPE`` rows on
    the host (waits for the copy)."""
    return np.ascontiguousarray(rows.cpu().numpy()).view(ROH_SAMPLE_DTYPE).reshape(-1)


def roh_segments_raw_device(ctx, bits, words_per_sample: int, num_sites: int, samples=None,
                            group=None, pos=None, min_sites: int = 512, min_length: int = 0,
                            bridge_sites: int = 0, segments: bool = False, max_segments=None,
                            out=None, stream=None):
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
    if isinstance(samples, torch.Tensor):   # (uint32 travels as its int32 bit pattern)
        d_samples = _device_tensor(ctx.device, samples, "samples", torch.int32)
        if d_samples.dim() != 1:
            raise ValueError(f"samples must be an [S] tensor, not {tuple(d_samples.shape)}")
        count = d_samples.shape[0]
    else:
        listed, count = _sample_list(samples, num_stored)
        d_samples = None if listed is None else torch.from_numpy(listed.view(np.int32)).to(dev)
    if out is None:
        out = torch.empty((count, 6), dtype=torch.int32, device=dev)
    else:
        _device_tensor(ctx.device, out, "out", torch.int32, shape=(count, 6))
    want = segments or max_segments is not None
    found = C.c_uint64(0)
    # (uploads ran on the current stream: `stream` waits for them)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())

    def call(capacity):
        segs = torch.empty((max(capacity, 1), 4), dtype=torch.int32, device=dev)
        return segs, ctx.lib.cuking_roh_samples(
            ctx.handle, bits.data_ptr(), num_stored, words_per_sample, num_sites,
            None if d_group is None or not num_sites else d_group.data_ptr(),
            None if d_pos is None or not num_sites else d_pos.data_ptr(), min_sites, min_length,
            bridge_sites, None if d_samples is None or not count else d_samples.data_ptr(), count,
            out.data_ptr() if count else None, segs.data_ptr() if want and capacity else None,
            capacity if want else 0, C.byref(found) if want else None, _stream_handle(stream))

    segs = _segment_buffer(call, count, want, max_segments, found)
    if stream is not None:  # (converted copies are freed on return)
        for t in (d_samples, d_group, d_pos, segs):
            if t is not None:
                t.record_stream(stream)
    return out, (segs if want else None), int(found.value)


def roh_segments_device(ctx, bits, words_per_sample: int, num_sites: int, samples=None,
                        group=None, pos=None, min_sites: int = 512, min_length: int = 0,
                        bridge_sites: int = 0, segments: bool = False, max_segments=None,
                        stream=None) -> ROHSamples:
    import torch
    host_group = group.cpu().numpy() if isinstance(group, torch.Tensor) else group
    host_pos = pos.cpu().numpy().view(np.uint32) if isinstance(pos, torch.Tensor) else pos
    total = genome_length(host_group, host_pos, num_sites)
    rows, segs, found = roh_segments_raw_device(
        ctx, bits, words_per_sample, num_sites, samples, group, pos, min_sites, min_length,
        bridge_sites, segments, max_segments, stream=stream)
    if stream is not None:
        stream.synchronize()
    return ROHSamples(rows_to_host(rows), total,
                      None if segs is None else segments_to_host(segs, found), int(min_sites),
                      int(min_length), int(bridge_sites))
