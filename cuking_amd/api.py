"""Host-side mirror of the reference's interface for the KING hot path.

Names follow cuking.cu: ``Submatrix`` (:129-179) with ``NumRows / NumCols /
NumSamples / Contains / SampleOffset``, ``KingResult`` records (:182-186), and
``KingContext.compute_king`` taking exactly the arguments of
``ComputeKingKernel`` (:191-195).  Everything is executed by libcuking_amd.so
through the C ABI (include/cuking_amd.h); torch only provides device memory
and the stream handle.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import CSubmatrix, CukingError, check

# cuking.cu:182-186
KING_RESULT_DTYPE = np.dtype(
    [("sample_i", "<u4"), ("sample_j", "<u4"), ("kin", "<f4"),
     ("ibs0", "<u4"), ("ibs1", "<u4"), ("ibs2", "<u4")])
KING_COUNTS_DTYPE = np.dtype(
    [("het_i", "<u4"), ("het_j", "<u4"), ("both_het", "<u4"),
     ("opposing_hom", "<u4"), ("concordant_hom", "<u4"), ("shared", "<u4")])

DEFAULT_KIN_THRESHOLD = 0.0884   # cuking.cu:43
DEFAULT_MAX_RESULTS = 10 << 20   # cuking.cu:40
# The KING cut-offs: 3rd / 2nd / 1st degree, duplicate (ascending, as the library wants them)
KING_CUTOFFS = (0.0442, 0.0884, 0.177, 0.354)


class ResourceExhaustedError(RuntimeError):
    """cuking.cu:747-751."""


class Submatrix:
    """cuking.cu:129-179: block (block_i <= block_j) of the relatedness matrix
    selected by ``shard_index`` out of ``split_factor*(split_factor+1)/2``."""

    def __init__(self, num_samples: int, split_factor: int = 1,
                 shard_index: int = 0):
        self.c = CSubmatrix()
        check(_lib.load().cuking_submatrix_init(
            C.byref(self.c), num_samples, split_factor, shard_index))

    @classmethod
    def from_ranges(cls, i_begin, i_end, j_begin, j_end) -> "Submatrix":
        self = cls.__new__(cls)
        self.c = CSubmatrix(i_begin, i_end, j_begin, j_end)
        return self

    i_begin = property(lambda s: s.c.i_begin)
    i_end = property(lambda s: s.c.i_end)
    j_begin = property(lambda s: s.c.j_begin)
    j_end = property(lambda s: s.c.j_end)

    def NumRows(self) -> int:
        return _lib.load().cuking_submatrix_num_rows(C.byref(self.c))

    def NumCols(self) -> int:
        return _lib.load().cuking_submatrix_num_cols(C.byref(self.c))

    def NumSamples(self) -> int:
        return _lib.load().cuking_submatrix_num_samples(C.byref(self.c))

    def Contains(self, index: int) -> bool:
        return bool(_lib.load().cuking_submatrix_contains(C.byref(self.c), index))

    def SampleOffset(self, index: int) -> int:
        return _lib.load().cuking_submatrix_sample_offset(C.byref(self.c), index)

    def NumPairs(self) -> int:
        return _lib.load().cuking_submatrix_num_pairs(C.byref(self.c))

    def as_tuple(self):
        return (self.i_begin, self.i_end, self.j_begin, self.j_end)

    def __repr__(self):
        return "Submatrix(i=[%d,%d), j=[%d,%d))" % self.as_tuple()


def padded_sites(num_sites: int) -> int:
    return _lib.load().cuking_padded_sites(num_sites)


def words_per_sample(num_sites: int) -> int:
    return _lib.load().cuking_words_per_sample(num_sites)


def bytes_per_pair(wps: int) -> int:
    return _lib.load().cuking_bytes_per_pair(wps)


def new_host_bitset(sm: Submatrix, num_sites: int) -> np.ndarray:
    """All-missing host bitset (cuking.cu:513-523)."""
    return np.full((sm.NumSamples(), words_per_sample(num_sites)),
                   np.uint64(0xFFFFFFFFFFFFFFFF), dtype=np.uint64)


def pack_host(sm: Submatrix, bit_set: np.ndarray, row_idx, col_idx,
              n_alt_alleles) -> None:
    """cuking.cu:675-703 on host memory (thread-safe relaxed atomics)."""
    row_idx = np.ascontiguousarray(row_idx, dtype=np.int64)
    col_idx = np.ascontiguousarray(col_idx, dtype=np.int64)
    n_alt = np.ascontiguousarray(n_alt_alleles, dtype=np.int32)
    assert bit_set.dtype == np.uint64 and bit_set.flags.c_contiguous
    assert row_idx.size == col_idx.size == n_alt.size
    check(_lib.load().cuking_pack_host(
        C.byref(sm.c), bit_set.shape[1], bit_set.ctypes.data,
        row_idx.ctypes.data, col_idx.ctypes.data, n_alt.ctypes.data,
        row_idx.size))


def pack_bed_host(sm: Submatrix, bit_set: np.ndarray, bed_rows, row_bytes: int,
                  site_begin: int, site_end: int, num_sites: int) -> None:
    """cuking_pack_bed_host: rows [site_begin, site_end) of a variant-major PLINK .bed
    (``bed_rows``: uint8, the row of ``site_begin`` first, ``row_bytes`` apart) into the
    block's host bitset.  Plain stores: the words of the chunk are overwritten, whatever
    ``bit_set`` held (include/cuking_amd.h has the mapping and the refused arguments)."""
    rows = np.ascontiguousarray(bed_rows, dtype=np.uint8).reshape(-1)
    assert bit_set.dtype == np.uint64 and bit_set.flags.c_contiguous
    if rows.size < (site_end - site_begin) * row_bytes:
        raise ValueError(f"bed_rows holds {rows.size} bytes, sites [{site_begin}, {site_end}) "
                         f"need {(site_end - site_begin) * row_bytes}")
    check(_lib.load().cuking_pack_bed_host(
        C.byref(sm.c), bit_set.shape[1] if bit_set.ndim == 2 else words_per_sample(num_sites),
        bit_set.ctypes.data, rows.ctypes.data, row_bytes, site_begin, site_end, num_sites))


def site_mask_words(keep) -> np.ndarray:
    """A bool array of ``num_sites`` -> the mask words the library takes: uint64
    ``[words_per_sample(num_sites) / 2]``, site s = bit ``s & 63`` of word ``s >> 6``."""
    keep = np.asarray(keep).astype(bool).reshape(-1)
    plane = words_per_sample(keep.size) // 2
    padded = np.zeros(plane * 64, dtype=np.uint8)
    padded[:keep.size] = keep
    return np.packbits(padded, bitorder="little").view("<u8").astype(np.uint64)


def site_mask_bool(keep_words, num_sites: int) -> np.ndarray:
    """The mask words of ``num_sites`` sites -> a bool array of ``num_sites``."""
    words = np.ascontiguousarray(keep_words, dtype=np.uint64).astype("<u8")
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:num_sites].astype(bool)


def _host_counts(counts, plane: int) -> np.ndarray:
    counts = np.asarray(counts)
    if counts.dtype not in (np.dtype(np.uint32), np.dtype(np.int32)) or \
            counts.shape != (plane * 64, 4):
        raise ValueError(f"counts must be a uint32 (or int32) array of shape ({plane * 64}, 4), "
                         f"not {counts.dtype} {counts.shape}")
    return np.ascontiguousarray(counts).view(np.uint32)


def site_mask_host(counts, num_sites: int, min_call_rate: float = 0.0, min_maf: float = 0.0,
                   min_mac: int = 0, also=None):
    """cuking_site_mask_host, the site rule: from the ``[64 P, 4]`` site counts (hom_ref,
    het, hom_var, missing per plane site, as ``site_counts`` gives them) the mask of the sites
    with a called genotype, ``called / n >= min_call_rate``, ``minor / (2 called) >= min_maf``
    and ``minor >= min_mac`` (include/cuking_amd.h has the exact comparisons); ``also``: a
    bool array of ``num_sites`` ANDed in (an LD-pruned list, a region).  Returns
    ``(keep_words, num_kept)``: uint64 ``[P]`` as ``compact_sites`` takes them."""
    num_sites = _count(num_sites, "num_sites")
    plane = words_per_sample(num_sites) // 2
    counts = _host_counts(counts, plane)
    also_words = None
    if also is not None:
        also = np.asarray(also)
        if also.shape != (num_sites,):
            raise ValueError(f"also must hold {num_sites} entries, not {also.shape}")
        also_words = site_mask_words(also)
    rule = _lib.CSiteFilter(float(min_call_rate), float(min_maf), _count(min_mac, "min_mac"))
    keep = np.zeros(plane, dtype=np.uint64)
    kept = C.c_uint32(0)
    check(_lib.load().cuking_site_mask_host(
        counts.ctypes.data, num_sites, plane, C.byref(rule),
        also_words.ctypes.data if also_words is not None else None, keep.ctypes.data,
        C.byref(kept)))
    return keep, int(kept.value)


HWE_MIDP = 1  # CUKING_HWE_MIDP


def hwe_sites_host(counts, num_sites: int, midp: bool = False) -> np.ndarray:
    """cuking_hwe_sites_host, the Hardy-Weinberg exact test per site: from the ``[*, 4]`` site
    counts (hom_ref, het, hom_var, missing per site, as ``site_counts`` gives them; missing is
    ignored) the p-value of each of the first ``num_sites`` rows as float64 ``[num_sites]``.
    ``midp``: the mid-p form (half the observed table's probability leaves the tail).  1.0 where
    nothing was called, NaN above 2^24 people (include/cuking_amd.h has the walk, operation by
    operation: the device call returns the same bytes)."""
    num_sites = _count(num_sites, "num_sites")
    counts = np.asarray(counts)
    if counts.dtype not in (np.dtype(np.uint32), np.dtype(np.int32)) or counts.ndim != 2 or \
            counts.shape[1] != 4 or counts.shape[0] < num_sites:
        raise ValueError(f"counts must be a uint32 (or int32) array of at least {num_sites} rows "
                         f"of 4, not {counts.dtype} {counts.shape}")
    counts = np.ascontiguousarray(counts).view(np.uint32)
    p = np.empty(num_sites, dtype=np.float64)
    check(_lib.load().cuking_hwe_sites_host(counts.ctypes.data, num_sites,
                                            HWE_MIDP if midp else 0, p.ctypes.data))
    return p


def _min_hwe_p(min_hwe_p) -> float:
    value = float(min_hwe_p)
    if not 0.0 <= value <= 1.0:  # (NaN fails)
        raise ValueError(f"min_hwe_p ({min_hwe_p}) must be in [0, 1]")
    return value


def hwe_site_mask(p, min_hwe_p: float, also=None) -> np.ndarray:
    """The Hardy-Weinberg rule of ``filter_sites`` on host arrays: site s passes iff ``p[s] >=
    min_hwe_p`` as doubles -- false for NaN -- and ``also[s]``, where ``also`` (a bool array of
    the same length) is given.  Returns the bool array that goes on as ``also``."""
    p = np.asarray(p, dtype=np.float64).reshape(-1)
    with np.errstate(invalid="ignore"):
        keep = p >= _min_hwe_p(min_hwe_p)
    if also is not None:
        also = np.asarray(also)
        if also.shape != p.shape:
            raise ValueError(f"also must hold {p.size} entries, not {also.shape}")
        keep &= also.astype(bool)
    return keep


def _keep_words(keep_words, words_per_sample_in: int) -> np.ndarray:
    keep = np.ascontiguousarray(keep_words, dtype=np.uint64).reshape(-1)
    if keep.size != words_per_sample_in // 2:
        raise ValueError(f"keep_words must hold {words_per_sample_in // 2} words (one per plane "
                         f"word), not {keep.size}")
    return keep


def _popcount(words: np.ndarray) -> int:
    return int(np.unpackbits(np.ascontiguousarray(words).view(np.uint8)).sum())


def compact_sites_host(bit_sets: np.ndarray, words_per_sample_in: int, keep_words,
                       num_sites: int, out=None):
    """cuking_compact_sites_host: the host bitset ``[rows, words_per_sample_in]`` restricted
    to the sites of ``keep_words`` -- the k-th kept site becomes site k, what follows the
    last one is missing -- as ``(new_bits, new_words_per_sample, num_kept)``.  ``out``: a
    uint64 ``[rows, words_per_sample(num_kept)]`` array to write into."""
    assert bit_sets.dtype == np.uint64 and bit_sets.flags.c_contiguous
    keep = _keep_words(keep_words, words_per_sample_in)
    rows = bit_sets.size // words_per_sample_in
    kept = _popcount(keep)
    wps_out = words_per_sample(max(kept, 1))
    if out is None:
        out = np.empty((rows, wps_out), dtype=np.uint64)
    assert out.dtype == np.uint64 and out.flags.c_contiguous and out.size >= rows * wps_out
    check(_lib.load().cuking_compact_sites_host(
        bit_sets.ctypes.data, rows, words_per_sample_in, keep.ctypes.data, num_sites,
        out.ctypes.data, wps_out))
    return out, wps_out, kept


def ld_site_words(num_stored: int) -> int:
    """Q: the uint64 words of one plane of one site in the site-major bitset."""
    return int(_lib.load().cuking_ld_site_words(_count(num_stored, "num_stored")))


def transpose_sites_host(bit_sets: np.ndarray, words_per_sample: int, num_sites: int, out=None):
    """cuking_transpose_sites_host: the host bitset ``[rows, words_per_sample]`` as the
    site-major bitset uint64 ``[num_sites, 2, Q]`` (plane 0 het, plane 1 hom_var, sample s =
    bit ``s % 64`` of word ``s // 64``, the tail of the last word set: missing)."""
    assert bit_sets.dtype == np.uint64 and bit_sets.flags.c_contiguous
    num_sites = _count(num_sites, "num_sites")
    rows = bit_sets.size // words_per_sample if words_per_sample else 0
    q = ld_site_words(rows)
    if out is None:
        out = np.empty((num_sites, 2, q), dtype=np.uint64)
    assert out.dtype == np.uint64 and out.flags.c_contiguous and out.size >= num_sites * 2 * q
    # (an empty array has no address worth passing: the library refuses NULL, not "nothing")
    pad = np.zeros(1, dtype=np.uint64)
    check(_lib.load().cuking_transpose_sites_host(
        (bit_sets if bit_sets.size else pad).ctypes.data, rows, words_per_sample, num_sites,
        (out if out.size else pad).ctypes.data, q))
    return out


def _ld_arguments(window, r2):
    window = _count(window, "window")
    if window < 2:
        raise ValueError(f"window must be at least 2 variants, not {window}")
    r2 = float(np.float32(r2))
    if not 0.0 <= r2 <= 1.0:
        raise ValueError(f"r2 must be in [0, 1], not {r2}")
    return min(window, 0xFFFFFFFF), r2


def _ld_default_records(num_sites: int, window: int) -> int:
    return max(1, min(num_sites * (window - 1), 4 * num_sites))


def _counted_buffer(call, default: int, max_items, name: str, found, attr: str):
    """THE buffer rule of every call with a counted output (LD edges, PC-Relate and IBD scan
    records, IBD and ROH segments): ``call(capacity)`` makes a buffer of ``capacity`` items (or
    takes the caller's ``out``), calls the library and returns ``(buffer, status)``; ``found``
    is the ``c_uint64`` the library counts into.  Without ``max_items`` (the user's ``name``
    argument) the buffer holds ``default`` items and the call is repeated once with the exact
    count if that overflows; with it an overflow raises ``ResourceExhaustedError`` whose
    ``attr`` (``num_records`` / ``num_segments``) is the exact count.  A list that is not
    wanted is ``default`` 0 with no counter given to the library: it cannot overflow.
    Returns the buffer of the call that succeeded."""
    grow = max_items is None
    buffer, status = call(default if grow else _count(max_items, name))
    if status == _lib.ERR_RESOURCE_EXHAUSTED and grow:
        buffer, status = call(int(found.value))
    if status == _lib.ERR_RESOURCE_EXHAUSTED:
        e = ResourceExhaustedError(_lib.load().cuking_last_error().decode())
        setattr(e, attr, int(found.value))
        raise e
    check(status)
    return buffer


def _out_capacity(out, max_records):
    """``max_records`` of a call that writes into the caller's ``out``: its rows by default, and
    never more than them."""
    max_records = out.shape[0] if max_records is None else max_records
    if _count(max_records, "max_records") > out.shape[0]:
        raise ValueError(f"out holds {out.shape[0]} records, max_records is {max_records}")
    return max_records


def _ld_edges(place, site_bits, num_sites, num_stored, window, r2, group, max_records,
              out=None):
    num_sites, num_stored = _count(num_sites, "num_sites"), _count(num_stored, "num_stored")
    window, r2 = _ld_arguments(window, r2)
    have, need = place.words(site_bits, "site_bits"), num_sites * 2 * ld_site_words(num_stored)
    if have != need:
        raise ValueError(f"site_bits holds {have} words, {num_sites} sites of {num_stored} "
                         f"samples take {need} (transpose_sites)")
    group = place.sites(group, "group", num_sites, np.int32)
    if out is not None:
        place.out(out, "out", KING_RESULT_DTYPE)
        max_records = _out_capacity(out, max_records)
    count = C.c_uint64(0)
    place.uploads_done()

    def call(capacity):
        recs = out if out is not None else place.alloc(max(capacity, 1), KING_RESULT_DTYPE)
        return recs, place.fn("ld_edges")(
            place.ptr(site_bits, pad=True), num_sites, num_stored, window, r2, place.ptr(group),
            place.ptr(recs, pad=True), capacity, C.byref(count))

    recs = _counted_buffer(call, _ld_default_records(num_sites, window), max_records,
                           "max_records", count, "num_records")
    place.keep()
    return place.trim(recs, count.value), int(count.value)


def ld_edges_host(site_bits: np.ndarray, num_sites: int, num_stored: int, window: int = 50,
                  r2: float = 0.2, group=None, max_records=None):
    """cuking_ld_edges_host: the pairs of sites ``a < b``, ``b - a < window``, of one
    ``group``, whose r^2 over the jointly called samples is above ``r2`` (include/cuking_amd.h
    "LD pruning" has the exact rule), as ``(records, count)``: KING_RESULT_DTYPE records with
    ``sample_i = a``, ``sample_j = b``, ``kin`` = r^2 and ``ibs0`` = the jointly called
    samples, sorted by (a, b).  Without ``max_records`` the buffer is sized like the device
    wrapper's and grown once to the exact count; with it, an overflow raises
    ``ResourceExhaustedError`` whose ``num_records`` is the exact count."""
    from ._place import HOST
    recs, count = _ld_edges(HOST, site_bits, num_sites, num_stored, window, r2, group, max_records)
    return sort_results(recs), count


def _geno_matmul(place, bits, words_per_row, num_cols, table, rhs, per_row, out):
    words_per_row, num_cols = _count(words_per_row, "words_per_row"), _count(num_cols, "num_cols")
    rows = place.bits(bits, words_per_row)
    table, ldt = place.matrix(table, "table", rows if per_row else num_cols, 4)
    if table.shape[0] > 1 and ldt != 4:
        raise ValueError("table must be contiguous")
    rhs, ldr = place.matrix(rhs, "rhs", num_cols)
    num_rhs = rhs.shape[1]
    if out is None:
        out = place.alloc((rows, num_rhs), np.float32)
    out, ldo = place.matrix(out, "out", rows, num_rhs)
    check(place.fn("geno_matmul")(
        place.ptr(bits, pad=True), rows, words_per_row, num_cols, place.ptr(table, pad=True),
        _lib.GENO_TABLE_PER_ROW if per_row else _lib.GENO_TABLE_PER_COLUMN,
        place.ptr(rhs, pad=True), ldr, num_rhs, place.ptr(out, pad=True), ldo))
    return out


def geno_matmul_host(bits: np.ndarray, words_per_row: int, num_cols: int, table, rhs,
                     per_row: bool = False, out=None) -> np.ndarray:
    """cuking_geno_matmul_host: ``out[r, c] = sum_k table[r or k, code(r, k)] * rhs[k, c]`` over
    the columns ``k < num_cols`` of the host bitset ``[rows, words_per_row]`` (a row is its het
    words, then its hom_var words; code 0 hom-ref, 1 het, 2 hom-var, 3 missing), accumulated in
    double and rounded once: the specification of ``KingContext.geno_matmul`` in executable
    form.  ``table``: float32 ``[num_cols, 4]``, or ``[rows, 4]`` with ``per_row``; ``rhs``:
    float32 ``[num_cols, num_rhs]``; ``out``: float32 ``[rows, num_rhs]`` to write into (both
    may be column slices of wider arrays: their row pitch is passed on)."""
    from ._place import HOST
    return _geno_matmul(HOST, bits, words_per_row, num_cols, table, rhs, per_row, out)


def ld_priority_host(counts, num_sites: int) -> np.ndarray:
    """cuking_ld_priority per site: float32 ``[num_sites]`` from the ``[64 P, 4]`` site counts
    -- the minor allele frequency among the called genotypes, NaN without one (ranked last)."""
    num_sites = _count(num_sites, "num_sites")
    counts = _host_counts(counts, words_per_sample(num_sites) // 2)
    fn = _lib.load().cuking_ld_priority
    return np.array([fn(counts[s].ctypes.data) for s in range(num_sites)], dtype=np.float32)


def sort_results(results: np.ndarray) -> np.ndarray:
    """cuking.cu:761-765 (in place)."""
    assert results.dtype == KING_RESULT_DTYPE and results.flags.c_contiguous
    _lib.load().cuking_sort_results(results.ctypes.data, results.size)
    return results


def device_count() -> int:
    return _lib.load().cuking_device_count()


def synth_models() -> list:
    """Names of the synthetic generator's cohort models, by number (the library's table)."""
    lib = _lib.load()
    return [lib.cuking_synth_model_name(k).decode() for k in range(lib.cuking_synth_num_models())]


def synth_model_number(model) -> int:
    """A cohort model given by number or by name -> its number; ValueError if unknown."""
    names = synth_models()
    if isinstance(model, str):
        if model not in names:
            raise ValueError(f"unknown synthetic cohort model '{model}' (known: {', '.join(names)})")
        return names.index(model)
    if isinstance(model, bool) or int(model) != model or not 0 <= int(model) < len(names):
        raise ValueError(f"unknown synthetic cohort model {model!r} (0..{len(names) - 1})")
    return int(model)


@dataclass
class KernelTiming:
    king_ms: float
    king_launches: int
    prepare_ms: float
    prepare_launches: int


def _stream_handle(stream=None) -> int:
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return int(s.cuda_stream)


def _device_tensor(device: int, t, name: str, dtype, shape=None, min_numel=None, cols=None,
                   contiguous: bool = True):
    """``t`` if it is a torch tensor of ``dtype`` on GPU ``device``, contiguous (unless told
    otherwise), of ``shape`` / at least ``min_numel`` elements / ``[*, cols]`` where given;
    ValueError otherwise."""
    import torch
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a device tensor, not {type(t).__name__}")
    if not t.is_cuda or t.device.index != device:
        raise ValueError(f"{name} must live on this context's GPU")
    if t.dtype != dtype or contiguous and not t.is_contiguous():
        raise ValueError(f"{name} must be a {'contiguous ' if contiguous else ''}"
                         f"{str(dtype).replace('torch.', '')} tensor")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, not {tuple(t.shape)}")
    if cols is not None and (t.dim() != 2 or t.shape[1] != cols):
        raise ValueError(f"{name} must be a [*, {cols}] tensor, not {tuple(t.shape)}")
    if min_numel is not None and t.numel() < min_numel:
        raise ValueError(f"{name} holds {t.numel()} elements, {min_numel} are needed")
    return t


def _whole_or_tiles(fn, fn_tiles, head, tile_range, tail) -> None:
    """The entry point of the whole block, or its ``_tiles`` twin with the tile range between
    the arguments the two share."""
    if tile_range is None:
        check(fn(*head, *tail))
    else:
        check(fn_tiles(*head, tile_range[0], tile_range[1], *tail))


class KingContext:
    """One per GPU (cuking_ctx).  Device buffers are torch tensors on that GPU;
    bitsets are int64 tensors holding the reference's uint64 words."""

    def __init__(self, device: int = 0):
        self.lib = _lib.load()
        self.device = device
        h = C.c_void_p()
        check(self.lib.cuking_ctx_create(device, C.byref(h)))
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            self.lib.cuking_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- options ------------------------------------------------------------
    def set_kernel(self, name: str) -> None:
        kernel = {"tiled": _lib.KERNEL_TILED, "stream": _lib.KERNEL_STREAM}[name]
        check(self.lib.cuking_ctx_set_kernel(self.handle, kernel))

    def set_option(self, key: str, value: int) -> None:
        check(self.lib.cuking_ctx_set_option(self.handle, key.encode(), value))

    def get_option(self, key: str) -> int:
        value = C.c_int64(0)
        check(self.lib.cuking_ctx_get_option(self.handle, key.encode(), C.byref(value)))
        return int(value.value)

    def variant_name(self, variant: int | None = None) -> str:
        v = self.get_option("variant") if variant is None else variant
        return self.lib.cuking_variant_name(v).decode()

    def num_tiles(self, sm: Submatrix) -> int:
        return self.lib.cuking_num_tiles(self.handle, C.byref(sm.c))

    def tile_samples(self) -> int:
        return self.lib.cuking_tile_samples(self.handle)

    # -- memory -------------------------------------------------------------
    def _tensor(self, shape, dtype):
        import torch
        return torch.empty(shape, dtype=dtype, device=f"cuda:{self.device}")

    def upload_bitset(self, host_bits: np.ndarray):
        import torch
        t = torch.from_numpy(host_bits.view(np.int64))
        return t.to(f"cuda:{self.device}", non_blocking=False)

    # -- hot path -----------------------------------------------------------
    def compute_king(self, submatrix: Submatrix, words_per_sample: int,
                     bit_sets, kin_threshold: float, max_results: int, results,
                     result_index, result_overflow, stream=None,
                     tile_range=None) -> None:
        """ComputeKingKernel (cuking.cu:191-195) + its launch (:734-741):
        appends to ``results`` (device, [max_results, 6] int32 = KingResult
        records) and bumps ``result_index`` / ``result_overflow`` (device u32,
        not reset here).  Asynchronous on the stream."""
        self._check_bits(submatrix, words_per_sample, bit_sets)
        assert results.numel() * results.element_size() >= max_results * 24
        _whole_or_tiles(self.lib.cuking_compute_king, self.lib.cuking_compute_king_tiles,
                        self._block(submatrix, words_per_sample, bit_sets), tile_range,
                        (kin_threshold, max_results, results.data_ptr(), result_index.data_ptr(),
                         result_overflow.data_ptr(), _stream_handle(stream)))

    def prepare_samples(self, submatrix: Submatrix, words_per_sample: int,
                        bit_sets, sample_begin: int, sample_end: int,
                        stream=None) -> None:
        """Staged operator, step 1 (diagonal block): convert samples
        [sample_begin, sample_end) into the kernel layout."""
        self._check_bits(submatrix, words_per_sample, bit_sets)
        check(self.lib.cuking_prepare_samples(
            *self._block(submatrix, words_per_sample, bit_sets), sample_begin, sample_end,
            _stream_handle(stream)))

    def compute_king_rect(self, submatrix: Submatrix, words_per_sample: int,
                          bit_sets, rows, cols, kin_threshold: float,
                          max_results: int, results, result_index,
                          result_overflow, stream=None) -> None:
        """Staged operator, step 2: pairs (i < j) of rows x cols from the
        prepared layout; appends like compute_king.  rows = (begin, end) or
        (begin, end, step): every tile row, or every (step / tile)-th one;
        cols = (begin, end); sample indices."""
        self._check_bits(submatrix, words_per_sample, bit_sets)
        assert results.numel() * results.element_size() >= max_results * 24
        step = rows[2] if len(rows) > 2 else 0
        check(self.lib.cuking_compute_king_rect(
            *self._block(submatrix, words_per_sample, bit_sets), rows[0], rows[1], step, cols[0],
            cols[1], kin_threshold, max_results, results.data_ptr(), result_index.data_ptr(),
            result_overflow.data_ptr(), _stream_handle(stream)))

    def reserve(self, submatrix: Submatrix, words_per_sample: int, streams=()) -> None:
        """Sizes the workspace for the block (and the split slabs of the
        streams named) up front: later compute / prepare calls on those streams
        neither allocate nor wait for the device."""
        handles = (C.c_void_p * max(len(streams), 1))(
            *[_stream_handle(s) for s in streams])
        check(self.lib.cuking_ctx_reserve(
            self.handle, C.byref(submatrix.c), words_per_sample, handles, len(streams)))

    def invalidate(self) -> None:
        """The bitset behind the pointer last converted has been rewritten in
        place (only matters with the option "reuse_prepared")."""
        check(self.lib.cuking_invalidate(self.handle))

    def compute_counts(self, submatrix: Submatrix, words_per_sample: int,
                       bit_sets, stream=None) -> np.ndarray:
        """Diagnostic: the six sums (cuking.cu:232-239) of every pair, as a
        [NumRows, NumCols] array (entries with i >= j are zero)."""
        import torch
        self._check_bits(submatrix, words_per_sample, bit_sets)
        r, c = submatrix.NumRows(), submatrix.NumCols()
        out = torch.zeros((r, c, 6), dtype=torch.int32,
                          device=f"cuda:{self.device}")
        check(self.lib.cuking_compute_counts(
            *self._block(submatrix, words_per_sample, bit_sets), out.data_ptr(),
            _stream_handle(stream)))
        torch.cuda.synchronize(self.device)
        return out.cpu().numpy().view(np.uint32).reshape(r, c, 6).view(
            KING_COUNTS_DTYPE).reshape(r, c)

    def kin_matrix(self, submatrix: Submatrix, words_per_sample: int, bit_sets,
                   out=None, symmetric: bool = False, tile_range=None, stream=None):
        """Dense kinship matrix (cuking_compute_kin_matrix): the float32 kinship of
        every pair of the block as a [NumRows, NumCols] device tensor, pair (i, j)
        at [i - i_begin, j - j_begin]; no threshold, no records.  Does not
        synchronise.  A diagonal block gets its entries with i < j; with
        ``symmetric`` also the mirrored ones and the diagonal (0.5, or NaN for a
        sample without a het site).  ``out``: a float32 tensor of that shape on
        this GPU to write into, possibly a view with a row pitch of its own
        (``stride(1) == 1``); entries the call does not write keep what they hold.
        Without it the result is allocated and untouched entries are NaN.
        ``tile_range``: only the tiles [begin, end) of the block's enumeration
        (``num_tiles``), as in ``compute_king``."""
        import torch
        self._check_bits(submatrix, words_per_sample, bit_sets)
        r, c = submatrix.NumRows(), submatrix.NumCols()
        if out is None:
            out = torch.full((r, c), float("nan"), dtype=torch.float32,
                             device=f"cuda:{self.device}")
        else:
            _device_tensor(self.device, out, "out", torch.float32, shape=(r, c), contiguous=False)
            if r > 1 and c > 0 and out.stride(0) < c or c > 1 and out.stride(1) != 1:
                raise ValueError("out must have unit column stride and a row stride of at "
                                 "least NumCols")
        if symmetric and submatrix.i_begin != submatrix.j_begin:
            raise ValueError("symmetric=True needs a diagonal block")
        if symmetric and tile_range is not None:
            raise ValueError("symmetric=True cannot be combined with a tile_range")
        if r == 0 or c == 0:
            return out
        ld = out.stride(0) if r > 1 else max(out.stride(0), c)
        flags = _lib.KIN_SYMMETRIC if symmetric else _lib.KIN_UPPER
        _whole_or_tiles(self.lib.cuking_compute_kin_matrix,
                        self.lib.cuking_compute_kin_matrix_tiles,
                        self._block(submatrix, words_per_sample, bit_sets), tile_range,
                        (out.data_ptr(), ld, flags, _stream_handle(stream)))
        return out

    def kin_summary(self, submatrix: Submatrix, words_per_sample: int, bit_sets,
                    lo: float = -1.0, hi: float = 0.5, bins: int = 1536, hist=None,
                    best=None, tile_range=None, stream=None) -> "KinSummary":
        """Kinship summary (cuking_compute_kin_summary): the histogram of the float32
        kinship of every pair of the block and every sample's nearest relative,
        without the matrix and without a threshold.  Does not synchronise; returns a
        ``KinSummary`` holding the two device tensors.  ``hist`` (``bins + 3`` int64)
        and ``best`` (``NumSamples()`` int64) are views of the library's uint64 data;
        the call ACCUMULATES into them (counts add, keys take the maximum), so the
        tensors of an earlier summary may be passed back in, e.g. for the tile
        ranges of one block.  Without them zeroed ones are allocated.
        ``tile_range``: only the tiles [begin, end) of the block's enumeration."""
        import torch
        self._check_bits(submatrix, words_per_sample, bit_sets)
        if isinstance(bins, bool) or int(bins) != bins or not 1 <= bins <= _lib.KIN_BINS_MAX:
            raise ValueError(f"bins must be an integer in [1, {_lib.KIN_BINS_MAX}]")
        lo, hi = float(np.float32(lo)), float(np.float32(hi))
        if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
            raise ValueError("the histogram needs finite bounds with lo < hi")

        def output(t, name, length):
            if t is None:
                return torch.zeros(length, dtype=torch.int64, device=f"cuda:{self.device}")
            return _device_tensor(self.device, t, name, torch.int64, shape=(length,))
        hist = output(hist, "hist", int(bins) + 3)
        best = output(best, "best", submatrix.NumSamples())
        summary = KinSummary(hist, best, lo, hi, int(bins), submatrix, self.device)
        if submatrix.NumRows() == 0 or submatrix.NumCols() == 0:
            return summary
        cbins = _lib.CKinBins(lo, hi, int(bins))
        _whole_or_tiles(self.lib.cuking_compute_kin_summary,
                        self.lib.cuking_compute_kin_summary_tiles,
                        self._block(submatrix, words_per_sample, bit_sets), tile_range,
                        (C.byref(cbins), hist.data_ptr(), best.data_ptr(), _stream_handle(stream)))
        return summary

    def relative_counts(self, submatrix: Submatrix, words_per_sample: int, bit_sets,
                        thresholds=KING_CUTOFFS, out=None, tile_range=None,
                        stream=None) -> "RelativeCounts":
        """Relative counts (cuking_compute_relative_counts): per stored sample of the
        block, the number of partners whose kinship falls in each band of ``thresholds``
        (1 to 8 finite values, strictly ascending; band t: the largest t with
        ``kin > thresholds[t]``, the comparison a record makes).  The thresholded call
        at ``thresholds[0]`` without the records: nothing can overflow.  Does not
        synchronise; returns a ``RelativeCounts`` holding the device tensor.  ``out``: a
        contiguous int32 ``[NumSamples(), len(thresholds)]`` tensor (a view of the
        library's uint32 data) the call ACCUMULATES into, e.g. for the tile ranges of
        one block; without it a zeroed one is allocated.  ``tile_range``: only the tiles
        [begin, end) of the block's enumeration."""
        self._check_bits(submatrix, words_per_sample, bit_sets)
        thr = np.asarray(thresholds, dtype=np.float32).reshape(-1)
        if not 1 <= thr.size <= _lib.REL_THRESHOLDS_MAX:
            raise ValueError(f"between 1 and {_lib.REL_THRESHOLDS_MAX} thresholds are needed")
        if not np.isfinite(thr).all() or not (np.diff(thr) > 0).all():
            raise ValueError("thresholds must be finite and strictly ascending (as float32)")
        out = self._counts_out(out, (submatrix.NumSamples(), int(thr.size)), zero=True)
        counts = RelativeCounts(out, thr, submatrix, self.device)
        if submatrix.NumRows() == 0 or submatrix.NumCols() == 0:
            return counts
        cthr = (C.c_float * thr.size)(*[float(t) for t in thr])
        _whole_or_tiles(self.lib.cuking_compute_relative_counts,
                        self.lib.cuking_compute_relative_counts_tiles,
                        self._block(submatrix, words_per_sample, bit_sets), tile_range,
                        (cthr, int(thr.size), out.data_ptr(), _stream_handle(stream)))
        return counts

    def count_records(self, submatrix: Submatrix, words_per_sample: int, bit_sets,
                      kin_threshold: float) -> int:
        """The exact number of records ``compute_king`` appends for this block at
        ``kin_threshold`` -- its smallest sufficient ``max_results`` -- from one count
        call with one threshold.  Waits for the device."""
        return self.relative_counts(submatrix, words_per_sample, bit_sets,
                                    thresholds=(kin_threshold,)).num_records(0)

    def unrelated_set(self, records, num_records: int, num_samples: int,
                      prune_threshold: float = float("-inf"), priority=None,
                      families: bool = True, stream=None) -> "UnrelatedSet":
        """Unrelated set and families from the records (cuking_unrelated_set), on the
        device.  ``records``: the device ``[*, 6]`` int32 tensor ``compute_king`` appended
        to (several shards' buffers may be concatenated; repeats count once),
        ``num_records`` its ``result_index``.  A record is an edge when ``kin >
        prune_threshold`` (strict float32).  ``priority``: an optional float32 device
        tensor of ``num_samples`` -- the higher priority is kept first, among equals the
        lower index, NaN last; without it ``-degree`` (distinct partners).  Returns an
        ``UnrelatedSet``: ``keep[s]`` = 1 iff no neighbour of s was kept before it in that
        order, ``family[s]`` = the lowest index of s's connected component.  A record that
        does not satisfy ``sample_i < sample_j < num_samples`` raises ``CukingError``
        (invalid argument).  WAITS for the stream."""
        import torch
        num_records, num_samples = _count(num_records, "num_records"), _count(num_samples,
                                                                               "num_samples")
        thr = float(np.float32(prune_threshold))
        if thr != thr:
            raise ValueError("prune_threshold must not be NaN")
        # (KingResult records; unrelated_set_host takes numpy)
        _device_tensor(self.device, records, "records", torch.int32, cols=6)
        if records.shape[0] < num_records:
            raise ValueError(f"records holds {records.shape[0]} records, num_records is "
                             f"{num_records}")
        if priority is not None:
            _device_tensor(self.device, priority, "priority", torch.float32, shape=(num_samples,))
        dev = f"cuda:{self.device}"
        keep = torch.empty(num_samples, dtype=torch.uint8, device=dev)
        family = torch.empty(num_samples, dtype=torch.int32, device=dev) if families else None
        rounds = C.c_uint32(0)
        check(self.lib.cuking_unrelated_set(
            self.handle, records.data_ptr() if num_records else None, num_records, num_samples,
            thr, priority.data_ptr() if priority is not None else None,
            keep.data_ptr() if num_samples else None,
            family.data_ptr() if families and num_samples else None, C.byref(rounds),
            _stream_handle(stream)))
        return UnrelatedSet(keep, family, int(rounds.value), thr, self.device)

    def prune(self, submatrix: Submatrix, words_per_sample: int, bit_sets,
              kin_threshold: float, priority=None, families: bool = True) -> "UnrelatedSet":
        """From bitsets to "these samples stay" for a whole-cohort diagonal block:
        ``count_records`` for the exact buffer size, ``compute_king`` at ``kin_threshold``,
        then ``unrelated_set`` on the records where they lie.  Waits for the device."""
        if not (submatrix.i_begin == submatrix.j_begin == 0 and
                submatrix.i_end == submatrix.j_end):
            raise ValueError(
                f"prune needs the whole-cohort diagonal block, not {submatrix!r}: for several "
                "shards concatenate their record buffers and call unrelated_set(records, "
                "num_records, num_samples)")
        count = self.count_records(submatrix, words_per_sample, bit_sets, kin_threshold)
        results, written, overflow = self._collect_records(
            submatrix, words_per_sample, bit_sets, kin_threshold, count,
            launch=submatrix.NumSamples() > 1)
        if overflow or written != count:
            raise RuntimeError(f"the record call wrote {written} records (overflow {overflow}), "
                               f"the count call announced {count}")
        return self.unrelated_set(results, count, submatrix.i_end, kin_threshold,
                                  priority=priority, families=families)

    def _collect_records(self, submatrix: Submatrix, words_per_sample: int, bit_sets,
                         kin_threshold: float, max_results: int, tile_range=None,
                         launch: bool = True):
        """Zeroed record buffer and index / overflow words, ``compute_king`` into them (unless
        ``launch`` is off), the wait for the device: ``(results, written, overflow)``."""
        import torch
        dev = f"cuda:{self.device}"
        results = torch.zeros((max(max_results, 1), 6), dtype=torch.int32, device=dev)
        index_and_flag = torch.zeros(2, dtype=torch.int32, device=dev)
        if launch:
            self.compute_king(submatrix, words_per_sample, bit_sets, kin_threshold, max_results,
                              results, index_and_flag[0:1], index_and_flag[1:2],
                              tile_range=tile_range)
        torch.cuda.synchronize(self.device)
        written, overflow = (int(x) & 0xFFFFFFFF for x in index_and_flag.tolist())
        return results, written, overflow

    def run(self, submatrix: Submatrix, words_per_sample: int, bit_sets,
            kin_threshold: float = DEFAULT_KIN_THRESHOLD,
            max_results: int = DEFAULT_MAX_RESULTS, tile_range=None,
            sort: bool = True) -> np.ndarray:
        """cuking.cu:713-765: allocate + zero the result buffer, launch, wait,
        raise on overflow, return the (sorted) host records."""
        results, count, overflow = self._collect_records(
            submatrix, words_per_sample, bit_sets, kin_threshold, max_results, tile_range)
        if overflow:
            raise ResourceExhaustedError(
                "Could not store all results: try increasing the "
                "--max_results parameter.")
        host = results[:count].cpu().numpy().view(np.uint32).reshape(-1)
        recs = host.view(KING_RESULT_DTYPE).copy()
        return sort_results(recs) if sort else recs

    def pack_device(self, submatrix: Submatrix, words_per_sample: int,
                    bit_set, row_idx, col_idx, n_alt_alleles, status,
                    stream=None) -> None:
        """cuking.cu:675-703 as a device kernel; all arguments device tensors
        (int64, int64, int32; status one int32, zeroed by the caller)."""
        import torch
        assert row_idx.dtype == torch.int64 and col_idx.dtype == torch.int64
        assert n_alt_alleles.dtype == torch.int32
        assert row_idx.numel() == col_idx.numel() == n_alt_alleles.numel()
        check(self.lib.cuking_pack_device(
            self.handle, C.byref(submatrix.c), words_per_sample,
            bit_set.data_ptr(), row_idx.data_ptr(), col_idx.data_ptr(),
            n_alt_alleles.data_ptr(), row_idx.numel(), status.data_ptr(),
            _stream_handle(stream)))

    def pack_bed(self, submatrix: Submatrix, words_per_sample: int, bed_rows, row_bytes: int,
                 site_begin: int, site_end: int, num_sites: int, out, stream=None) -> None:
        """cuking_pack_bed_device: rows [site_begin, site_end) of a variant-major PLINK
        .bed -- ``bed_rows``, a uint8 device tensor (any alignment: a view into a larger
        buffer is fine), the row of ``site_begin`` first -- into the block's device bitset
        ``out``.  A bit transpose with plain stores: the words of the chunk are overwritten
        whatever ``out`` held, chunks covering [0, num_sites) write every word, no memset.
        Asynchronous on the stream."""
        import torch
        self._check_bits(submatrix, words_per_sample, out)
        _device_tensor(self.device, bed_rows, "bed_rows", torch.uint8)
        if site_begin <= site_end and bed_rows.numel() < (site_end - site_begin) * row_bytes:
            raise ValueError(f"bed_rows holds {bed_rows.numel()} bytes, sites [{site_begin}, "
                             f"{site_end}) need {(site_end - site_begin) * row_bytes}")
        if submatrix.NumSamples() == 0 or site_begin == site_end:
            return
        check(self.lib.cuking_pack_bed_device(
            self.handle, C.byref(submatrix.c), words_per_sample, out.data_ptr(),
            bed_rows.data_ptr(), row_bytes, site_begin, site_end, num_sites,
            _stream_handle(stream)))

    def load_bed(self, prefix, submatrix: Submatrix, chunk_bytes: int = 64 << 20, out=None):
        """The block's device bitset from ``PREFIX.bed / .bim / .fam`` (cuking_amd.plink):
        the file is read in chunks of a multiple of 64 sites (about ``chunk_bytes`` each)
        into two pinned staging tensors, copied on a copy stream and transposed by
        ``pack_bed`` on a pack stream, ordered by events -- the host only waits where a
        staging tensor has to come free.  Nothing is sized by the whole file but the
        result: ``[max(NumSamples, 1), words_per_sample]`` int64 (``out`` to write into).
        Waits for the last chunk before it returns."""
        import torch
        from . import plink
        dev = f"cuda:{self.device}"
        with plink.open_bed(prefix) as bed:
            if max(submatrix.i_end, submatrix.j_end) > bed.num_samples:
                raise ValueError(f"{submatrix!r} reaches past the {bed.num_samples} samples of "
                                 f"{bed.path}")
            wps = words_per_sample(bed.num_sites)
            stored = submatrix.NumSamples()
            if out is None:
                out = torch.empty((max(stored, 1), wps), dtype=torch.int64, device=dev)
            self._check_bits(submatrix, wps, out)
            if stored == 0 or bed.num_sites == 0:
                return out
            sites = max(64, int(chunk_bytes) // bed.row_bytes // 64 * 64)
            sites = min(sites, (bed.num_sites + 63) // 64 * 64)
            host = [torch.empty(sites * bed.row_bytes, dtype=torch.uint8).pin_memory()
                    for _ in range(2)]
            rows = [torch.empty(sites * bed.row_bytes, dtype=torch.uint8, device=dev)
                    for _ in range(2)]
            copy_stream, pack_stream = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
            copied = [torch.cuda.Event() for _ in range(2)]
            packed = [torch.cuda.Event() for _ in range(2)]
            pack_stream.wait_stream(torch.cuda.current_stream(self.device))
            for k, begin in enumerate(range(0, bed.num_sites, sites)):
                end, b = min(begin + sites, bed.num_sites), k & 1
                nbytes = (end - begin) * bed.row_bytes
                if k >= 2:
                    copied[b].synchronize()         # the staging tensor is free again
                    copy_stream.wait_event(packed[b])   # and so is its device copy
                bed.read_rows(begin, end, host[b].numpy())
                with torch.cuda.stream(copy_stream):
                    rows[b][:nbytes].copy_(host[b][:nbytes], non_blocking=True)
                copied[b].record(copy_stream)
                pack_stream.wait_event(copied[b])
                self.pack_bed(submatrix, wps, rows[b][:nbytes], bed.row_bytes, begin, end,
                              bed.num_sites, out, stream=pack_stream)
                packed[b].record(pack_stream)
            pack_stream.synchronize()
        return out

    # -- site QC --------------------------------------------------------------
    def _rows_of(self, bit_sets, words_per_sample: int) -> int:
        import torch
        _device_tensor(self.device, bit_sets, "bit_sets", torch.int64)
        if words_per_sample <= 0 or words_per_sample % 2 or bit_sets.numel() % words_per_sample:
            raise ValueError(f"bit_sets holds {bit_sets.numel()} words: not rows of "
                             f"{words_per_sample} (a positive even number)")
        return bit_sets.numel() // words_per_sample

    def _counts_out(self, out, shape, zero: bool):
        import torch
        if out is None:
            make = torch.zeros if zero else torch.empty
            return make(shape, dtype=torch.int32, device=f"cuda:{self.device}")
        return _device_tensor(self.device, out, "out", torch.int32, shape=shape)

    def site_counts(self, bit_sets, words_per_sample: int, out=None, stream=None):
        """Genotype counts per site (cuking_site_counts): for every plane site ``0 .. 64 P -
        1`` the number of the rows of ``bit_sets`` (any row range of a bitset: ``[rows,
        words_per_sample]``) that are hom-ref, het, hom-var and missing, as a device tensor
        ``[64 P, 4]`` int32 (a view of uint32 data).  The call ACCUMULATES into ``out``, so
        row ranges, blocks and GPUs merge by passing the tensor back in (or by sum); without
        it a zeroed one is allocated.  Padding sites count as missing.  Does not
        synchronise."""
        rows = self._rows_of(bit_sets, words_per_sample)
        out = self._counts_out(out, (words_per_sample // 2 * 64, 4), zero=True)
        check(self.lib.cuking_site_counts(self.handle, bit_sets.data_ptr(), rows,
                                          words_per_sample, out.data_ptr(),
                                          _stream_handle(stream)))
        return out

    def sample_counts(self, bit_sets, words_per_sample: int, num_sites: int, out=None,
                      stream=None):
        """Genotype counts per sample (cuking_sample_counts): (hom_ref, het, hom_var,
        missing) of every row of ``bit_sets`` over the sites ``[0, num_sites)`` -- padding is
        not counted -- as a device tensor ``[rows, 4]`` int32, OVERWRITTEN.  Call rate and
        heterozygosity follow: the usual ``priority`` of ``unrelated_set``.  Does not
        synchronise."""
        rows = self._rows_of(bit_sets, words_per_sample)
        out = self._counts_out(out, (rows, 4), zero=False)
        check(self.lib.cuking_sample_counts(self.handle, bit_sets.data_ptr(), rows,
                                            words_per_sample, _count(num_sites, "num_sites"),
                                            out.data_ptr(), _stream_handle(stream)))
        return out

    def compact_sites(self, bit_sets, words_per_sample: int, keep_words, num_sites: int,
                      out=None, stream=None):
        """The bitset restricted to the sites of a mask (cuking_compact_sites): the k-th
        kept site of every row becomes site k of the result, what follows the last one is
        missing -- byte for byte the bitset packed from the genotypes of the kept sites.
        ``keep_words``: host uint64 ``[P]`` (``site_mask_host``, ``site_mask_words``); ANY
        mask, not only the rule's.  Returns ``(new_bits, new_words_per_sample, num_kept)``;
        ``out``: an int64 tensor of ``rows x words_per_sample(num_kept)`` words to write
        into, not overlapping ``bit_sets``.  A mask that keeps no site raises ``CukingError``
        ("no site passes").  Waits for the upload of the mask's table on ``stream``; the
        kernel is asynchronous."""
        import torch
        rows = self._rows_of(bit_sets, words_per_sample)
        keep = _keep_words(keep_words, words_per_sample)
        kept = _popcount(keep)
        wps_out = self.lib.cuking_words_per_sample(max(kept, 1))
        if out is None:
            out = torch.empty((max(rows, 1), wps_out), dtype=torch.int64,
                              device=f"cuda:{self.device}")
        elif self._rows_of(out, wps_out) < rows:
            raise ValueError(f"out holds {out.numel()} words, {rows} rows of {wps_out} are "
                             "needed")
        check(self.lib.cuking_compact_sites(
            self.handle, bit_sets.data_ptr(), rows, words_per_sample, keep.ctypes.data,
            _count(num_sites, "num_sites"), out.data_ptr(), wps_out, _stream_handle(stream)))
        return out, wps_out, kept

    def hwe_sites(self, counts, num_sites: int, midp: bool = False, out=None, stream=None):
        """The Hardy-Weinberg exact test per site (cuking_hwe_sites): from the device counts
        tensor of ``site_counts`` (int32 ``[*, 4]``, at least ``num_sites`` rows; missing is
        ignored) the p-values of the first ``num_sites`` sites as a float64 device tensor
        ``[num_sites]``, OVERWRITTEN -- byte for byte what ``hwe_sites_host`` returns.  ``midp``:
        the mid-p form.  ``out``: a float64 ``[num_sites]`` tensor to write into.  Does not
        synchronise."""
        import torch
        num_sites = _count(num_sites, "num_sites")
        _device_tensor(self.device, counts, "counts", torch.int32, cols=4,
                       min_numel=4 * num_sites)
        if out is None:
            out = torch.empty((num_sites,), dtype=torch.float64, device=f"cuda:{self.device}")
        else:
            _device_tensor(self.device, out, "out", torch.float64, shape=(num_sites,))
        check(self.lib.cuking_hwe_sites(self.handle, counts.data_ptr(), num_sites,
                                        HWE_MIDP if midp else 0, out.data_ptr(),
                                        _stream_handle(stream)))
        return out

    def filter_sites(self, bit_sets, words_per_sample: int, num_sites: int,
                     min_call_rate: float = 0.0, min_maf: float = 0.0, min_mac: int = 0,
                     also=None, stream=None, min_hwe_p: float = 0.0, hwe_midp: bool = False,
                     hwe_counts=None) -> "SiteQC":
        """Count, mask and compact in one call: ``site_counts`` of the rows of
        ``bit_sets``, ``site_mask_host`` with the rule given, ``compact_sites`` with its
        mask.  Returns a ``SiteQC`` whose ``bits`` / ``words_per_sample`` / ``num_sites``
        everything behind (records, matrix, summary, relative counts) takes in place of the
        unfiltered ones.  Waits for the counts.

        ``min_hwe_p`` > 0 adds the Hardy-Weinberg rule: ``hwe_sites`` (``hwe_midp``: its mid-p
        form) runs on the call's own counts -- or on ``hwe_counts``, a ``[64 P, 4]`` counts
        tensor of the rows the test should see, e.g. ``site_counts(bits[unrelated])`` for
        PLINK's "founders only" -- and a site is additionally kept iff ``p >= min_hwe_p``
        (false for NaN), ANDed into ``also``; ``SiteQC.hwe_p()`` has the p-values."""
        import torch
        min_hwe_p = _min_hwe_p(min_hwe_p)
        if hwe_counts is not None and not min_hwe_p > 0.0:
            raise ValueError("hwe_counts is read by the Hardy-Weinberg rule only: min_hwe_p must "
                             "be above 0")
        if hwe_counts is not None:
            _device_tensor(self.device, hwe_counts, "hwe_counts", torch.int32,
                           shape=(max(words_per_sample, 0) // 2 * 64, 4))
        counts = self.site_counts(bit_sets, words_per_sample, stream=stream)
        hwe_p = None
        if min_hwe_p > 0.0:
            hwe_p = self.hwe_sites(counts if hwe_counts is None else hwe_counts,
                                   _count(num_sites, "num_sites"), hwe_midp, stream=stream)
        (stream if stream is not None else torch.cuda.current_stream(self.device)).synchronize()
        host = counts.cpu().numpy().view(np.uint32)
        if hwe_p is not None:
            hwe_p = hwe_p.cpu().numpy()
            also = hwe_site_mask(hwe_p, min_hwe_p, also)
        keep, kept = site_mask_host(host, num_sites, min_call_rate, min_maf, min_mac, also)
        bits, wps, _ = self.compact_sites(bit_sets, words_per_sample, keep, num_sites,
                                          stream=stream)
        return SiteQC(host, keep, num_sites, bits, wps, kept, hwe_p)

    # -- LD pruning -------------------------------------------------------------
    def transpose_sites(self, bit_sets, words_per_sample: int, num_sites: int, out=None,
                        stream=None):
        """The site-major bitset (cuking_transpose_sites): the rows of ``bit_sets`` as an
        int64 device tensor ``[num_sites, 2, Q]`` -- per site its het and its hom_var plane
        over the samples, sample s = bit ``s % 64`` of word ``s // 64``, the tail of the last
        word missing.  Plain stores into every word of ``out``; does not synchronise."""
        import torch
        rows = self._rows_of(bit_sets, words_per_sample)
        num_sites = _count(num_sites, "num_sites")
        q = self.lib.cuking_ld_site_words(rows)
        if out is None:
            out = torch.empty((num_sites, 2, q), dtype=torch.int64, device=f"cuda:{self.device}")
        else:
            _device_tensor(self.device, out, "out", torch.int64, min_numel=num_sites * 2 * q)
        check(self.lib.cuking_transpose_sites(
            self.handle, bit_sets.data_ptr(), rows, words_per_sample, num_sites, out.data_ptr(),
            q, _stream_handle(stream)))
        return out

    def ld_edges(self, site_bits, num_sites: int, num_stored: int, window: int = 50,
                 r2: float = 0.2, group=None, max_records=None, out=None, stream=None):
        """The LD edges of a site-major bitset (cuking_ld_edges): the pairs ``a < b`` with ``b
        - a < window``, of one ``group`` (an int32 device tensor of ``num_sites``, e.g.
        chromosomes; None = one group), whose r^2 is above ``r2``, as records ``sample_i = a,
        sample_j = b, kin = r^2, ibs0 = jointly called samples`` in no particular order.
        Returns ``(records, count)``: the ``[*, 6]`` int32 device tensor
        ``unrelated_set`` takes and the number of edges.  Without ``max_records`` the buffer
        holds ``min(num_sites x (window - 1), 4 x num_sites)`` records and the call is repeated
        once with the exact count if that overflows; with it (or with ``out``, a tensor to
        write into), an overflow raises ``ResourceExhaustedError`` whose ``num_records`` is
        the exact count -- nothing is written past the buffer.  WAITS for the stream."""
        from ._place import DevicePlace
        return _ld_edges(DevicePlace(self, stream), site_bits, num_sites, num_stored, window, r2,
                         group, max_records, out)

    def ld_prune(self, bit_sets, words_per_sample: int, num_sites: int, window: int = 50,
                 r2: float = 0.2, group=None, priority=None, compact: bool = True) -> "LDPrune":
        """LD pruning of a bitset where it lies: ``transpose_sites``; ``site_counts`` and from
        them the default ``priority`` (minor allele frequency; or a float32 vector of
        ``num_sites``, host or device: the higher is kept first, among equals the lower site);
        ``ld_edges`` within ``window`` variants and ``group`` above ``r2``; ``unrelated_set``
        on the edges -- the kept sites are the lexicographically first maximal independent
        set in descending priority: no two kept sites of a group within the window have r^2
        above ``r2``, every dropped site has a kept neighbour --; ``site_mask_words`` and,
        with ``compact``, ``compact_sites``.  Returns an ``LDPrune`` whose ``bits`` /
        ``words_per_sample`` / ``num_sites`` everything behind takes in place of the input's
        (the input itself when every site is kept, or without ``compact``).  Waits for the
        device."""
        import torch
        rows = self._rows_of(bit_sets, words_per_sample)
        num_sites = _count(num_sites, "num_sites")
        dev = f"cuda:{self.device}"
        site_bits = self.transpose_sites(bit_sets, words_per_sample, num_sites)
        if priority is None:
            counts = self.site_counts(bit_sets, words_per_sample).cpu().numpy().view(np.uint32)
            priority = ld_priority_host(counts, num_sites)
        if not isinstance(priority, torch.Tensor):
            priority = torch.from_numpy(np.ascontiguousarray(priority, dtype=np.float32)).to(dev)
        records, count = self.ld_edges(site_bits, num_sites, rows, window, r2, group=group)
        del site_bits
        chosen = self.unrelated_set(records, count, num_sites, priority=priority, families=False)
        keep = chosen.keep.cpu().numpy() == 1
        keep_words = site_mask_words(keep)
        kept = int(keep.sum())
        bits, wps, sites = bit_sets, words_per_sample, num_sites
        if compact and kept != num_sites:
            bits, wps, sites = self.compact_sites(bit_sets, words_per_sample, keep_words, num_sites)
            torch.cuda.synchronize(self.device)
        return LDPrune(keep_words, num_sites, bits, wps, sites, records, count, chosen.rounds)

    # -- genotype matrix products, PCA ------------------------------------------
    def geno_matmul(self, bits, words_per_row: int, num_cols: int, table, rhs,
                    per_row: bool = False, out=None, stream=None):
        """The 2-bit genotype matrix times a dense float32 matrix (cuking_geno_matmul), the
        genotypes never expanded: ``out[r, c] = sum_k table[r or k, code(r, k)] * rhs[k, c]``
        over the columns ``k < num_cols`` of ``bits`` (``[rows, words_per_row]``: a row is its
        het words, then its hom_var words; code 0 hom-ref, 1 het, 2 hom-var, 3 missing).  The
        sample-major bitset with a per-column ``table`` (float32 ``[num_cols, 4]``) gives ``Z
        B``; ``transpose_sites`` of it, as ``[num_sites, 2 Q]`` with ``num_cols`` = the samples
        and ``per_row`` (``table`` ``[rows, 4]``), gives ``Z^T A``.  ``rhs``: float32
        ``[num_cols, num_rhs <= 64]``; ``out``: float32 ``[rows, num_rhs]``, overwritten (both
        may be column slices of wider tensors).  Exact for integer tables and ``rhs`` while the
        sums stay below 2^24; the same bits on every call.  Does not synchronise."""
        from ._place import DevicePlace
        return _geno_matmul(DevicePlace(self, stream), bits, words_per_row, num_cols, table, rhs,
                            per_row, out)

    def pca(self, bits, words_per_sample: int, num_sites: int, k: int = 10, fit=None,
            oversample: int = 10, iterations: int = 10, seed: int = 0):
        """Principal components of the standardized genotype matrix (cuking_amd/pca.py has the
        definition): fitted on the rows of ``bits`` that the boolean mask ``fit`` (host or
        device, one entry per row, e.g. ``UnrelatedSet.keep``; None = all) selects, every row
        projected.  ``site_counts`` of the fit rows, ``hwe_table``, ``transpose_sites``, then
        randomized subspace iteration whose only contact with the genotypes is
        ``geno_matmul``.  Returns a ``PCAResult`` of host arrays.  Waits for the device."""
        from . import pca as _pca
        return _pca.pca_device(self, bits, words_per_sample, num_sites, k=k, fit=fit,
                               oversample=oversample, iterations=iterations, seed=seed)

    def pcrelate_matrix(self, bits, words_per_sample: int, num_sites: int, x, beta, lo: float,
                        hi: float, block=None, out=None, stream=None):
        """The bare PC-Relate kernel call (cuking_pcrelate_matrix; include/cuking_amd.h
        "PC-Relate" has the definition): the float32 kinship ``num / (4 den)`` of every pair of
        ``block`` (a ``Submatrix`` or ``(i_begin, i_end, j_begin, j_end)`` over the rows of
        ``bits``; None = all) as a ``[rows, cols]`` device tensor, from ``x`` float32
        ``[num_stored, d <= 32]`` (column 0 the intercept), ``beta`` float32 ``[>= num_sites,
        d]`` and the bounds ``lo < mu < hi``.  ``out``: a float32 tensor of that shape to write
        into, possibly a view with a row pitch of its own.  The same bytes on every call and
        stream; ``[i, j]`` and ``[j, i]`` are the same bytes.  Does not synchronise."""
        from . import pcrelate as _pcr
        return _pcr.pcrelate_matrix_device(self, bits, words_per_sample, num_sites, x, beta,
                                           float(lo), float(hi), block, out, stream)

    def pcrelate(self, bits, words_per_sample: int, num_sites: int, scores, fit=None,
                 min_maf: float = 0.01, block=None, out=None, stream=None):
        """PC-Relate (cuking_amd/pcrelate.py has the definition): the ancestry-adjusted kinship
        of every pair of ``block`` (None = the whole cohort).  ``scores``: float32
        ``[num_stored, k]`` on host or device, e.g. ``PCAResult.scores[:, :k]``; ``fit``: the
        boolean mask of the rows the allele-frequency model is fitted on (None = all), e.g.
        ``PCAResult.fit``.  ``site_counts`` and ``transpose_sites`` of the fit rows, one
        ``geno_matmul`` for the per-site regression on ``[1, scores]``, a ``d x d`` solve in
        float64, then ``pcrelate_matrix`` with the bounds ``min_maf < mu < 1 - min_maf``.
        Returns a ``PCRelateResult`` whose ``kin`` is a device tensor; the fit waits for the
        device, the matrix call does not."""
        from . import pcrelate as _pcr
        return _pcr.pcrelate_device(self, bits, words_per_sample, num_sites, scores, fit=fit,
                                    min_maf=min_maf, block=block, out=out, stream=stream)

    def pcrelate_records_raw(self, bits, words_per_sample: int, num_sites: int, x, beta,
                             lo: float, hi: float, min_kin: float, block=None, max_records=None,
                             out=None, stream=None):
        """The bare kernel call for the pairs above a threshold (cuking_pcrelate_records;
        include/cuking_amd.h "PC-Relate records" has the definition): the pairs of ``block``
        (as ``pcrelate_matrix`` takes it; of a diagonal block those with ``i < j``) whose
        kinship is above ``min_kin`` in the strict float32 comparison, as records ``sample_i <
        sample_j, kin, ibs0 = ibs1 = ibs2 = 0`` in no particular order, ``kin`` the bytes
        ``pcrelate_matrix`` writes for the pair.  Returns ``(records, count)``: the ``[*, 6]``
        int32 device tensor ``unrelated_set`` and ``pcrelate_pairs`` take and the number of
        records.  Only the upper triangle of a diagonal block's tiles is launched; no matrix
        exists.  Without ``max_records`` the buffer holds 16 records per sample of the block
        and the call is repeated once with the exact count if that overflows; with it (or with
        ``out``, a tensor to write into), an overflow raises ``ResourceExhaustedError`` whose
        ``num_records`` is the exact count -- nothing is written past the buffer;
        ``max_records=0`` only counts.  WAITS for the stream."""
        from . import pcrelate as _pcr
        return _pcr.pcrelate_records_raw_device(self, bits, words_per_sample, num_sites, x, beta,
                                                float(lo), float(hi), min_kin, block,
                                                max_records, out, stream)

    def pcrelate_records(self, bits, words_per_sample: int, num_sites: int, scores=None,
                         model=None, fit=None, min_maf: float = 0.01,
                         min_kinship: float = KING_CUTOFFS[0], block=None, max_records=None):
        """PC-Relate for all pairs above a kinship threshold, without a matrix: the
        counterpart of ``compute_king`` whose list holds the cross-ancestry relatives a KING
        threshold misses.  ``model``: an earlier ``PCRelateResult``, ``PCRelateRecords`` or
        ``PCRelatePairs`` whose ``x`` and ``beta`` are reused; otherwise the model is fitted on
        ``scores`` and ``fit`` as ``pcrelate`` does.  ``min_kinship`` defaults to the third-degree
        cut-off ``KING_CUTOFFS[0]``, a convention.  Returns a ``PCRelateRecords`` whose
        ``records`` / ``num_records`` go to ``pcrelate_pairs`` (with ``model=`` the result) and
        ``unrelated_set`` as they stand.  Waits for the device."""
        from . import pcrelate as _pcr
        return _pcr.pcrelate_records_device(self, bits, words_per_sample, num_sites,
                                            scores=scores, model=model, fit=fit, min_maf=min_maf,
                                            min_kinship=min_kinship, block=block,
                                            max_records=max_records)

    def pcrelate_pairs_raw(self, bits, words_per_sample: int, num_sites: int, x, beta, lo: float,
                           hi: float, pairs, f=None, num_records=None, out=None, stream=None):
        """The bare kernel call for listed pairs (cuking_pcrelate_pairs; include/cuking_amd.h
        "PC-Relate for listed pairs" has the definition): ``kin``, ``k0``, ``k1``, ``k2``,
        ``ibs0`` and ``sites`` of every pair of ``pairs`` -- the int32 ``[*, 6]`` record tensor
        of ``compute_king`` with ``num_records``, an int32 / int64 ``[P, 2]`` tensor, or a host
        array of either form -- from ``x``, ``beta`` and the bounds as ``pcrelate_matrix``
        takes them and ``f``, a float32 device tensor of the stored samples' inbreeding
        coefficients (None = all zero).  Returns an int32 ``[P, 8]`` device tensor, one
        cuking_pcrelate_pair per row in input order (``pcrelate.pairs_to_host`` gives it
        names); ``out``: such a tensor to write into.  A row depends on its own pair only; an
        index outside the stored samples gives a NaN row.  One thread runs all sites of a
        pair: a short list is bound by that latency.  Does not synchronise."""
        from . import pcrelate as _pcr
        return _pcr.pcrelate_pairs_raw_device(self, bits, words_per_sample, num_sites, x, beta,
                                              float(lo), float(hi), pairs, f, num_records, out,
                                              stream)

    def pcrelate_pairs(self, bits, words_per_sample: int, num_sites: int, pairs, scores=None,
                       model=None, fit=None, min_maf: float = 0.01, inbreeding=None,
                       num_records=None, stream=None):
        """PC-Relate on a list of pairs, without a matrix: ancestry-adjusted kinship and the
        IBD-sharing coefficients k0, k1, k2 of ``pairs`` (as ``pcrelate_pairs_raw`` takes them;
        ``num_records`` with a record buffer).  ``model``: an earlier ``PCRelateResult`` or
        ``PCRelatePairs`` whose ``x`` and ``beta`` are reused; otherwise the model is fitted on
        ``scores`` and ``fit`` as ``pcrelate`` does.  ``inbreeding``: float32 ``[num_stored]``
        on the host, or None: then the self pairs ``(s, s)`` of all stored samples run first
        and ``f = 2 kin(s, s) - 1`` (a NaN stays NaN and makes that sample's ``k2`` NaN).  A
        pair outside the stored samples raises ValueError.  Returns a ``PCRelatePairs`` of host
        arrays; waits for the device."""
        from . import pcrelate as _pcr
        return _pcr.pcrelate_pairs_device(self, bits, words_per_sample, num_sites, pairs,
                                          scores=scores, model=model, fit=fit, min_maf=min_maf,
                                          inbreeding=inbreeding, num_records=num_records,
                                          stream=stream)

    def ibd_segments_raw(self, bits, words_per_sample: int, num_sites: int, pairs, group=None,
                         pos=None, min_sites: int = 512, min_length: int = 0,
                         segments: bool = False, max_segments=None, num_records=None, out=None,
                         stream=None, bridge_sites: int = 0):
        """The bare kernel call for IBD segments (cuking_ibd_pairs; include/cuking_amd.h "IBD
        segments for listed pairs" has the definition): for every pair of ``pairs`` (as
        ``pcrelate_pairs_raw`` takes them) the number, summed length and longest of the runs of
        at least ``min_sites`` sites and ``min_length`` positions without an opposite
        homozygote (kind 1) and without a difference (kind 2).  ``group``: int32
        ``[num_sites]`` (chromosomes, as ``ld_prune`` takes them) and ``pos``: uint32
        ``[num_sites]`` (non-decreasing inside a group), host arrays or int32 device tensors;
        None = one group, the site index.  Returns ``(rows, segments, num_segments)``: an int32
        ``[P, 10]`` device tensor, one cuking_ibd_pair per row in input order
        (``ibd.rows_to_host`` gives it names; ``out``: such a tensor to write into), and with
        ``segments`` (or a ``max_segments``) an int32 ``[*, 4]`` device tensor whose first
        ``num_segments`` rows are cuking_ibd_segment in no particular order, else None and 0.
        Without ``max_segments`` the buffer is grown once to the exact count; with it an
        overflow raises ``ResourceExhaustedError`` whose ``num_segments`` is the exact count.
        Waits for the stream when ``pos`` is given or segments are counted.
        ``bridge_sites`` (0, or at least 64) links two runs of at least that many sites across
        one break site of a group (cuking_ibd_pairs_bridged, "IBD segments with bridged
        breaks"); the call then returns a fourth value, ``bridged``: an int32 ``[P, 2]`` device
        tensor (``ibd.bridged_to_host``) with the bridged breaks inside the counted segments of
        kind 1 and of kind 2.  0 is the strict call and the strict kernel."""
        from . import ibd as _ibd
        return _ibd.ibd_segments_raw_device(self, bits, words_per_sample, num_sites, pairs, group,
                                            pos, min_sites, min_length, segments, max_segments,
                                            num_records, out, stream, bridge_sites)

    def ibd_segments(self, bits, words_per_sample: int, num_sites: int, pairs, group=None,
                     pos=None, min_sites: int = 512, min_length: int = 0, segments: bool = False,
                     max_segments=None, num_records=None, stream=None, bridge_sites: int = 0):
        """IBD segments of a list of pairs -- typically the records of ``compute_king`` with
        ``num_records`` -- as an ``IBDPairs`` of host arrays (arguments as ``ibd_segments_raw``
        takes them): its ``proportions()`` are the IBD1 / IBD2 shares of ``genome_length`` and
        a kinship, its ``relationship()`` the degree with the parent-child / full-sibling
        split, with no allele frequency and no principal component involved.  With
        ``bridge_sites = 0`` one wrong homozygote splits a segment; ``bridge_sites`` of 64 or
        more forgives an isolated one between two runs of at least that many sites, and
        ``IBDPairs.bridged`` counts the forgiven.  Waits for the device."""
        from . import ibd as _ibd
        return _ibd.ibd_segments_device(self, bits, words_per_sample, num_sites, pairs, group,
                                        pos, min_sites, min_length, segments, max_segments,
                                        num_records, stream, bridge_sites)

    def ibd_scan_raw(self, bits, words_per_sample: int, num_sites: int, group=None, pos=None,
                     min_sites: int = 512, min_length: int = 0, min_total: int = 0, block=None,
                     max_records=None, out=None, stream=None):
        """The bare kernel call for the IBD scan of a block (cuking_ibd_scan; include/cuking_amd.h
        "IBD scan of a block" has the definition): every pair of ``block`` (as
        ``pcrelate_records_raw`` takes it; None = all stored samples) is scanned as
        ``ibd_segments_raw`` scans a listed pair, strictly, and the pairs with a kind-1 segment
        and ``length1 >= min_total`` become records.  Returns ``(records, num_records)``: an
        int32 ``[*, 10]`` device tensor whose first ``num_records`` rows are cuking_ibd_pair
        with ``sample_i < sample_j``, in no particular order (``ibd.records_to_host`` sorts and
        names them; ``out``: such a tensor to write into).  Without ``max_records`` the buffer
        is 16 records per sample of the block, grown once to the exact count; with it an
        overflow raises ``ResourceExhaustedError`` whose ``num_records`` is the exact count,
        and ``max_records=0`` counts.  Waits for the stream once, to read the count, and once
        more when ``pos`` is given."""
        from . import ibd as _ibd
        return _ibd.ibd_scan_raw_device(self, bits, words_per_sample, num_sites, group, pos,
                                        min_sites, min_length, min_total, block, max_records,
                                        out, stream)

    def ibd_scan(self, bits, words_per_sample: int, num_sites: int, group=None, pos=None,
                 min_sites: int = 512, min_length: int = 0, min_total: int = 0, block=None,
                 max_records=None, stream=None):
        """The pairs of a block that share an IBD1 segment, found without a list, as an
        ``IBDPairs`` of host arrays by ``(sample_i, sample_j)`` (arguments as ``ibd_scan_raw``
        takes them): ``proportions()`` and ``relationship()`` work as for ``ibd_segments``, and
        ``pairs()`` is the list to hand to ``ibd_segments`` -- with ``bridge_sites = B``, a
        scan at ``min_sites = B`` misses no pair the bridged call would report -- or to
        ``pcrelate_pairs``.  Waits for the device."""
        from . import ibd as _ibd
        return _ibd.ibd_scan_device(self, bits, words_per_sample, num_sites, group, pos,
                                    min_sites, min_length, min_total, block, max_records, stream)

    def pi_hat_records(self, sm: Submatrix, words_per_sample: int, bits, num_sites: int,
                       min_pi_hat: float = 2 * KING_CUTOFFS[0], counts=None, model=None,
                       bounded: bool = True, max_results=None, stream=None):
        """PI_HAT for every pair of a block (cuking_compute_pihat; include/cuking_amd.h "PI_HAT
        (PLINK --genome)" has the definition): the method-of-moments IBD estimate of PLINK
        ``--genome`` / ``hl.identity_by_descent``, decided on the matrix cores for every pair
        and returned as a ``PiHatRecords`` of the pairs with ``(float32)pi_hat > min_pi_hat``
        (default: the third-degree KING cut-off doubled, a convention).  ``counts``: the
        ``site_counts`` tensor or array of the rows the allele frequencies come from (founders,
        an unrelated set); by default the block's own stored samples.  ``model``: an earlier
        call's or ``pi_hat_model_host``'s instead -- the blocks of a split cohort must share
        one.  ``bounded=False`` skips the bounding of z0, z1, z2.  Without ``max_results`` the
        buffer is 16 records per sample of the block, grown once to the exact count; with it an
        overflow raises ``ResourceExhaustedError`` whose ``num_records`` is the exact count, and
        ``max_results=0`` counts.  Contexts of the tiled kernel with variant 5, 6 or 7 only.
        PI_HAT assumes one homogeneous population.  Waits for the device."""
        from . import pihat as _pihat
        return _pihat.pi_hat_records_device(self, sm, words_per_sample, bits, num_sites,
                                            min_pi_hat, counts, model, bounded, max_results,
                                            stream)

    def roh_segments_raw(self, bits, words_per_sample: int, num_sites: int, samples=None,
                         group=None, pos=None, min_sites: int = 512, min_length: int = 0,
                         bridge_sites: int = 0, segments: bool = False, max_segments=None,
                         out=None, stream=None):
        """The bare kernel call for runs of homozygosity (cuking_roh_samples;
        include/cuking_amd.h "Runs of homozygosity" has the definition): for every sample of
        ``samples`` (an integer ``[S]`` host array or int32 device tensor, repeats and any order
        allowed; None: every row of ``bits``) the number, summed length and longest of the runs
        of at least ``min_sites`` sites and ``min_length`` positions without a heterozygous
        call.  ``group``, ``pos``, ``bridge_sites`` (which here forgives one isolated het),
        ``segments``, ``max_segments`` and the waits are those of ``ibd_segments_raw``.  Returns
        ``(rows, segments, num_segments)``: an int32 ``[S, 6]`` device tensor, one
        cuking_roh_sample per row in list order (``roh.rows_to_host`` gives it names; ``out``:
        such a tensor to write into), and with ``segments`` an int32 ``[*, 4]`` device tensor
        whose first ``num_segments`` rows are cuking_ibd_segment (``pair`` = the row index,
        ``kind`` 0) in no particular order, else None and 0.  The buffer defaults to four
        segments per sample and is grown once to the exact count."""
        from . import roh as _roh
        return _roh.roh_segments_raw_device(self, bits, words_per_sample, num_sites, samples,
                                            group, pos, min_sites, min_length, bridge_sites,
                                            segments, max_segments, out, stream)

    def roh_segments(self, bits, words_per_sample: int, num_sites: int, samples=None,
                     group=None, pos=None, min_sites: int = 512, min_length: int = 0,
                     bridge_sites: int = 0, segments: bool = False, max_segments=None,
                     stream=None):
        """Runs of homozygosity of the listed samples as a ``ROHSamples`` of host arrays
        (arguments as ``roh_segments_raw`` takes them): its ``froh()`` is the share of
        ``genome_length`` inside the runs -- the inbreeding estimate with no allele frequency
        and no principal component involved --, its ``segment_list`` says where they lie.
        ``bridge_sites`` of 64 or more forgives an isolated het between two runs of at least
        that many sites, and ``ROHSamples.bridged`` counts the forgiven.  Waits for the
        device."""
        from . import roh as _roh
        return _roh.roh_segments_device(self, bits, words_per_sample, num_sites, samples, group,
                                        pos, min_sites, min_length, bridge_sites, segments,
                                        max_segments, stream)

    def mendel_errors_raw(self, bits, words_per_sample: int, num_sites: int, trios,
                          error_bits=None, out=None, stream=None):
        """The bare kernel call for Mendelian errors (cuking_mendel_trios; include/cuking_amd.h
        "Mendelian errors" has the definition and the table of the eight codes): for every
        ``(child, father, mother)`` of ``trios`` (an integer ``[T, 3]`` host array or int32
        device tensor; ``mendel.NO_PARENT`` for an absent parent; repeats, any order and shared
        parents allowed) the sites with each error code and the called sites.  Returns ``(rows,
        error_bits)``: an int32 ``[T, 12]`` device tensor, one cuking_mendel_trio per row in
        list order (``mendel.rows_to_host`` gives it names; ``out``: such a tensor to write
        into), and -- with ``error_bits`` True or an int64 ``[T, words_per_sample / 2]`` device
        tensor -- the error mask of every trio, which ``mendel.site_counts_device`` sums per
        site; else None.  Does not synchronise."""
        from . import mendel as _mendel
        return _mendel.mendel_errors_raw_device(self, bits, words_per_sample, num_sites, trios,
                                                error_bits, out, stream)

    def mendel_errors(self, bits, words_per_sample: int, num_sites: int, trios,
                      site_counts: bool = False, stream=None, _chunk_trios=None):
        """Mendelian errors of the listed trios and duos as a ``MendelErrors`` of host arrays
        (arguments as ``mendel_errors_raw`` takes them): ``errors`` ``[T, 8]`` by PLINK's and
        Hail's codes, ``called``, ``total()``, ``rate()`` and ``per_sample()``; with
        ``site_counts`` also ``site_errors``, the number of listed trios with an error at each
        site.  The error mask behind the site counts goes through one buffer of at most 64 MB
        in chunks of trios, which does not change the result.  Waits for the device."""
        from . import mendel as _mendel
        return _mendel.mendel_errors_device(self, bits, words_per_sample, num_sites, trios,
                                            site_counts, stream, _chunk_trios)

    def synth_bitset(self, seed: int, kind, pa, pb, sample_begin: int,
                     sample_end: int, num_sites: int, out=None, stream=None, model=0):
        """Synthetic reference-layout bitset rows [sample_begin, sample_end)
        (bit-identical to oracle/synth_oracle.c).  ``model``: a cohort model of
        the generator by number or name (``synth_models()``); 0 = "baseline"."""
        import torch
        model = synth_model_number(model)
        wps = words_per_sample(num_sites)
        if out is None:
            out = self._tensor((sample_end - sample_begin, wps), torch.int64)
        assert out.numel() >= (sample_end - sample_begin) * wps
        check(self.lib.cuking_synth_bitset_model(
            self.handle, model, seed, kind.data_ptr(), pa.data_ptr(), pb.data_ptr(),
            sample_begin, sample_end, num_sites, wps, out.data_ptr(),
            _stream_handle(stream)))
        return out

    # -- measurement ----------------------------------------------------------
    def timing_enable(self, enabled: bool = True) -> None:
        check(self.lib.cuking_timing_enable(self.handle, int(enabled)))

    def timing_reset(self) -> None:
        check(self.lib.cuking_timing_reset(self.handle))

    def timing_collect(self) -> KernelTiming:
        a, b = C.c_double(), C.c_double()
        na, nb = C.c_uint64(), C.c_uint64()
        check(self.lib.cuking_timing_collect(
            self.handle, C.byref(a), C.byref(na), C.byref(b), C.byref(nb)))
        return KernelTiming(a.value, na.value, b.value, nb.value)

    def clock_probe(self, microseconds: int, stream):
        """Starts the sustained-clock probe on ``stream`` (a side stream);
        returns a function that waits for it and gives the clock in MHz."""
        import torch
        ticks = torch.zeros(2, dtype=torch.int64, device=f"cuda:{self.device}")
        stream.wait_stream(torch.cuda.current_stream())
        check(self.lib.cuking_clock_probe(self.handle, int(microseconds), ticks.data_ptr(),
                                          _stream_handle(stream)))

        def result() -> float:
            stream.synchronize()
            shader, real = ticks.tolist()
            return 100.0 * shader / real if real else 0.0
        return result

    # -- helpers --------------------------------------------------------------
    def _check_bits(self, sm: Submatrix, wps: int, bit_sets) -> None:
        import torch
        _device_tensor(self.device, bit_sets, "bit_sets", torch.int64,
                       min_numel=sm.NumSamples() * wps)

    def _block(self, sm: Submatrix, wps: int, bit_sets) -> tuple:
        """The arguments every call on a block starts with."""
        return (self.handle, C.byref(sm.c), wps, bit_sets.data_ptr())


class KinSummary:
    """What ``KingContext.kin_summary`` returns: the device tensors ``hist`` (``bins + 3``
    slots: UNDER, the bins, OVER, NAN) and ``best`` (one key per stored sample of the
    block, rows first, then columns), int64 views of uint64 data, and ``(lo, hi, bins)``.
    The accessors wait for the device."""

    def __init__(self, hist, best, lo: float, hi: float, bins: int, submatrix: Submatrix,
                 device: int):
        self.hist, self.best = hist, best
        self.lo, self.hi, self.bins = lo, hi, bins
        self.submatrix, self.device = submatrix, device

    def _host(self, t) -> np.ndarray:
        import torch
        torch.cuda.synchronize(self.device)
        return t.cpu().numpy().view(np.uint64)

    def counts(self) -> np.ndarray:
        """The ``bins + 3`` slot counts as uint64."""
        return self._host(self.hist)

    def edges(self) -> np.ndarray:
        """The ``bins + 1`` NOMINAL bin edges (float64); a kinship within a float32
        rounding of one may be counted on either side (cuking_kin_bin_slot decides)."""
        return self.lo + (self.hi - self.lo) * np.arange(self.bins + 1) / self.bins

    def keys(self) -> np.ndarray:
        """The nearest-relative keys as uint64 (0 = no partner with a defined kinship)."""
        return self._host(self.best)

    def nearest(self):
        """``(kin float32, partner int64)`` per stored sample: the largest kinship the
        sample has with any partner inside the block and that partner's GLOBAL index (the
        lowest among equals); NaN and -1 where no pair of the sample has a defined kinship."""
        keys = self.keys()
        ordered = (keys >> np.uint64(32)).astype(np.uint32)
        bits = np.where(ordered & np.uint32(0x80000000), ordered ^ np.uint32(0x80000000),
                        ~ordered).astype(np.uint32)
        kin = np.where(keys != 0, bits.view(np.float32), np.float32("nan")).astype(np.float32)
        partner = np.where(keys != 0, (~keys & np.uint64(0xFFFFFFFF)).astype(np.int64),
                           np.int64(-1))
        return kin, partner

    def count_at_least(self, b: int) -> int:
        """Pairs in bin ``b`` (0-based) and above, OVER included, NAN not: the pairs whose
        kinship is at least the nominal edge ``edges()[b]``."""
        if not 0 <= b <= self.bins:
            raise ValueError(f"bin {b} outside [0, {self.bins}]")
        return int(self.counts()[1 + b:self.bins + 2].sum())


class RelativeCounts:
    """What ``KingContext.relative_counts`` returns: the device tensor ``counts``
    (``[NumSamples(), len(thresholds)]`` int32, a view of uint32 data; one row per stored
    sample of the block, rows first, then columns) and the float32 ``thresholds``.  The
    accessors wait for the device."""

    def __init__(self, counts, thresholds, submatrix: Submatrix, device: int):
        self.counts = counts
        self.thresholds = np.asarray(thresholds, dtype=np.float32)
        self.submatrix, self.device = submatrix, device

    def bands(self) -> np.ndarray:
        """Host ``[NumSamples, T]`` uint32: partners of each stored sample in band t
        (``thresholds[t] < kin <= thresholds[t + 1]``; the last band is open above)."""
        import torch
        torch.cuda.synchronize(self.device)
        return self.counts.cpu().numpy().view(np.uint32).reshape(self.counts.shape)

    def at_least(self) -> np.ndarray:
        """Host ``[NumSamples, T]`` uint64: partners of each stored sample with
        ``kin > thresholds[t]`` -- the suffix sums of ``bands()``."""
        b = self.bands().astype(np.uint64)
        return np.cumsum(b[:, ::-1], axis=1, dtype=np.uint64)[:, ::-1]

    def num_records(self, t: int) -> int:
        """The exact number of records ``compute_king(kin_threshold=thresholds[t])`` appends
        for this block: every such pair is counted at both its samples -- on a diagonal
        block half the column sum, on an off-diagonal one the column sum over its rows."""
        if not 0 <= t < self.thresholds.size:
            raise ValueError(f"threshold {t} outside [0, {self.thresholds.size})")
        column = self.at_least()[:, t]
        sm = self.submatrix
        if sm.i_begin == sm.j_begin:
            return int(column.sum()) // 2
        return int(column[:sm.NumRows()].sum())


class SiteQC:
    """What ``KingContext.filter_sites`` returns.  The filtered cohort: ``bits`` (device
    int64 ``[rows, words_per_sample]``), ``words_per_sample`` and ``num_sites`` (the number of
    kept sites).  The input's sites: ``num_sites_in``, ``counts()``, ``keep()``,
    ``kept_index()``, ``allele_freq()``, ``call_rate()`` and ``hwe_p()`` -- host arrays, one
    entry per site of the INPUT."""

    def __init__(self, site_counts: np.ndarray, keep_words: np.ndarray, num_sites_in: int,
                 bits, words_per_sample: int, num_sites: int, hwe_p=None):
        self.site_counts, self.keep_words, self.num_sites_in = site_counts, keep_words, num_sites_in
        self.bits, self.words_per_sample, self.num_sites = bits, words_per_sample, num_sites
        self._hwe_p = hwe_p

    def hwe_p(self):
        """float64 ``[num_sites_in]``: the Hardy-Weinberg exact p-value of every input site, or
        ``None`` when the rule was not asked for (``min_hwe_p`` = 0)."""
        return self._hwe_p

    def counts(self) -> np.ndarray:
        """uint32 ``[num_sites_in, 4]``: samples hom-ref, het, hom-var and missing."""
        return self.site_counts[:self.num_sites_in]

    def keep(self) -> np.ndarray:
        """bool ``[num_sites_in]``: the sites that passed."""
        return site_mask_bool(self.keep_words, self.num_sites_in)

    def kept_index(self) -> np.ndarray:
        """The input sites that passed, ascending: site k of ``bits`` is input site
        ``kept_index()[k]``."""
        return np.flatnonzero(self.keep())

    def allele_freq(self) -> np.ndarray:
        """float64 ``[num_sites_in]``: the frequency of the counted allele among the called
        genotypes, ``(het + 2 hom_var) / (2 called)``; NaN where nothing was called."""
        c = self.counts().astype(np.float64)
        called = c[:, 0] + c[:, 1] + c[:, 2]
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(called > 0, (c[:, 1] + 2 * c[:, 2]) / (2 * called), np.nan)

    def call_rate(self) -> np.ndarray:
        """float64 ``[num_sites_in]``: ``called / (called + missing)``; NaN without samples."""
        c = self.counts().astype(np.float64)
        n = c.sum(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(n > 0, (n - c[:, 3]) / n, np.nan)


class LDPrune:
    """What ``KingContext.ld_prune`` returns.  The pruned cohort: ``bits`` (device int64
    ``[rows, words_per_sample]``), ``words_per_sample`` and ``num_sites`` -- like ``SiteQC``'s,
    the input of everything behind.  About the input's sites: ``num_sites_in``, ``keep()``,
    ``kept_index()``; about the graph: ``num_edges``, ``rounds`` (of the parallel greedy) and
    ``edges()``."""

    def __init__(self, keep_words: np.ndarray, num_sites_in: int, bits, words_per_sample: int,
                 num_sites: int, records, num_edges: int, rounds: int):
        self.keep_words, self.num_sites_in = keep_words, num_sites_in
        self.bits, self.words_per_sample, self.num_sites = bits, words_per_sample, num_sites
        self.records, self.num_edges, self.rounds = records, num_edges, rounds

    def keep(self) -> np.ndarray:
        """bool ``[num_sites_in]``: the sites that stay."""
        return site_mask_bool(self.keep_words, self.num_sites_in)

    def kept_index(self) -> np.ndarray:
        """The input sites that stay, ascending: site k of a compacted ``bits`` is input
        site ``kept_index()[k]``."""
        return np.flatnonzero(self.keep())

    def edges(self) -> np.ndarray:
        """The edge records (``sample_i = a``, ``sample_j = b``, ``kin`` = r^2, ``ibs0`` = the
        jointly called samples) on the host, sorted by (a, b)."""
        host = self.records[:self.num_edges].cpu().numpy().view(np.uint32).reshape(-1)
        return sort_results(host.view(KING_RESULT_DTYPE).copy())


def _count(value, name: str) -> int:
    if isinstance(value, bool) or int(value) != value or int(value) < 0:
        raise ValueError(f"{name} must be a non-negative integer, not {value!r}")
    return int(value)


class UnrelatedSet:
    """What ``KingContext.unrelated_set`` returns: the device tensors ``keep`` (uint8, 1 =
    kept) and ``family`` (int32, a view of uint32 data: the lowest sample index of each
    sample's connected component; None without ``families``), and ``rounds``, the number of
    rounds of the parallel greedy that had a live edge (the call has waited: an int).  The
    accessors copy to the host."""

    def __init__(self, keep, family, rounds: int, prune_threshold: float, device: int):
        self.keep, self.family, self.rounds = keep, family, rounds
        self.prune_threshold, self.device = prune_threshold, device

    def kept(self) -> np.ndarray:
        """Indices of the kept samples, ascending."""
        return np.flatnonzero(self.keep.cpu().numpy() == 1)

    def dropped(self) -> np.ndarray:
        """Indices of the dropped samples, ascending."""
        return np.flatnonzero(self.keep.cpu().numpy() != 1)

    def families(self) -> dict:
        """root -> members (ascending) for every component of at least two samples."""
        if self.family is None:
            raise ValueError("this UnrelatedSet was computed with families=False")
        return family_members(self.family.cpu().numpy().view(np.uint32))


def family_members(family: np.ndarray) -> dict:
    """root -> members (ascending index arrays) of the components of size >= 2 of a
    ``family`` vector."""
    family = np.asarray(family)
    order = np.argsort(family, kind="stable")
    roots, starts, sizes = np.unique(family[order], return_index=True, return_counts=True)
    return {int(r): order[b:b + n] for r, b, n in zip(roots, starts, sizes) if n >= 2}


def unrelated_set(ctx: KingContext, records, num_records: int, num_samples: int,
                  **kwargs) -> UnrelatedSet:
    """``ctx.unrelated_set(...)``: unrelated set and families from device records."""
    return ctx.unrelated_set(records, num_records, num_samples, **kwargs)


def unrelated_key(priority: float, sample: int) -> int:
    """cuking_unrelated_key: the uint64 order key of a sample (host helper)."""
    return int(_lib.load().cuking_unrelated_key(float(np.float32(priority)), int(sample)))


def unrelated_set_host(records, num_samples: int, prune_threshold: float = float("-inf"),
                       priority=None, families: bool = True):
    """cuking_unrelated_set_host: the same contract on host memory, without a GPU.
    ``records``: a numpy array of KING_RESULT_DTYPE records, or ``[*, 6]`` int32 / uint32
    words.  Returns ``(keep uint8, family uint32 or None)``."""
    num_samples = _count(num_samples, "num_samples")
    recs = np.asarray(records)
    if recs.dtype == KING_RESULT_DTYPE:
        recs = recs.reshape(-1)
    elif recs.dtype in (np.dtype(np.int32), np.dtype(np.uint32)) and \
            (recs.ndim == 2 and recs.shape[1] == 6 or recs.size == 0):
        recs = recs.reshape(-1, 6)
    else:
        raise ValueError("records must be KING_RESULT_DTYPE records or [*, 6] int32 / uint32 "
                         f"words, not {recs.dtype} {recs.shape}")
    recs = np.ascontiguousarray(recs)
    thr = float(np.float32(prune_threshold))
    if thr != thr:
        raise ValueError("prune_threshold must not be NaN")
    prio = None
    if priority is not None:
        prio = np.ascontiguousarray(priority, dtype=np.float32)
        if prio.shape != (num_samples,):
            raise ValueError(f"priority must be a vector of {num_samples} entries, not "
                             f"{prio.shape}")
    keep = np.zeros(num_samples, dtype=np.uint8)
    family = np.zeros(num_samples, dtype=np.uint32) if families else None
    check(_lib.load().cuking_unrelated_set_host(
        recs.ctypes.data if recs.shape[0] else None, recs.shape[0], num_samples, thr,
        prio.ctypes.data if prio is not None else None, keep.ctypes.data if num_samples else None,
        family.ctypes.data if families and num_samples else None))
    return keep, family


def kin_matrix(ctx: KingContext, submatrix: Submatrix, words_per_sample: int, bit_sets,
               **kwargs):
    """``ctx.kin_matrix(...)``: the dense float32 kinship matrix of a block."""
    return ctx.kin_matrix(submatrix, words_per_sample, bit_sets, **kwargs)


def kin_summary(ctx: KingContext, submatrix: Submatrix, words_per_sample: int, bit_sets,
                **kwargs) -> KinSummary:
    """``ctx.kin_summary(...)``: all-pairs kinship histogram and nearest relatives."""
    return ctx.kin_summary(submatrix, words_per_sample, bit_sets, **kwargs)


def relative_counts(ctx: KingContext, submatrix: Submatrix, words_per_sample: int, bit_sets,
                    **kwargs) -> RelativeCounts:
    """``ctx.relative_counts(...)``: per-sample partner counts at kinship thresholds."""
    return ctx.relative_counts(submatrix, words_per_sample, bit_sets, **kwargs)


__all__ = [
    "Submatrix", "KingContext", "kin_matrix", "kin_summary", "KinSummary",
    "relative_counts", "RelativeCounts", "KING_CUTOFFS",
    "unrelated_set", "unrelated_set_host", "unrelated_key", "UnrelatedSet", "family_members",
    "KING_RESULT_DTYPE", "KING_COUNTS_DTYPE",
    "ResourceExhaustedError", "CukingError", "padded_sites",
    "words_per_sample", "bytes_per_pair", "new_host_bitset", "pack_host", "pack_bed_host",
    "site_mask_host", "site_mask_words", "site_mask_bool", "compact_sites_host", "SiteQC",
    "ld_site_words", "transpose_sites_host", "ld_edges_host", "ld_priority_host", "LDPrune",
    "geno_matmul_host",
    "sort_results", "device_count", "synth_models", "synth_model_number",
    "DEFAULT_KIN_THRESHOLD",
    "DEFAULT_MAX_RESULTS",
]
