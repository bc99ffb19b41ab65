"""Mendelian errors of trios and duos: the sites at which a child's genotype cannot come from its
parents' -- ``plink --mendel``, ``hl.mendel_errors``, the trio check of KING ``--build`` and of
gnomAD's sample QC -- counted per trio and, on request, per site, on the bitset where it lies.
include/cuking_amd.h "Mendelian errors" holds the definition and the table of the eight codes
(PLINK's and Hail's numbers, autosomal only); every decision is on integers, so the device call,
the host twin and a per-site walk agree byte for byte.

Trios come from a ``.fam`` (``plink.read_fam_parents`` -> ``trios_from_parents``) or from what the
library already reports about pairs (``candidate_trios``); ``mendel_errors`` is what confirms one.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ._lib import check
from ._place import HOST, DevicePlace, tensor_to_host
from .api import _count
from .pcrelate import PARENT_CHILD

NO_PARENT = 0xFFFFFFFF   # CUKING_MENDEL_NO_PARENT
NUM_CODES = 8
# cuking_mendel_trio
MENDEL_TRIO_DTYPE = np.dtype([("child", "<u4"), ("father", "<u4"), ("mother", "<u4"),
                              ("called", "<u4"), ("errors", "<u4", (NUM_CODES,))])
assert MENDEL_TRIO_DTYPE.itemsize == 48
# The wrapper's error mask never takes more than this: the trios go through in chunks.
MASK_BYTES = 64 << 20
# PLINK's .imendel rule: whom an error of code k + 1 implicates, as columns (child, father, mother)
_IMPLICATES = np.array([[1, 1, 1], [1, 1, 1], [1, 1, 0], [1, 0, 1],
                        [1, 1, 1], [1, 1, 0], [1, 0, 1], [1, 1, 1]], dtype=np.int64)


@dataclass
class MendelErrors:
    """What ``KingContext.mendel_errors`` / ``mendel_errors_host`` return, as host arrays:
    ``rows`` (``MENDEL_TRIO_DTYPE`` ``[T]``, one per listed trio in list order) and its fields
    ``child``, ``father``, ``mother`` (uint32, as listed; ``NO_PARENT`` for an absent parent),
    ``called`` (uint32: the sites where the child and every parent that is not ``NO_PARENT`` are
    called) and ``errors`` (uint32 ``[T, 8]``: ``errors[:, k]`` counts code ``k + 1``);
    ``site_errors`` (uint32 ``[num_sites]``: the number of listed trios with an error at each
    site, or None when it was not asked for)."""
    rows: np.ndarray
    site_errors: object = None

    child = property(lambda self: self.rows["child"])
    father = property(lambda self: self.rows["father"])
    mother = property(lambda self: self.rows["mother"])
    called = property(lambda self: self.rows["called"])
    errors = property(lambda self: self.rows["errors"])

    def total(self) -> np.ndarray:
        """Errors per trio: the row sum of ``errors`` (int64)."""
        return self.errors.sum(axis=1, dtype=np.int64)

    def rate(self) -> np.ndarray:
        """``total() / called`` in float64 on the host; NaN where nothing is called."""
        called = self.called.astype(np.float64)
        out = np.full(len(self.rows), np.nan, dtype=np.float64)
        np.divide(self.total().astype(np.float64), called, out=out, where=called > 0)
        return out

    def per_sample(self, num_samples: int) -> np.ndarray:
        """The errors that implicate each of the samples ``0 .. num_samples - 1`` (int64), by
        PLINK's ``.imendel`` rule: codes 1, 2, 5 and 8 count for child, father and mother, 3 and 6
        for child and father, 4 and 7 for child and mother.  A repeated trio counts each time it
        is listed; ``NO_PARENT`` and indices ``>= num_samples`` are left out."""
        num_samples = _count(num_samples, "num_samples")
        out = np.zeros(num_samples, dtype=np.int64)
        share = self.errors.astype(np.int64) @ _IMPLICATES    # [T, 3]
        for column, who in enumerate((self.child, self.father, self.mother)):
            inside = who < num_samples
            np.add.at(out, who[inside].astype(np.int64), share[inside, column])
        return out


def _trio_list(trios) -> np.ndarray:
    """``trios`` as a contiguous uint32 ``[T, 3]`` host array (child, father, mother)."""
    trios = np.asarray(trios)
    if trios.size == 0 and trios.ndim <= 2:   # (an empty list has no shape to speak of)
        return np.zeros((0, 3), dtype=np.uint32)
    if trios.ndim != 2 or trios.shape[1] != 3 or trios.dtype.kind not in "iu":
        raise ValueError(f"trios must be an integer [T, 3] array, not {trios.dtype} "
                         f"{trios.shape}")
    if trios.size and (int(trios.min()) < 0 or int(trios.max()) > 0xFFFFFFFF):
        raise ValueError("trios must fit uint32 (NO_PARENT for an absent parent)")
    return np.ascontiguousarray(trios, dtype=np.uint32).reshape(-1, 3)


def _chunk_rows(plane: int, chunk) -> int:
    """Trios per mask buffer: ``chunk`` if given, else what fits ``MASK_BYTES``."""
    if chunk is not None:
        chunk = _count(chunk, "_chunk_trios")
        if chunk == 0:
            raise ValueError("_chunk_trios must be positive")
        return chunk
    return max(1, MASK_BYTES // (8 * max(plane, 1)))


def trios_from_parents(parents) -> np.ndarray:
    """``[T, 3]`` uint32 (child, father, mother) from the ``int64 [n, 2]`` of
    ``plink.read_fam_parents`` (row index of father and mother, -1 for none): one row per sample
    with at least one parent present, in sample order, ``NO_PARENT`` for -1."""
    parents = np.asarray(parents)
    if parents.ndim != 2 or parents.shape[1] != 2 or (parents.size and
                                                      parents.dtype.kind not in "iu"):
        raise ValueError(f"parents must be an integer [n, 2] array, not {parents.dtype} "
                         f"{parents.shape}")
    parents = parents.astype(np.int64)
    if parents.size and (int(parents.min()) < -1 or int(parents.max()) >= NO_PARENT):
        raise ValueError("parents must be row indices or -1")
    children = np.flatnonzero((parents >= 0).any(axis=1))
    out = np.empty((len(children), 3), dtype=np.uint32)
    out[:, 0] = children
    out[:, 1:] = np.where(parents[children] < 0, NO_PARENT, parents[children])
    return out


def _pair_set(pairs, name: str) -> set:
    pairs = np.asarray(pairs)
    if pairs.size == 0:
        return set()
    if pairs.ndim != 2 or pairs.shape[1] != 2 or pairs.dtype.kind not in "iu":
        raise ValueError(f"{name} must be an integer [P, 2] array, not {pairs.dtype} "
                         f"{pairs.shape}")
    return {(min(int(i), int(j)), max(int(i), int(j))) for i, j in pairs}


def candidate_trios(pairs, relationship, related=None) -> np.ndarray:
    """Trios inferred from pairs, on the host: every ``(c, a, b)`` with ``a < b`` such that the
    pairs ``(c, a)`` and ``(c, b)`` carry the parent-child code of ``relationship()``
    (``PCRelatePairs.relationship()``, ``IBDPairs.relationship()``) and ``(a, b)`` is not among
    ``related`` (an integer ``[R, 2]`` array of every related pair; default: ``pairs``).
    ``pairs`` is an integer ``[P, 2]`` array and ``relationship`` its ``[P]`` codes.

    Two children of one parent are at least half siblings, and a grandparent and a grandchild
    are second-degree relatives: when ``related`` was drawn at a third-degree threshold, a sample
    with two parent-child relatives that are unrelated to each other is their child.  Sex is
    unknown, so ``a`` fills the father column and ``b`` the mother's.  Returns uint32 ``[T, 3]``
    sorted by ``(c, a, b)``: a function of the SET of pairs, not of their order or of repeats.

    A candidate is a hypothesis from pairwise sharing only; ``mendel_errors`` is what confirms
    it: a true trio shows next to no errors, and no codes 1, 2, 5 or 8 beyond genotyping error."""
    pairs = np.asarray(pairs)
    relationship = np.asarray(relationship).reshape(-1)
    everyone = _pair_set(pairs, "pairs")
    if len(relationship) != (len(pairs) if pairs.size else 0):
        raise ValueError(f"{len(relationship)} relationship codes for {len(pairs)} pairs")
    linked = everyone if related is None else _pair_set(related, "related")
    relatives = {}   # sample -> its parent-child relatives
    for (i, j), code in zip(pairs.tolist() if pairs.size else [], relationship.tolist()):
        if code == PARENT_CHILD and i != j:
            relatives.setdefault(int(i), set()).add(int(j))
            relatives.setdefault(int(j), set()).add(int(i))
    found = []
    for c in sorted(relatives):
        others = sorted(relatives[c])
        for x, a in enumerate(others):
            for b in others[x + 1:]:
                if (a, b) not in linked:
                    found.append((c, a, b))
    return np.array(found, dtype=np.uint32).reshape(-1, 3)


# ---- the calls, over a place (the host twin and the device) ---------------------------------------
def _mendel_errors_raw(place, bits, words_per_sample, num_sites, trios, error_bits, out=None):
    words_per_sample = _count(words_per_sample, "words_per_sample")
    num_sites = _count(num_sites, "num_sites")
    num_stored = place.bits(bits, words_per_sample)
    listed = place.index_list(trios, "trios", 3, _trio_list)
    count = listed.shape[0]
    out = place.alloc(count, MENDEL_TRIO_DTYPE) if out is None else \
        place.out(out, "out", MENDEL_TRIO_DTYPE, count)
    if error_bits is True:
        error_bits = place.alloc((count, words_per_sample // 2), np.uint64)
    elif error_bits is not None and error_bits is not False:
        place.out(error_bits, "error_bits", np.uint64, (count, words_per_sample // 2))
    else:
        error_bits = None
    place.uploads_done()
    check(place.fn("mendel_trios")(place.ptr(bits, pad=True), num_stored, words_per_sample,
                                   num_sites, place.ptr(listed), count, place.ptr(out),
                                   place.ptr(error_bits)))
    place.keep()
    return out, error_bits


def _site_counts(place, error_bits, counts):
    place.words(error_bits, "error_bits")
    if error_bits.ndim != 2:
        raise ValueError(f"error_bits must be [T, W], not {tuple(error_bits.shape)}")
    num_trios, plane = error_bits.shape
    fresh = None
    if counts is None:
        counts = fresh = place.zeros(64 * plane, np.uint32)   # (zeroed on the current stream)
    else:
        place.out(counts, "counts", np.uint32, 64 * plane)
    place.uploads_done()
    check(place.fn("mendel_site_counts")(place.ptr(error_bits), num_trios if plane else 0,
                                         max(plane, 1), place.ptr(counts)))
    place.keep(fresh)
    return counts


def _mendel_errors(place, bits, words_per_sample, num_sites, trios, site_counts, chunk):
    listed = place.index_list(_trio_list(place.host_sites(trios, np.uint32)), "trios", 3,
                              _trio_list)
    count = listed.shape[0]
    rows = place.alloc(count, MENDEL_TRIO_DTYPE)
    counts = None
    if not site_counts:
        _mendel_errors_raw(place, bits, words_per_sample, num_sites, listed, None, rows)
    else:
        plane = _count(words_per_sample, "words_per_sample") // 2
        step = min(_chunk_rows(plane, chunk), max(count, 1))
        # ONE mask buffer for every chunk: the calls of a stream run in order
        mask = place.alloc((step, plane), np.uint64)
        counts = place.zeros(64 * plane, np.uint32)
        for lo in range(0, count, step):
            n = min(step, count - lo)
            _mendel_errors_raw(place, bits, words_per_sample, num_sites, listed[lo:lo + n],
                               mask[:n], rows[lo:lo + n])
            _site_counts(place, mask[:n], counts)
        place.keep(mask, counts)
    place.keep(rows)
    place.finish()
    host_rows = place.to_host(rows, MENDEL_TRIO_DTYPE)
    if counts is None:
        return MendelErrors(host_rows)
    return MendelErrors(host_rows, place.to_host(counts, np.uint32)[:num_sites].copy())


def mendel_errors_raw_host(bits: np.ndarray, words_per_sample: int, num_sites: int, trios,
                           error_bits: bool = False):
    """cuking_mendel_trios_host, the bare call: ``(rows, error_bits)`` -- one
    ``MENDEL_TRIO_DTYPE`` row per entry of ``trios`` (an integer ``[T, 3]`` array) and, with
    ``error_bits``, the uint64 ``[T, words_per_sample / 2]`` error mask, else None.  Bit for bit
    what ``KingContext.mendel_errors_raw`` gives."""
    return _mendel_errors_raw(HOST, bits, words_per_sample, num_sites, trios, bool(error_bits))


def site_counts_host(error_bits: np.ndarray, counts=None) -> np.ndarray:
    """cuking_mendel_site_counts_host: ADDS the column sums of the uint64 ``[T, W]`` mask to
    ``counts`` (uint32 ``[64 W]``; default: zeros) and returns it."""
    return _site_counts(HOST, error_bits, counts)


def mendel_errors_host(bits: np.ndarray, words_per_sample: int, num_sites: int, trios,
                       site_counts: bool = False, _chunk_trios=None) -> MendelErrors:
    """``KingContext.mendel_errors`` on host memory and the host twin: no GPU."""
    return _mendel_errors(HOST, bits, words_per_sample, num_sites, trios, site_counts,
                          _chunk_trios)


def rows_to_host(rows) -> np.ndarray:
    """The ``[T, 12]`` int32 device tensor of ``mendel_errors_raw`` as ``MENDEL_TRIO_DTYPE`` rows
    on the host (waits for the copy)."""
    return tensor_to_host(rows, MENDEL_TRIO_DTYPE)


def mendel_errors_raw_device(ctx, bits, words_per_sample: int, num_sites: int, trios,
                             error_bits=None, out=None, stream=None):
    return _mendel_errors_raw(DevicePlace(ctx, stream), bits, words_per_sample, num_sites, trios,
                              error_bits, out)


def site_counts_device(ctx, error_bits, counts=None, stream=None):
    return _site_counts(DevicePlace(ctx, stream), error_bits, counts)


def mendel_errors_device(ctx, bits, words_per_sample: int, num_sites: int, trios,
                         site_counts: bool = False, stream=None, _chunk_trios=None):
    return _mendel_errors(DevicePlace(ctx, stream), bits, words_per_sample, num_sites, trios,
                          site_counts, _chunk_trios)
