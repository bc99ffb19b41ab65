"""IBD scan of a block: what the host and the GPU tests share.  The scan decides nothing of its
own, so its reference is the LISTED call over the explicit list of the block's pairs, filtered by
the record rule (``listed_records``); the cases of ibd_cases.py add the per-site numpy walk of
that file (``check_reference``).  Every comparison is on bytes.

The block cohort: 70 samples -- three tile rows at 32 samples a tile, the last one partial -- with
planted pairs inside a tile, across tiles, on a tile edge and in the partial tile, two groups
and positions.  At 64 sites two groups leave no room for a segment of 64 sites, so that size is
run with one group as well.
"""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import ibd_cases as ic
from cuking_amd.ibd import ibd_scan_raw_host, ibd_segments_raw_host

TILE = 32              # kScanTile of csrc/king_ibd_scan.hip
CHUNK_SITES = 16 * 64  # one LDS chunk: kScanChunk words
FILL = 0x2B2B2B2B      # what the refusal tests pre-fill their outputs with


# ---- the record rule on the rows of the listed call ----------------------------------------------
def block_pairs(block):
    """The pairs of ``(i_begin, i_end, j_begin, j_end)`` in ascending (i, j): uint32 ``[P, 2]``."""
    i0, i1, j0, j1 = block
    diag = (i0, i1) == (j0, j1)
    pairs = [(i, j) for i in range(i0, i1) for j in range(i + 1 if diag else j0, j1)]
    return np.array(pairs, dtype=np.uint32).reshape(-1, 2)


def filtered(rows, min_total=0):
    """The rows that are records: segments1 >= 1 and length1 >= min_total."""
    return rows[(rows["segments1"] >= 1) & (rows["length1"] >= np.uint64(min_total))]


def listed_records(bits, wps, sites, group, pos, min_sites, min_length, block, min_total=0):
    """The records of ``block`` from cuking_ibd_pairs_host over the explicit list of its pairs."""
    rows, _ = ibd_segments_raw_host(bits, wps, sites, block_pairs(block), group, pos, min_sites,
                                    min_length)
    return filtered(rows, min_total)


def by_pair(rows):
    """(i, j) -> the row's bytes from segments1 on."""
    return {(int(r["sample_i"]), int(r["sample_j"])): r.tobytes()[8:] for r in rows}


def check_sorted(records):
    """Host order: ascending (i, j), i < j, no pair twice."""
    keys = [(int(r["sample_i"]), int(r["sample_j"])) for r in records]
    assert keys == sorted(set(keys)) and all(i < j for i, j in keys)


def check_reference(case: ic.Case, records):
    """The scan's records of the whole diagonal block of an ibd_cases case against the per-site
    numpy walk of that file: every listed pair i != j inside the cohort that the walk gives a
    kind-1 segment is a record with the walk's bytes, and no other listed pair is a record."""
    rows, _ = ic.reference(case)
    got = by_pair(records)
    seen = 0
    for r in rows:
        i, j = int(r["sample_i"]), int(r["sample_j"])
        if i == j or i >= case.samples or j >= case.samples:
            continue
        key = (min(i, j), max(i, j))
        if r["segments1"] >= 1:
            assert got.get(key) == r.tobytes()[8:], (case.name, key)
            seen += 1
        else:
            assert key not in got, (case.name, key)
    return seen


def scan_case(case: ic.Case, ones_padding=False, **kw):
    inp = ic.inputs(case)
    return ibd_scan_raw_host(inp.bits(ones_padding), inp.wps, case.sites, inp.group, inp.pos,
                             case.min_sites, case.min_length, **kw)


def listed_case(case: ic.Case, min_total=0):
    inp = ic.inputs(case)
    return listed_records(inp.bits(), inp.wps, case.sites, inp.group, inp.pos, case.min_sites,
                          case.min_length, (0, case.samples, 0, case.samples), min_total)


# ---- the block cohort ----------------------------------------------------------------------------
COHORT_SAMPLES = 70
# (sites, two groups): a whole word closed beyond the plane, one chunk exactly, one chunk and 37
# sites, four chunks and 37 sites (beyond two LDS chunks plus 37)
COHORTS = [(64, False), (64, True), (CHUNK_SITES, True), (CHUNK_SITES + 37, True),
           (4096 + 37, True)]
BLOCKS = {
    "diagonal": (0, 70, 0, 70),
    "sub-block": (5, 41, 5, 41),
    "off-diagonal": (0, 33, 33, 70),
    "one row": (3, 4, 60, 70),
}
# inside a tile, across tiles, on a tile edge, in the partial tile, in every block above
PLANTED = ((0, 1, 2), (3, 65, 1), (10, 40, 2), (31, 32, 1), (6, 34, 2), (33, 69, 1), (64, 69, 2),
           (3, 61, 2), (5, 6, 1), (35, 40, 2), (0, 69, 1))


@dataclass
class Cohort:
    sites: int
    code: np.ndarray
    wps: int
    group: object
    pos: np.ndarray
    min_sites: int
    min_length: int

    def bits(self, ones_padding=False):
        return ic.pack_codes(self.code, self.wps // 2, ones_padding)

    def args(self):
        """(wps, sites, group, pos, min_sites, min_length)."""
        return self.wps, self.sites, self.group, self.pos, self.min_sites, self.min_length


@lru_cache(maxsize=None)
def cohort(sites: int, grouped: bool = True) -> Cohort:
    rng = np.random.default_rng(7000 + sites)
    code = ic.draw_codes(rng, COHORT_SAMPLES, sites)
    whole = sites == 64
    for k, (i, j, kind) in enumerate(PLANTED):
        # (staggered ends; at 64 sites the only possible segment is the whole word)
        first = 0 if whole else (sites // 16) * (k % 4)
        last = sites - 1 if whole else sites - 1 - (sites // 16) * (k % 3)
        ic.plant(code, i, j, first, last, kind)
    group = None
    steps = rng.integers(0, 9, size=sites).astype(np.int64)
    pos = np.cumsum(steps)
    if grouped:
        bound = sites // 2 + 3
        group = (np.arange(sites) >= bound).astype(np.int32) * 5
        pos[bound:] -= pos[bound] - 11   # (a new group may start below its predecessor)
    # (tight planes: at a multiple of 64 the word of bit num_sites lies beyond them)
    return Cohort(sites, code, 2 * -(-sites // 64), group, pos.astype(np.uint32),
                  64 if whole else 100, 0 if whole else 400)


@lru_cache(maxsize=None)
def cohort_records(sites: int, grouped: bool, block_name: str):
    """The listed call's records of one block of a cohort: the reference, computed once."""
    c = cohort(sites, grouped)
    return listed_records(c.bits(), *c.args(), BLOCKS[block_name])


@lru_cache(maxsize=None)
def duplicates():
    """70 copies of one sample: every pair is a record, more than the wrapper's default buffer
    of 16 records per sample of the block."""
    rng = np.random.default_rng(31)
    code = np.repeat(ic.draw_codes(rng, 1, 200), COHORT_SAMPLES, axis=0)
    return Cohort(200, code, 2 * 4, None, None, 64, 0)


# ---- the refusals through the raw ABI ------------------------------------------------------------
# name -> (the arguments replaced (see raw_arguments), status, part of the message)
REFUSALS = {
    "null block": (dict(block=None), "INVALID", "null submatrix"),
    "reversed block": (dict(block=(5, 3, 5, 3)), "INVALID", "reversed"),
    "overlapping block": (dict(block=(0, 5, 3, 8)), "INVALID", "identical or disjoint"),
    "columns first": (dict(block=(4, 8, 0, 4)), "INVALID", "identical or disjoint"),
    "same start, other end": (dict(block=(0, 4, 0, 8)), "INVALID", "identical row and column"),
    "rows outside the stored samples": (dict(block=(0, 9, 0, 9)), "INVALID", "outside the 8"),
    "columns outside the stored samples": (dict(block=(0, 4, 4, 9)), "INVALID", "outside the 8"),
    "words_per_sample zero": (dict(wps=0), "INVALID", "positive even"),
    "words_per_sample odd": (dict(wps=3), "INVALID", "positive even"),
    "sites beyond the planes": (dict(num_sites=64 * 3 + 1), "INVALID", "do not fit"),
    "min_sites below 64": (dict(min_sites=63), "INVALID", "min_sites (63) must be at least 64"),
    "null num_records": (dict(found=None), "INVALID", "null num_records pointer"),
    "null records with room asked": (dict(records=None), "INVALID", "null records pointer"),
    "null bits": (dict(bits=None), "INVALID", "null bits pointer"),
    "pos decreases inside a group": (dict(pos="decreasing"), "PRECONDITION",
                                     "pos must not decrease inside a group, but pos[100] = 5 "
                                     "follows pos[99] = 99"),
}
REFUSAL_CASE = ic.REFUSAL_CASE   # 8 samples, 180 sites, three plane words, one planted pair
# calls without work: 0 records and OK, the buffer untouched
NO_WORK = {
    "empty block": dict(block=(3, 3, 3, 3)),
    "no rows": dict(block=(2, 2, 4, 8)),
    "1 x 1 diagonal block": dict(block=(4, 5, 4, 5)),
    "no sites": dict(num_sites=0),
    "no sites and no bits": dict(num_sites=0, bits=None),
}


def decreasing_pos(sites):
    pos = np.arange(sites, dtype=np.uint32)
    pos[100] = 5
    return pos


def raw_arguments(inp, pointers, **over):
    """The argument list of cuking_ibd_scan_host (the device call adds ctx and stream around it):
    ``pointers`` holds bits, group, pos, block (a ctypes reference or None), records, found."""
    a = dict(pointers, num_stored=inp.case.samples, wps=inp.wps, num_sites=inp.case.sites,
             min_sites=inp.case.min_sites, min_length=inp.case.min_length, min_total=0,
             max_records=16)
    a.update(over)
    return (a["bits"], a["num_stored"], a["wps"], a["num_sites"], a["group"], a["pos"],
            a["min_sites"], a["min_length"], a["block"], a["min_total"], a["records"],
            a["max_records"], a["found"])
