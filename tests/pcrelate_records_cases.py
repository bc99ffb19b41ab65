"""What the host and the GPU tests of the PC-Relate records share (no GPU, no test of its own):
the cases -- those of pcrelate_cases.py, imported as they stand, plus one at d = 7 for the D = 8
instantiation of the kernel --, the pairs of a block, the thresholds of a case and the checks of
a record list.

Thresholds.  Every case has -inf (every pair with a defined kinship is a record) and +inf
(none).  A case with at least 8 pairs of defined kinship also has two GAP thresholds, one near
the median and one near the 95th percentile of the float64 reference's kinship over the block's
pairs: the midpoint of a gap between two neighbouring reference values, chosen so that NO pair
lies within its own matrix tolerance (Reference.tolerance()) of the threshold -- then a float32
backend within tolerance, the host twin, the device and the float64 reference all threshold to
the same set, and no comparison ever has to leave a pair out.  gap_thresholds() asserts that
condition; the gap is the admissible one whose rank is nearest to the target rank, and how far
that is from the target is printed by test_pcrelate_records_host.py.
"""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import pcrelate_cases as pc

CASES = pc.CASES + (pc.Case("130x65 d7", 130, 65, 7, (0, 130, 0, 130), pad=2),)
EXACT_CASES = tuple(c for c in CASES if c.exact)
INF = float("inf")


def is_diagonal(block) -> bool:
    return block[0] == block[2]


def pair_mask(block) -> np.ndarray:
    """bool [rows, cols]: the entries of the block that are pairs (i < j on a diagonal block)."""
    rows, cols = block[1] - block[0], block[3] - block[2]
    if is_diagonal(block):
        return np.triu(np.ones((rows, cols), dtype=bool), 1)
    return np.ones((rows, cols), dtype=bool)


def num_pairs(block) -> int:
    return int(pair_mask(block).sum())


@dataclass(frozen=True)
class Gap:
    threshold: float      # a float32 value
    target_rank: int      # the rank (among the sorted defined kinships) aimed at
    rank: int             # the number of defined kinships below the threshold
    margin: float         # the smallest |kin - threshold| / tolerance over the pairs, > 1


@lru_cache(maxsize=None)
def gap_thresholds(case) -> tuple:
    """The Gaps near the median and the 95th percentile of the case, () for a case with fewer
    than 8 pairs of defined kinship."""
    ref = pc.reference(case)
    mask = pair_mask(case.block) & ~np.isnan(ref.kin)
    kin, tol = ref.kin[mask], ref.tolerance()[mask]
    if kin.size < 8:
        return ()
    order = np.argsort(kin, kind="stable")
    kin, tol = kin[order], tol[order]
    # the forbidden interval of every pair; a threshold is admissible outside all of them
    lo_edge, hi_edge = kin - tol, kin + tol
    reach = np.maximum.accumulate(hi_edge)             # the furthest right edge up to rank k
    floor = np.minimum.accumulate(lo_edge[::-1])[::-1]  # the furthest left edge from rank k on
    gaps = []
    for q in (0.5, 0.95):
        target = int(q * kin.size)
        # admissible cut between ranks k - 1 and k: reach[k - 1] < floor[k], with room for a float32
        ok = np.nonzero(reach[:-1] < floor[1:])[0] + 1
        assert ok.size, f"{case.name}: no admissible threshold"
        for k in ok[np.argsort(np.abs(ok - target), kind="stable")]:
            t = float(np.float32(0.5 * (reach[k - 1] + floor[k])))
            margin = float((np.abs(kin - t) / tol).min())
            if margin > 1.0 and kin[k - 1] < t < kin[k]:
                gaps.append(Gap(t, target, int(k), margin))
                break
        else:
            raise AssertionError(f"{case.name}: no admissible float32 threshold")
    # THE condition: no pair within its tolerance of a threshold
    for g in gaps:
        assert (np.abs(kin - g.threshold) > tol).all(), (case.name, g)
    return tuple(gaps)


def thresholds(case) -> tuple:
    """(-inf, +inf, the gap thresholds) of a case."""
    return (-INF, INF) + tuple(g.threshold for g in gap_thresholds(case))


def threshold_matrix(kin: np.ndarray, block, min_kin: float) -> np.ndarray:
    """The records a kinship matrix of the block gives: KING_RESULT_DTYPE rows in ascending
    (sample_i, sample_j) with the matrix's kinship bytes.  The comparison is the strict float32
    one for a float32 matrix, and false for a NaN."""
    from cuking_amd import KING_RESULT_DTYPE
    threshold = np.float32(min_kin) if kin.dtype == np.float32 else min_kin
    with np.errstate(invalid="ignore"):
        hit = pair_mask(block) & (kin > threshold)
    ii, jj = np.nonzero(hit)          # (row-major: ascending (i, j))
    out = np.zeros(ii.size, dtype=KING_RESULT_DTYPE)
    out["sample_i"], out["sample_j"] = ii + block[0], jj + block[2]
    out["kin"] = kin[ii, jj].astype(np.float32)
    return out


def pair_set(records) -> set:
    return set(zip(records["sample_i"].tolist(), records["sample_j"].tolist()))


def check_records(records, block):
    """What holds for every record list: sample_i < sample_j, inside the block, zero ibs
    fields, no duplicate pair."""
    i, j = records["sample_i"].astype(np.int64), records["sample_j"].astype(np.int64)
    assert (i < j).all()
    assert ((i >= block[0]) & (i < block[1]) & (j >= block[2]) & (j < block[3])).all()
    for name in ("ibs0", "ibs1", "ibs2"):
        assert not records[name].any()
    assert len(pair_set(records)) == records.shape[0]


def check_records_reference(ref, block, records, name, label="", quiet=False):
    """The records of a call at -inf against a pcrelate_cases.Reference of the block: what
    check_reference asks of a matrix, on the block's pairs -- the pairs of the records are the
    pairs whose reference kinship is not NaN (identical NaN positions), and every kinship is
    within the reference's tolerance.  Returns the largest error / tolerance."""
    assert ref.margin_violations() == 0, f"{name}: choose another seed"
    check_records(records, block)
    want = pair_mask(block) & ~np.isnan(ref.kin)
    ii = records["sample_i"].astype(np.int64) - block[0]
    jj = records["sample_j"].astype(np.int64) - block[2]
    have = np.zeros_like(want)
    have[ii, jj] = True
    assert np.array_equal(have, want), np.argwhere(have != want)[:5]
    if not records.shape[0]:
        return 0.0
    ratio = float((np.abs(records["kin"] - ref.kin[ii, jj]) / ref.tolerance()[ii, jj]).max())
    if not quiet:
        print(f"{name} {label}: {records.shape[0]} records, largest error / tolerance {ratio:.3g}")
    assert ratio <= 1.0, (name, label, ratio)
    return ratio


def same_records(got, want):
    """Both sorted by (sample_i, sample_j): the same pairs and the same kinship bytes."""
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got["sample_i"], want["sample_i"])
    assert np.array_equal(got["sample_j"], want["sample_j"])
    assert got["kin"].tobytes() == want["kin"].tobytes()
