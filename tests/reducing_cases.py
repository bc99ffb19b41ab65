"""What the three reducing calls must give -- the dense kinship matrix (kin_matrix), the
histogram and the nearest relatives (kin_summary), the per-sample band counts
(relative_counts) -- restated in numpy from the CPU oracle's kinship of every pair
(oracle.all_pairs), in one place: tests/test_gpu_kin_matrix.py, test_gpu_kin_summary.py,
test_gpu_relative_counts.py and the fuzzer (fuzz_cases.run_reducing) judge the kernels by
these, and tests/test_reducing_cases.py judges these by plain Python loops.

`sm` is a block's (i_begin, i_end, j_begin, j_end); (oi, oj, kin) the global indices and the
float32 kinship of every pair the oracle lists for it.  Stored samples of a block: its rows
first, then its columns (a diagonal block's samples once)."""
from collections import namedtuple

import numpy as np

f32, u32, u64 = np.float32, np.uint32, np.uint64
SENTINEL = np.float32(-7.0)        # what a matrix entry holds that no pair writes


# ---- dense kinship matrix --------------------------------------------------------------------
def assert_same(got, exp, what=""):
    """Bit-equal on the uint32 view; NaN where the expectation is NaN."""
    assert got.shape == exp.shape and got.dtype == np.float32, what
    nan = np.isnan(exp)
    assert np.isnan(got[nan]).all(), f"{what}: a NaN entry of the oracle is not NaN"
    bad = got.view(np.uint32)[~nan] != exp.view(np.uint32)[~nan]
    if bad.any():
        where = np.argwhere(~nan)[bad][0]
        raise AssertionError(f"{what}: {int(bad.sum())} entries differ, first at "
                             f"{tuple(where)}: got {got[tuple(where)]!r}, "
                             f"expected {exp[tuple(where)]!r}")


# ---- kinship summary -------------------------------------------------------------------------
def slots_of(kin, lo, hi, num_bins):
    """The slot rule, vectorised: float32 operations, one rounding each."""
    lo, hi, nb = f32(lo), f32(hi), f32(num_bins)
    scale = f32(nb / f32(hi - lo))
    with np.errstate(invalid="ignore", over="ignore"):
        t = ((kin - lo).astype(f32) * scale).astype(f32)
        inside = ~np.isnan(kin) & ~(kin < lo) & (t < nb)
    slot = np.where(inside, 1 + np.where(inside, t, 0).astype(np.int64), num_bins + 1)
    slot = np.where(kin < lo, 0, slot)
    return np.where(np.isnan(kin), num_bins + 2, slot)


def histogram_of(kin, lo, hi, num_bins):
    return np.bincount(slots_of(kin, lo, hi, num_bins), minlength=num_bins + 3).astype(u64)


def key_of(kin, partner):
    bits = np.asarray(kin, dtype=f32).view(u32)
    ordered = np.where(bits & u32(0x80000000), ~bits, bits ^ u32(0x80000000)).astype(u32)
    key = (ordered.astype(u64) << u64(32)) | (~np.asarray(partner).astype(u32)).astype(u64)
    return np.where(np.isnan(kin), u64(0), key)


def nearest_of(sm, oi, oj, kin):
    """Arg-max per stored sample of the block (rows first, then columns): the largest
    kinship that is not NaN, the lowest partner among equals.  -> (kin, partner, keys)."""
    i_begin, i_end, j_begin, j_end = sm
    diag = i_begin == j_begin
    rows = i_end - i_begin
    count = rows if diag else rows + (j_end - j_begin)
    off_i = oi - i_begin
    off_j = oj - j_begin + (0 if diag else rows)
    sample = np.concatenate([off_i, off_j]).astype(np.int64)
    partner = np.concatenate([oj, oi]).astype(np.int64)
    k = np.concatenate([kin, kin])
    keep = ~np.isnan(k)
    sample, partner, k = sample[keep], partner[keep], k[keep]
    order = np.lexsort((partner, -k.astype(np.float64), sample))
    sample, partner, k = sample[order], partner[order], k[order]
    first = np.ones(sample.size, dtype=bool)
    first[1:] = sample[1:] != sample[:-1]
    best_kin = np.full(count, f32("nan"), dtype=f32)
    best_partner = np.full(count, -1, dtype=np.int64)
    best_kin[sample[first]] = k[first]
    best_partner[sample[first]] = partner[first]
    keys = np.where(best_partner >= 0, key_of(best_kin, np.maximum(best_partner, 0)), u64(0))
    return best_kin, best_partner, keys


# ---- relative counts -------------------------------------------------------------------------
def bands_of(kin, thresholds):
    """The band rule, vectorised: the largest t with kin > thresholds[t] (strict, float32;
    ascending thresholds: the number of thresholds below kin, less one), -1 = none."""
    thr = np.asarray(thresholds, dtype=f32)
    with np.errstate(invalid="ignore"):
        return (np.asarray(kin, dtype=f32)[:, None] > thr[None, :]).sum(axis=1) - 1


def counts_of(sm, oi, oj, kin, thresholds):
    """[stored samples of the block (rows first, then columns), T] uint32."""
    i_begin, i_end, j_begin, j_end = sm
    diag = i_begin == j_begin
    rows = i_end - i_begin
    count = rows if diag else rows + (j_end - j_begin)
    band = bands_of(kin, thresholds)
    keep = band >= 0
    out = np.zeros((count, len(thresholds)), dtype=u32)
    np.add.at(out, ((oi - i_begin)[keep], band[keep]), 1)
    np.add.at(out, ((oj - j_begin + (0 if diag else rows))[keep], band[keep]), 1)
    return out


# ---- all of them from one oracle call --------------------------------------------------------
Expected = namedtuple("Expected", "pairs matrix hist best_kin best_partner keys bands")


def expect_all(sm, all_pairs, bins, thresholds, sentinel=SENTINEL):
    """From ONE `pyoracle.all_pairs(osm, bits)` result of the block `sm`: the pairs as (oi, oj,
    kin) int64 / int64 / float32; the [rows, columns] matrix with `sentinel` wherever the
    oracle lists no pair; the histogram of `bins` = (lo, hi, num_bins); the nearest relatives
    (kin, partner, keys); the [stored samples, T] band counts of `thresholds`."""
    oi, oj, _, ok = all_pairs
    oi, oj = np.asarray(oi, dtype=np.int64), np.asarray(oj, dtype=np.int64)
    kin = np.asarray(ok, dtype=f32)
    i_begin, i_end, j_begin, j_end = sm
    matrix = np.full((i_end - i_begin, j_end - j_begin), sentinel, dtype=f32)
    matrix[oi - i_begin, oj - j_begin] = kin
    keys = best_keys_of(sm, oi, oj, kin)
    best_kin, best_partner = decode_keys(keys)
    return Expected((oi, oj, kin), matrix, histogram_of(kin, *bins), best_kin, best_partner,
                    keys, counts_of(sm, oi, oj, kin, thresholds))


def best_keys_of(sm, oi, oj, kin):
    """The keys nearest_of gives, as the maximum of key_of over each stored sample's pairs:
    two stable integer sorts where nearest_of sorts three columns of twice the pairs (the 21
    million pairs of a 6,500-sample block: seconds, not half a minute)."""
    i_begin, i_end, j_begin, j_end = sm
    diag = i_begin == j_begin
    rows = i_end - i_begin
    best = np.zeros(rows if diag else rows + (j_end - j_begin), dtype=u64)
    if kin.size == 0:
        return best
    for sample, partner in ((oi - i_begin, oj), (oj - j_begin + (0 if diag else rows), oi)):
        order = np.argsort(sample, kind="stable")
        sample, key = sample[order], key_of(kin, partner)[order]
        starts = np.flatnonzero(np.concatenate([[True], sample[1:] != sample[:-1]]))
        who = sample[starts]
        best[who] = np.maximum(best[who], np.maximum.reduceat(key, starts))
    return best


def decode_keys(keys):
    """(kin float32, partner int64) of uint64 keys; NaN and -1 for key 0."""
    keys = np.asarray(keys, dtype=u64)
    ordered = (keys >> u64(32)).astype(u32)
    bits = np.where(ordered & u32(0x80000000), ordered ^ u32(0x80000000), ~ordered).astype(u32)
    kin = np.where(keys != 0, bits.view(f32), f32("nan")).astype(f32)
    partner = np.where(keys != 0, (~keys & u64(0xFFFFFFFF)).astype(np.int64), np.int64(-1))
    return kin, partner
