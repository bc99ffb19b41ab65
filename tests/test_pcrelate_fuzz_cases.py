"""The PC-Relate sweep without a GPU: what fuzz_cases.run_pcrelate rests on, held on the
generator (pcrelate_fuzz_cases.py), the float64 references and the host twins alone, for every
committed (seed, cases, class) of tests/test_gpu_fuzz.py.

Measured on the CPU with this file (it prints them), seeds 601 / 602 / 603 ("small", 60 cases
each) and 611 ("tiles", 40 cases):
  rounds     no case needed more than ONE round of redrawing (24 / 18 / 14 of 60 needed one, 14 of
             40 in "tiles"; the exact sweep, seed 621, has no margin condition).
  compared   0.991 / 0.991 / 0.989 and 0.992 of the matrix entries are not NaN (the all-missing
             sample's row and column are most of the rest); 0.989 in the exact sweep.
  defects    cases whose matrix a defect moves by at least 10 tolerances, of 60 / 60 / 60 / 40:
             missing as hom-ref 60 / 60 / 60 / 39, factor 4 dropped 60 / 60 / 60 / 40, last step
             skipped 60 / 60 / 59 / 39, planes swapped 60 / 60 / 60 / 40, bounds ignored 59 / 57 /
             59 / 39, beta reversed 58 / 60 / 56 / 40 (d = 1 is immune to it).
  host twins 12 cases of each of the five sweeps go through the three host twins in 5 s.
"""
import hashlib
from functools import lru_cache

import numpy as np
import pytest

import pcrelate_cases as pc
import pcrelate_fuzz_cases as pf
import pcrelate_pairs_cases as pp
import pcrelate_records_cases as rc

from cuking_amd import pcrelate as pcr

HOST_CASES = 12     # cases of every committed sweep that go through the host twins here


def _sweeps():
    import test_gpu_fuzz as sweeps
    return sweeps.PCRELATE_SWEEPS


@lru_cache(maxsize=None)
def _drawn(seed, cases, size_class):
    return tuple(pf.pcrelate_sweep_cases(seed, cases, size_class=size_class))


def test_every_case_is_delivered_within_the_rounds_and_the_share_is_compared():
    """The delivery condition (a case that kept a margin violation would raise in the
    generator), the compared share the GPU gate asserts, the D buckets and the split launches
    it asserts, from the reference alone."""
    for seed, cases, size_class in _sweeps():
        drawn = _drawn(seed, cases, size_class)
        assert len(drawn) == cases
        entries = compared = split = 0
        rounds, buckets = [], set()
        for tag, inp in drawn:
            assert tag["rounds"] <= pf.MAX_ROUNDS
            rounds.append(tag["rounds"])
            buckets.add(pf.bucket(tag["d"]))
            split += sum(pf.split_launches(tag).values())
            if size_class != "exact":
                assert inp.ref.margin_violations() == 0 == inp.pair_ref.margin_violations()
                kin = inp.ref.kin
            else:
                kin = pc.exact_expected_of(inp.code, inp.beta, inp.block)
            entries += kin.size
            compared += int((~np.isnan(kin)).sum())
        print(f"seed {seed} ({size_class}): rounds {np.bincount(rounds).tolist()}, "
              f"{compared} of {entries} entries not NaN ({compared / entries:.3f}), "
              f"{split} split calls, D buckets {sorted(buckets)}")
        assert split > 0
        assert sorted(buckets) == ([4] if size_class == "exact" else [4, 8, 16, 32])
        if size_class != "exact":
            assert compared >= 0.9 * entries, (seed, compared, entries)


def test_generator_is_deterministic_and_the_skip_names_the_same_cases():
    def digest(tag, inp):
        h = hashlib.sha256(repr(sorted(tag.items())).encode())
        for a in (inp.bits, np.ascontiguousarray(inp.x), np.ascontiguousarray(inp.beta),
                  inp.index, np.ascontiguousarray(inp.pairs).view(np.uint8), inp.part):
            h.update(np.ascontiguousarray(a).tobytes())
        return h.hexdigest()
    for size_class in pf.SIZE_CLASSES:
        whole = [digest(*c) for c in pf.pcrelate_sweep_cases(7, 6, size_class=size_class)]
        again = [digest(*c) for c in pf.pcrelate_sweep_cases(7, 6, size_class=size_class)]
        tail = [digest(*c) for c in pf.pcrelate_sweep_cases(7, 6, 4, size_class=size_class)]
        assert whole == again and tail == whole[4:]


def test_blocks_are_valid_and_the_menu_is_drawn():
    kinds = set()
    for seed, cases, size_class in _sweeps():
        for tag, inp in _drawn(seed, cases, size_class):
            n, (i0, i1, j0, j1) = tag["n"], inp.block
            assert 0 <= i0 < i1 <= n and 0 <= j0 < j1 <= n
            assert (i0, i1) == (j0, j1) or i1 <= j0        # identical, or disjoint rows first
            a0, a1, b0, b1 = inp.sub_block
            assert i0 <= a0 < a1 <= i1 and j0 <= b0 < b1 <= j1
            assert (a0, a1) == (b0, b1) or a1 <= b0
            assert inp.index.shape == (tag["pairs"], 2) and tag["pairs"] >= 1
            if tuple(inp.block) != (0, n, 0, n):
                kinds.add(tag["kind"])
    assert kinds == set(pf.BLOCK_MENU), kinds
    # the widest menu entry where the cohort has the samples: two tiles more columns than rows
    i0, i1, j0, j1 = pf.draw_block(385, "wide rectangle", [0.5, 0.9, 0.9, 0.9, 0.5])
    assert (j1 - j0) - (i1 - i0) >= 2 * pf.TILE


def _on_host(tag, inp):
    """One case through the host twins: what run_pcrelate asks of the device, without one."""
    model = (inp.bits, inp.wps, tag["sites"], inp.x, inp.beta, inp.lo, inp.hi)
    exact = tag["size_class"] == "exact"
    kin = pcr.pcrelate_matrix_host(*model, block=inp.block)
    rows = pcr.pcrelate_pairs_raw_host(*model, inp.pairs, inp.f)
    pp.check_rows_of(inp.index, rows)
    if exact:
        assert kin.tobytes() == pc.exact_expected_of(inp.code, inp.beta, inp.block).tobytes()
        assert rows.tobytes() == pp.exact_expected_of(inp).tobytes()
    else:
        pc.check_reference_of(inp.ref, kin, "matrix", quiet=True)
        pp.check_reference_of(inp.pair_ref, inp.index, rows, "pairs", quiet=True)
    sub = inp.sub_block
    part = pcr.pcrelate_matrix_host(*model, block=sub)
    b = inp.block
    assert part.tobytes() == np.ascontiguousarray(
        kin[sub[0] - b[0]:sub[1] - b[0], sub[2] - b[2]:sub[3] - b[2]]).tobytes()
    values = np.sort(kin[rc.pair_mask(inp.block) & ~np.isnan(kin)])
    on_value = [float(values[int(q * values.size)]) for q in (0.5, 0.95)] if values.size else []
    for t in [-rc.INF, rc.INF] + on_value:
        recs, count = pcr.pcrelate_records_raw_host(*model, t, block=inp.block)
        rc.check_records(recs, inp.block)
        rc.same_records(recs, rc.threshold_matrix(kin, inp.block, t))
        if t == -rc.INF and not exact:
            rc.check_records_reference(inp.ref, inp.block, recs, "records", quiet=True)
    moved = pcr.pcrelate_pairs_raw_host(*model, np.ascontiguousarray(inp.pairs[inp.part]), inp.f)
    assert moved.tobytes() == rows[inp.part].tobytes()


def test_the_generator_through_the_host_twins():
    for seed, cases, size_class in _sweeps():
        for tag, inp in _drawn(seed, cases, size_class)[:HOST_CASES]:
            try:
                _on_host(tag, inp)
            except AssertionError as e:
                raise AssertionError(f"{tag}: {e}") from e


def test_every_defect_is_caught_by_every_seed():
    """For every defect of pcrelate_cases.DEFECTS, every committed sweep of a real-valued class
    holds a case whose matrix the defect moves by at least 10 tolerances; the share of cases
    that do is printed (and stands in the module docstring)."""
    for seed, cases, size_class in _sweeps():
        if size_class == "exact":
            continue
        caught = {defect: 0 for defect in pc.DEFECTS}
        for tag, inp in _drawn(seed, cases, size_class):
            for defect in pc.DEFECTS:
                bad = pc.Reference(inp.code, inp.x, inp.beta, inp.lo, inp.hi, inp.block, defect)
                caught[defect] += pc.defect_ratio_of(inp.ref, bad) >= 10.0
        print(f"seed {seed} ({size_class}): of {cases} cases, caught by " +
              ", ".join(f"{k}: {v}" for k, v in caught.items()))
        assert all(v > 0 for v in caught.values()), (seed, caught)
