"""The PI_HAT sweep without a GPU: what fuzz_cases.run_pihat rests on, held on the generator
(pihat_fuzz_cases.py), the CPU oracle and the numpy restatement (pihat_cases.py) alone, for every
committed (seed, cases, class) of tests/test_gpu_fuzz.py.  These are conditions on the inputs,
not measurements: the seeds were chosen so that they hold.

Printed by this file on the CPU, seeds 701 / 702 / 704 ("small", 40 cases each), 711 ("edges", 30)
and 727 ("tiles", 9):
  pairs      1.75 / 1.20 / 1.51 million, 1.77 million and 17.8 million; the thresholded call
             returns 0.24 / 0.36 / 0.58 million, 0.60 million and 4.3 million of them.
  ties       at 0.0: 37491 / 115178 / 135786, 42606, 1305059; at 0.5: 14 / 18142 / 48218, 89, 7;
             at 1.0: 5 / 6 / 2, 10, 10247.
  SPLIT      10 / 6 / 10 cases of the small sweeps have PI_HAT launches with remainder pieces
             (36 / 20 / 25 launches); no case of the other classes (at most 5 k-steps, or one).
  defects    the first case that tells: `no z2 < 0 step`, `ibs1 = shared - ibs2` and `bounded
             ignored` case 0 of each sweep, `threshold >=` case 1 / 2 / 3, `z1 > 1 step last` case
             7 / 28 / 16, `no float32 rounding` case 33 of seed 704 alone.
  runtime    32 s for the file, 21 s of it the one pass over the three small sweeps."""
import hashlib
from functools import lru_cache

import numpy as np
import pytest

import pihat_cases as pc
import pihat_fuzz_cases as pf

from oracle import pyoracle


def _sweeps():
    import test_gpu_fuzz as sweeps
    return sweeps.PIHAT_SWEEPS


def _digest(ref) -> tuple:
    return tuple(hashlib.sha256(ref.records[key].tobytes()).hexdigest()
                 for key in sorted(ref.records))


@lru_cache(maxsize=None)
def _summary(seed, cases, size_class) -> dict:
    """One pass over a committed sweep: per case the tag, what its block holds of the planted
    rows, the bounding steps its pairs take, its ties and the size of the thresholded call's
    answer; for the class "small" the defects of pihat_cases.DEFECTS that change the reference
    records of some case, with the first such case.  (The references themselves are not kept:
    a case of the class "tiles" has 2.6 million pairs.)"""
    rows, caught = [], {}
    for tag, geno, _ in pf.cases(seed, cases, size_class=size_class):
        model = pf.model_of(tag, geno)
        ref = pf.reference(tag, geno, model)
        rows.append(dict(tag=tag, planted=pf.planted_pairs(tag), taken=dict(ref.taken),
                         ties=ref.ties, pairs=len(ref.all_pairs[0]),
                         records=len(ref.records[(tag["thr"], tag["bounded"])]),
                         everything=len(ref.records[(-1.0, not tag["bounded"])])))
        if size_class != "small":
            continue
        right = _digest(ref)
        for defect in pc.DEFECTS:
            if defect not in caught and \
                    _digest(pf.reference(tag, geno, model, defect, oracle=ref)) != right:
                caught[defect] = tag["case"]
    return dict(rows=rows, caught=caught, split=pf.split_launches([r["tag"] for r in rows]))


@pytest.mark.parametrize("name", sorted(pc.MODELS))
@pytest.mark.parametrize("bounded", [True, False])
def test_vector_restatement_equals_the_scalar_one_bitwise(name, bounded):
    """z_of_counts_np against z_of_counts, the definition: every seeded triple, every model made
    by hand, both settings; any NaN as the one NaN."""
    model = pc.MODELS[name]()
    triples = pc.seeded_triples()
    want = np.array([pc.z_of_counts(model, *t, bounded) for t in triples], dtype=np.float64)
    a = np.array(triples, dtype=np.uint32)
    taken = {}
    got = np.stack(pc.z_of_counts_np(model, a[:, 0], a[:, 1], a[:, 2], bounded, taken=taken),
                   axis=1)
    differ = np.flatnonzero((pc.bits(got) != pc.bits(want)).any(axis=1))
    assert differ.size == 0, [(triples[k], got[k], want[k]) for k in differ[:5]]
    assert taken["nan"] == int(np.isnan(want[:, 3]).sum())
    # ... and records_np keeps the pairs the scalar comparison keeps, in ascending (i, j)
    import cuking_amd
    sm = cuking_amd.Submatrix(len(triples) + 1)
    i = np.arange(len(triples), dtype=np.uint32)[::-1].copy()
    recs = pc.records_np(sm, i, i + 1, a[:, 0], a[:, 1], a[:, 2], model, 0.25, bounded)
    with np.errstate(over="ignore"):
        want32 = want[:, 3].astype(np.float32)
    keep = [k for k in range(len(triples)) if want32[k] > np.float32(0.25)]
    assert recs["sample_i"].tolist() == sorted(int(i[k]) for k in keep)
    by_i = {int(i[k]): k for k in keep}
    for r in recs:
        k = by_i[int(r["sample_i"])]
        assert (r["ibs0"], r["ibs1"], r["ibs2"]) == triples[k]
        assert r["kin"].tobytes() == want32[k].tobytes()


def test_ibs_of_counts_equals_the_oracles_records():
    """The independent leg: ibs0/1/2 from the sums of pyoracle.all_pairs equal the ibs fields of
    the oracle's own records (pyoracle.compute at -1e30), for every pair both list."""
    shared = pairs = 0
    for tag, geno, _ in pf.cases(5, 8, size_class="small"):
        osm = pyoracle.submatrix(tag["n"], tag["split_factor"], tag["shard"])
        bits = pyoracle.bitset_from_genotypes(geno, osm)
        oi, oj, oc, _ = pyoracle.all_pairs(osm, bits)
        recs, overflow, _ = pyoracle.compute(osm, bits, -1e30)
        assert not overflow
        ibs0, ibs1, ibs2 = pc.ibs_of_counts(oc)
        at = {(int(a), int(b)): k for k, (a, b) in enumerate(zip(oi, oj))}
        rows = np.array([at[(int(r["sample_i"]), int(r["sample_j"]))] for r in recs], dtype=int)
        assert np.array_equal(ibs0[rows], recs["ibs0"]) and np.array_equal(ibs1[rows], recs["ibs1"])
        assert np.array_equal(ibs2[rows], recs["ibs2"])
        assert np.array_equal((ibs0.astype(np.int64) + ibs1 + ibs2), oc["shared"])
        shared += len(recs)
        pairs += len(oi)
    assert 0 < shared < pairs           # (the all-missing sample's pairs are no records)


def test_generator_is_deterministic_and_the_skip_names_the_same_cases():
    def digest(tag, geno, spec):
        h = hashlib.sha256(repr(sorted(tag.items())).encode())
        h.update(np.ascontiguousarray(geno).tobytes())
        return h.hexdigest()
    for size_class in pf.SIZE_CLASSES:
        whole = [digest(*c) for c in pf.cases(7, 5, size_class=size_class)]
        again = [digest(*c) for c in pf.cases(7, 5, size_class=size_class)]
        tail = [digest(*c) for c in pf.cases(7, 5, 3, size_class=size_class)]
        assert whole == again and tail == whole[3:]
    with pytest.raises(ValueError):
        next(pf.cases(7, 1, size_class="giveup"))


def test_shapes_of_the_classes():
    for seed, cases, size_class in _sweeps():
        for tag in pf.tags(seed, cases, size_class=size_class) if size_class != "small" else \
                [r["tag"] for r in _summary(seed, cases, size_class)["rows"]]:
            n, m = tag["n"], tag["m"]
            b = pf.block_of(tag)
            assert b[1] > b[0] and b[3] > b[2], tag
            if size_class == "edges":
                assert min(abs(n - e) for e in (128, 256, 384, 512)) <= 1 and tag["split_factor"] == 1
                assert min(abs(m - 64 * q) for q in range(1, 20)) <= 1
            elif size_class == "tiles":
                assert 1400 <= n <= 2300 and 1 <= m <= 600 and pf.num_tiles(tag) * \
                    (4 if tag["variant"] == 7 else 1) >= 64
            else:
                assert 2 <= n <= 700 and (1 <= m <= 2500 or 8000 <= m <= 30000)
                assert (m >= 8000) == (tag["split_wgs"] in (3, 6, 16))
    # sites one off a multiple of the k-step are among the edges
    assert any(abs(m - q * pf.K_STEP_SITES) == 1 for m in pf.EDGE_SITES for q in (1, 2, 3, 4))


def test_conditions_across_each_committed_sweep():
    measured = []
    for seed, cases, size_class in _sweeps():
        s = _summary(seed, cases, size_class)
        rows = s["rows"]
        assert len(rows) == cases
        taken = {step for r in rows for step, count in r["taken"].items() if count}
        assert taken == set(pc.BRANCHES), (seed, sorted(set(pc.BRANCHES) - taken))
        specs = [r["tag"]["model"] for r in rows]
        assert set(specs) == set(pf.SPECS), seed
        assert 4 * sum(spec in pf.HAND_MODELS for spec in specs) >= len(specs)
        assert {r["tag"]["variant"] for r in rows} == set(pf.VARIANTS)
        ties = {}
        for r in rows:
            ties[r["tag"]["thr"]] = ties.get(r["tag"]["thr"], 0) + r["ties"]
        assert all(ties.get(t, 0) > 0 for t in pf.TIE_THRESHOLDS), (seed, ties)
        for variant in pf.VARIANTS:
            assert any(0 < r["records"] < r["pairs"] for r in rows
                       if r["tag"]["variant"] == variant), (seed, variant)
        for what in ("all_missing", "parent_child", "duplicate"):
            assert any(r["planted"][what] for r in rows), (seed, what)
        # at -1.0 every pair that is not NaN is a record: fewer than the block's pairs wherever
        # the all-missing sample is in the block
        assert all(r["everything"] < r["pairs"] for r in rows if r["planted"]["all_missing"])
        if size_class == "small":
            assert sum(s["split"]) > 0, seed
        measured.append(f"seed {seed} ({size_class}): {sum(r['pairs'] for r in rows)} pairs, "
                        f"{sum(r['records'] for r in rows)} records of the thresholded call, ties "
                        f"{ {t: ties.get(t, 0) for t in pf.TIE_THRESHOLDS} }, "
                        f"{sum(c > 0 for c in s['split'])} cases with SPLIT launches "
                        f"({sum(s['split'])} launches)")
    print("\n".join(measured))


def test_every_defect_changes_the_reference_of_a_small_sweep():
    """Each subtly wrong restatement of pihat_cases.DEFECTS changes the reference records of at
    least one case of the committed sweeps of the class "small": the inputs can tell a kernel
    that is wrong in that way from a right one.  (Five of the six are told by every such sweep;
    "no float32 rounding" needs a pair whose double PI_HAT lies above the threshold by less than
    half a float32 step, which one of the three sweeps holds.)"""
    told = set()
    for seed, cases, size_class in _sweeps():
        if size_class != "small":
            continue
        caught = _summary(seed, cases, size_class)["caught"]
        print(f"seed {seed}: first case that tells, per defect: {caught}")
        assert set(pc.DEFECTS) - set(caught) <= {"no float32 rounding"}, (seed, caught)
        told |= set(caught)
    assert told == set(pc.DEFECTS), sorted(set(pc.DEFECTS) - told)
