"""PI_HAT without a GPU: the Python restatement of pihat_cases.py against exact rationals, the
host twins against the restatement bit for bit, cuking_compute_pihat_host against a per-site
numpy walk byte for byte and against the oracle's KING records, the smoke() cohort with its
measured gap, the refusals, the ABI symbols, and the stand-alone sanitizer driver."""
import ctypes as C
import math
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import cuking_amd
from cuking_amd import _lib
from cuking_amd.pihat import PiHatModel, site_counts_of_host_bits

import pihat_cases as pc
from host_driver import run_sanitized_driver
from oracle import pyoracle

ROOT = Path(__file__).resolve().parent.parent


def block_bits(host, sm):
    """The stored samples of block `sm`: its rows, then an off-diagonal block's columns."""
    if sm.i_begin == sm.j_begin:
        return np.ascontiguousarray(host[sm.i_begin:sm.i_end])
    return np.ascontiguousarray(np.concatenate([host[sm.i_begin:sm.i_end],
                                                host[sm.j_begin:sm.j_end]]))


def test_restatement_against_exact_rationals():
    """Every count row of 2 .. 12 people.  Both identities hold exactly in the rationals.  A term
    is at most four exact factors multiplied (three roundings), two such products, one or two
    sums and a divide by a product of three roundings: about ten roundings, 10 * 2^-53 ~ 1.1e-15.
    Bound 1e-14; measured on the CPU: 1.06e-16 (N <= 24: every product here is exact)."""
    worst = 0.0
    for row in pc.small_rows(12):
        exact, got = pc.site_terms_exact(*row), pc.site_terms(*row)
        assert exact[0] + exact[1] + exact[2] == 1 and exact[3] + exact[4] == 1, row
        for e, f in zip(exact, got):
            if e == 0:
                assert f == 0.0 and not math.copysign(1.0, f) < 0, row
                continue
            rel = abs(Fraction(f) - e) / e
            worst = max(worst, float(rel))
            assert rel <= Fraction(1, 10 ** 14), (row, f, float(e))
    print(f"worst relative error vs exact arithmetic: {worst:.3g}")
    # ... and the model of all of them: 454 sums of terms in [0, 1], each sum one rounding
    rows = pc.small_rows(12)
    model = pc.model_of_rows(rows)
    for k in range(5):
        exact = sum(pc.site_terms_exact(*r)[k] for r in rows) / len(rows)
        assert abs(Fraction(model[k]) - exact) / exact <= Fraction(len(rows), 2 ** 52)
    assert model[5] == len(rows)


def test_model_host_equals_restatement_bitwise():
    rows = pc.seeded_count_rows()
    counts = pc.counts_array(rows)
    got = cuking_amd.pi_hat_model_host(counts, len(rows))
    want = pc.model_of_rows(rows)
    assert got.sites_used == want[5] == sum(1 for r in rows if sum(r) >= 2)
    assert pc.bits(got.as_tuple()[:5]).tolist() == pc.bits(want[:5]).tolist()
    # fewer sites read fewer rows; int32 counts are the same bytes
    for n in (0, 1, 5, 11, 100):
        got = cuking_amd.pi_hat_model_host(counts.view(np.int32), n)
        want = pc.model_of_rows(rows[:n])
        assert got.sites_used == want[5]
        assert pc.bits(got.as_tuple()[:5]).tolist() == pc.bits(want[:5]).tolist(), n
    # no used site: NaNs, and no pair qualifies
    empty = cuking_amd.pi_hat_model_host(pc.counts_array([(0, 0, 0), (1, 0, 0)]), 2)
    assert empty.sites_used == 0 and all(math.isnan(x) for x in empty.as_tuple()[:5])
    z = cuking_amd.pi_hat_of_records(pc.records_of_triples([(1, 2, 3)]), empty)
    assert np.isnan(z).all()
    # a monomorphic site needs no special case: a00 = a01 = a11 = 0, a02 = a12 = 1
    mono = cuking_amd.pi_hat_model_host(pc.counts_array([(40, 0, 0)]), 1)
    assert mono.as_tuple() == (0.0, 0.0, 1.0, 0.0, 1.0, 1)
    # more than 2^24 people in a row fails the call
    with pytest.raises(_lib.CukingError, match="2\\^24"):
        cuking_amd.pi_hat_model_host(pc.counts_array([(1, 1, 1), (pc.MAX_PEOPLE, 1, 0)]), 2)
    assert cuking_amd.pi_hat_model_host(pc.counts_array([(pc.MAX_PEOPLE, 0, 0)]), 1).sites_used == 1


MODELS = pc.MODELS


@pytest.mark.parametrize("name", sorted(MODELS))
@pytest.mark.parametrize("bounded", [True, False])
def test_records_host_equals_restatement_bitwise(name, bounded):
    model = MODELS[name]()
    triples = pc.seeded_triples()
    recs = pc.records_of_triples(triples)
    got = cuking_amd.pi_hat_of_records(recs, PiHatModel(*model), bounded=bounded)
    assert got.dtype == np.float64 and got.shape == (len(triples), 4)
    want = np.array([pc.z_of_counts(model, *t, bounded) for t in triples], dtype=np.float64)
    differ = np.flatnonzero((pc.bits(got) != pc.bits(want)).any(axis=1))
    assert differ.size == 0, [(triples[k], got[k], want[k]) for k in differ[:5]]
    assert np.isnan(got[0]).all()                        # S = 0
    # num_records reads fewer rows
    few = cuking_amd.pi_hat_of_records(recs, PiHatModel(*model), bounded, num_records=7)
    assert pc.bits(few).tolist() == pc.bits(want[:7]).tolist()


def test_every_bounding_branch_is_driven():
    seen = set()
    for name in ("333 x 5000", "negative e00"):
        model = MODELS[name]()
        for t in pc.seeded_triples():
            raw = pc.z_of_counts(model, *t, bounded=False)
            got = pc.z_of_counts(model, *t, bounded=True)
            if raw[0] != raw[0]:
                seen.add("nan")
                continue
            for k in range(3):
                if raw[k] > 1.0:
                    seen.add(f"z{k} > 1")
                if raw[k] < 0.0:
                    seen.add(f"z{k} < 0")
            if name == "negative e00":
                continue
            assert all(0.0 <= z <= 1.0 for z in got[:3]), (t, raw, got)
            assert abs(sum(got[:3]) - 1.0) < 1e-9 and 0.0 <= got[3] <= 1.0, (t, got)
    assert seen == {"nan", "z0 > 1", "z1 > 1", "z2 > 1", "z0 < 0", "z1 < 0", "z2 < 0"}, seen
    # a zero e00 takes what IEEE gives: ibs0 / 0 is inf (z0 > 1 -> (1, 0, 0)) or NaN
    zero = MODELS["zero e00"]()
    assert zero[0] == 0.0
    assert pc.z_of_counts(zero, 3, 5, 9)[:3] == (1.0, 0.0, 0.0)
    assert all(math.isnan(z) for z in pc.z_of_counts(zero, 0, 5, 9))


SHAPES = [(2, 64, "ones"), (5, 130, "ones"), (70, 1000, "zeros"), (70, 1000, "ones")]


@pytest.mark.parametrize("n,m,pad", SHAPES)
def test_compute_host_equals_numpy_walk(n, m, pad):
    rng = np.random.default_rng(1000 * n + m)
    wps = cuking_amd.words_per_sample(m)
    host = pc.random_bits(rng, n, m, wps, pad)
    g = pc.genotypes_of_bits(host, wps)
    counts = pc.site_counts_of_genotypes(g)
    assert np.array_equal(counts, site_counts_of_host_bits(host, wps))
    model_t = pc.model_of_rows([tuple(int(x) for x in c[:3]) for c in counts[:m]])
    model = cuking_amd.pi_hat_model_host(counts, m)
    assert pc.bits(model.as_tuple()[:5]).tolist() == pc.bits(model_t[:5]).tolist()
    blocks = [cuking_amd.Submatrix(n)]
    if n >= 5:
        blocks += [cuking_amd.Submatrix(n, 2, k) for k in range(3)]
    for sm in blocks:
        bits_b = block_bits(host, sm)
        # (all-zero padding reads as hom-ref and counts as IBS2 in the twin as in a KING record:
        #  the walk covers every bit of the planes; all-ones padding is missing and counts nowhere)
        walk_g = pc.genotypes_of_bits(bits_b, wps)
        for bounded in (True, False):
            want = pc.walk_records(sm, walk_g, model_t, 0.05, bounded)
            got = cuking_amd.pi_hat_records_host(sm, wps, bits_b, m, min_pi_hat=0.05,
                                                 model=model, bounded=bounded)
            assert got.num_records == len(want) and got.records.dtype == cuking_amd.KING_RESULT_DTYPE
            assert got.records.tobytes() == want.tobytes(), (sm, bounded)
            assert got.sorted().tobytes() == want.tobytes()     # ascending (i, j) already
        # counting, exact, one short
        total = len(want)
        exact = cuking_amd.pi_hat_records_host(sm, wps, bits_b, m, 0.05, model=model,
                                               bounded=False, max_results=total)
        assert exact.records.tobytes() == want.tobytes()
        if total:
            for cap in (0, total - 1):
                with pytest.raises(cuking_amd.ResourceExhaustedError) as e:
                    cuking_amd.pi_hat_records_host(sm, wps, bits_b, m, 0.05, model=model,
                                                   bounded=False, max_results=cap)
                assert e.value.num_records == total
            # the raw call: the count, and nothing written past the buffer
            buf = np.zeros(total + 3, dtype=cuking_amd.KING_RESULT_DTYPE)
            count = C.c_uint32(0)
            st = _lib.load().cuking_compute_pihat_host(
                C.byref(sm.c), wps, bits_b.ctypes.data, C.byref(model.c), 0.05,
                _lib.PIHAT_UNBOUNDED, total - 1, buf.ctypes.data, C.byref(count))
            assert st == _lib.ERR_RESOURCE_EXHAUSTED and count.value == total
            assert buf[:total - 1].tobytes() == want[:total - 1].tobytes()
            assert not buf[total - 1:].view(np.uint8).any()
        # the ibs fields are those of the oracle's KING records, for every pair both list
        king, _, _ = pyoracle.compute(pyoracle.Submatrix(*sm.as_tuple()), bits_b, -1e30)
        every = cuking_amd.pi_hat_records_host(sm, wps, bits_b, m, -1.0, model=model).records
        both = {(int(r["sample_i"]), int(r["sample_j"])): r for r in king}
        shared = 0
        for r in every:
            k = both.get((int(r["sample_i"]), int(r["sample_j"])))
            if k is not None:
                shared += 1
                assert (r["ibs0"], r["ibs1"], r["ibs2"]) == (k["ibs0"], k["ibs1"], k["ibs2"])
        assert shared > 0


def test_smoke_cohort():
    """The smoke() cohort: 333 x 5000, `baseline`.  It plants 17 pairs, not 15: 14 parent-child,
    1 duplicate, 1 full-sibling and 1 half-sibling pair.  Measured with the host twin on the CPU
    (model of the cohort's own samples, bounded): the largest PI_HAT of an unplanted pair is
    0.14300692 ((4, 330)), the smallest of a planted one 0.26482689 (the half-siblings (331,
    332)); the full siblings sit at 0.5 among the parent-child pairs, so no threshold on PI_HAT
    returns the 15 parent-child and duplicate pairs alone: the clean gap is the one between
    planted and unplanted pairs, and the scan at its middle returns exactly the 17."""
    cohort, host, wps = pc.smoke_cohort()
    n, m = pc.SMOKE["n"], pc.SMOKE["m"]
    sm = cuking_amd.Submatrix(n)
    every = cuking_amd.pi_hat_records_host(sm, wps, host, m, min_pi_hat=-1.0)
    assert every.num_records == n * (n - 1) // 2 and every.model.sites_used == m
    planted = {(min(a, b), max(a, b)): kind for a, b, kind in cohort.planted}
    kinds = sorted(planted.values())
    assert kinds.count("po") + kinds.count("dup") == 15 and len(planted) == 17
    key = [(int(r["sample_i"]), int(r["sample_j"])) for r in every.records]
    is_planted = np.array([k in planted for k in key])
    lo, hi = pc.SMOKE_GAP
    assert float(every.records["kin"][~is_planted].max()) == lo
    assert float(every.records["kin"][is_planted].min()) == hi
    assert hi - lo > 0.1
    found = cuking_amd.pi_hat_records_host(sm, wps, host, m, min_pi_hat=(lo + hi) / 2)
    assert found.num_records == 17
    assert {(int(a), int(b)) for a, b in found.pairs()} == set(planted)
    z = found.z()
    kind = [planted[(int(a), int(b))] for a, b in found.pairs()]
    by_z1 = [kind[k] for k in np.argsort(-z[:, 1], kind="stable")]
    assert by_z1[:14] == ["po"] * 14                 # parent-child pairs have the largest z1
    assert kind[int(np.argmax(z[:, 2]))] == "dup" and z[:, 2].max() == 1.0
    # the 15 parent-child and duplicate pairs: z0 = 0 (bounded), PI_HAT 1/2 and 1
    strong = np.array([k in ("po", "dup") for k in kind])
    assert strong.sum() == 15 and (z[strong, 0] < 0.02).all()
    assert np.allclose(z[strong, 3], [1.0 if k == "dup" else 0.5 for k in kind if k in ("po", "dup")],
                       atol=0.03)
    # the wrapper's default threshold is the third-degree cut-off doubled
    assert cuking_amd.pihat.DEFAULT_MIN_PI_HAT == 2 * cuking_amd.KING_CUTOFFS[0]


def test_refusals():
    lib = _lib.load()
    sm = cuking_amd.Submatrix(4)
    bits = np.zeros((4, 2), dtype=np.uint64)
    model = PiHatModel(0.1, 0.4, 0.5, 0.4, 0.6, 10)
    n = C.c_uint32(9)
    recs = np.zeros(8, dtype=cuking_amd.KING_RESULT_DTYPE)
    args = (C.byref(sm.c), 2, bits.ctypes.data, C.byref(model.c), 0.1)
    assert lib.cuking_compute_pihat_host(*args, 2, 8, recs.ctypes.data, C.byref(n)) == 1
    assert b"unknown flags" in lib.cuking_last_error() and n.value == 0
    assert lib.cuking_compute_pihat_host(C.byref(sm.c), 2, bits.ctypes.data, None, 0.1, 0, 8,
                                         recs.ctypes.data, C.byref(n)) == 1
    assert b"null model" in lib.cuking_last_error()
    assert lib.cuking_compute_pihat_host(*args, 0, 8, None, C.byref(n)) == 1
    assert lib.cuking_compute_pihat_host(*args, 0, 8, recs.ctypes.data, None) == 1
    assert lib.cuking_compute_pihat_host(C.byref(sm.c), 3, bits.ctypes.data, C.byref(model.c),
                                         0.1, 0, 8, recs.ctypes.data, C.byref(n)) == 1
    # (all hom-ref: every pair is IBS2 everywhere, PI_HAT 1; max_results = 0 counts them)
    assert lib.cuking_compute_pihat_host(*args, 0, 0, None, C.byref(n)) == 3 and n.value == 6
    # NaN threshold: no pair
    assert lib.cuking_compute_pihat_host(C.byref(sm.c), 2, bits.ctypes.data, C.byref(model.c),
                                         float("nan"), 0, 8, recs.ctypes.data, C.byref(n)) == 0
    assert n.value == 0
    assert lib.cuking_pihat_records_host(recs.ctypes.data, 8, C.byref(model.c), 4, None) == 1
    assert lib.cuking_pihat_records_host(None, 8, C.byref(model.c), 0, None) == 1
    assert lib.cuking_pihat_records_host(None, 0, C.byref(model.c), 0, None) == 0
    assert lib.cuking_pihat_model_host(None, 3, C.byref(model.c)) == 1
    assert lib.cuking_pihat_model_host(None, 0, None) == 1
    # the device forms refuse a null context before anything touches a device
    assert lib.cuking_compute_pihat(None, C.byref(sm.c), 2, bits.ctypes.data, C.byref(model.c),
                                    0.1, 0, 0, None, recs.ctypes.data, recs.ctypes.data,
                                    None) == 1
    assert b"null context" in lib.cuking_last_error()
    with pytest.raises(ValueError, match="counts or model"):
        cuking_amd.pi_hat_records_host(sm, 2, bits, 64, counts=np.zeros((64, 4), np.uint32),
                                       model=model)
    with pytest.raises(ValueError, match="counts"):
        cuking_amd.pi_hat_model_host(np.zeros((3, 4), np.uint32), 4)
    with pytest.raises(ValueError, match="model"):
        cuking_amd.pi_hat_records_host(sm, 2, bits, 64, model=(0.1, 0.4, 0.5, 0.4, 0.6, 3))


def test_abi_symbols_and_exports():
    lib = _lib.load()
    raw = C.CDLL(lib._name)
    header = (ROOT / "include" / "cuking_amd.h").read_text()
    for name in ("cuking_pihat_model_host", "cuking_pihat_records_host",
                 "cuking_compute_pihat_host", "cuking_compute_pihat",
                 "cuking_compute_pihat_tiles"):
        assert getattr(raw, name) is not None and name in _lib.SIGNATURES
        assert name + "(" in header
    assert "#define CUKING_PIHAT_UNBOUNDED 1u" in header and _lib.PIHAT_UNBOUNDED == 1
    assert C.sizeof(_lib.CPihatModel) == 48
    import inspect
    sig = inspect.signature(cuking_amd.KingContext.pi_hat_records)
    assert list(sig.parameters) == ["self", "sm", "words_per_sample", "bits", "num_sites",
                                    "min_pi_hat", "counts", "model", "bounded", "max_results",
                                    "stream"]
    assert sig.parameters["min_pi_hat"].default == 2 * cuking_amd.KING_CUTOFFS[0]
    assert sig.parameters["bounded"].default is True
    for name in ("pi_hat_model_host", "pi_hat_of_records", "pi_hat_records_host",
                 "pi_hat_records_device", "PiHatRecords", "PiHatModel"):
        assert hasattr(cuking_amd, name)


def test_host_side_under_asan_ubsan(tmp_path):
    """csrc/king_host.cc and a stand-alone driver (tests/pihat_host_driver.cc) built with
    AddressSanitizer + UBSan, contraction off.  A program of its own on the CPU: nothing is loaded
    into Python.  It recomputes the model of the seeded rows and the branch triples; the test
    compares the bits with the restatement."""
    rows = pc.seeded_count_rows(num=40)
    triples = pc.BRANCH_TRIPLES
    text = f"{len(rows)} {len(triples)}\n" + "".join(f"{a} {b} {c}\n" for a, b, c in rows) + \
        "".join(f"{a} {b} {c}\n" for a, b, c in triples)
    done = run_sanitized_driver(tmp_path, "pihat_host_driver", stdin=text)
    lines = done.stdout.splitlines()
    model = pc.model_of_rows(rows)
    got = next(l for l in lines if l.startswith("model "))
    words = got.split()[1:]
    assert [int(w, 16) for w in words[:5]] == pc.bits(model[:5]).tolist()
    assert int(words[5]) == model[5]
    zl = [l for l in lines if l.startswith("z ")]
    assert len(zl) == 2 * len(triples)
    k = 0
    for bounded in (True, False):
        for t in triples:
            want = pc.bits(pc.z_of_counts(model, *t, bounded)).tolist()
            got = np.array([int(w, 16) for w in zl[k].split()[1:]], dtype=np.uint64)
            assert pc.bits(got.view(np.float64)).tolist() == want, (t, bounded)   # (any NaN)
            k += 1


def test_admixed_cohort_inflates_pi_hat_where_pcrelate_does_not():
    """PI_HAT assumes one homogeneous population.  On the `admixed` model (two ancestries; 192
    samples x 4000 sites, seed 7, every pair of founders is unrelated) the pooled allele
    frequencies make two founders of the SAME ancestry look alike: their PI_HAT is positive on
    average and a good share of them passes the default threshold, while pairs across the
    ancestries are bounded to 0; PC-Relate on one principal component, on the scale of PI_HAT
    (2 x kinship), stays around 0 for both.  The bounds are qualitative, set from that reasoning
    and not from the figures: a tenth of the same-ancestry pairs against a hundredth.  Measured
    on the CPU: same ancestry (9027 pairs) mean PI_HAT 0.0348, 18.7 % above 0.0884, 0.35 % above
    0.1875; 2 x PC-Relate kinship mean -0.0106, 0.08 % above 0.0884.  Across (9118 pairs): mean
    PI_HAT 0.0006, 0.12 % above; 2 x PC-Relate mean -0.0001, 0.44 % above."""
    import synth_models_twin as twin
    from cuking_amd.synth import plan_cohort
    n, m, seed = 192, 4000, 7
    cohort = plan_cohort(n, seed)
    bits = twin.synth_bitset("admixed", seed, cohort.kind, cohort.pa, cohort.pb, 0, n, m)
    wps = bits.shape[1]
    founder = np.asarray(cohort.kind) == 0
    ancestry = twin.ancestry("admixed", seed, np.arange(n))
    every = cuking_amd.pi_hat_records_host(cuking_amd.Submatrix(n), wps, bits, m, -1.0).records
    pi_hat = np.full((n, n), np.nan)
    pi_hat[every["sample_i"], every["sample_j"]] = every["kin"]
    pca = cuking_amd.pca_host(bits, wps, m, k=2, fit=founder)
    twice_kin = 2.0 * np.asarray(
        cuking_amd.pcrelate_host(bits, wps, m, pca.scores[:, :1], fit=pca.fit).kin)
    pairs = np.triu(founder[:, None] & founder[None, :], 1)
    same = pairs & (ancestry[:, None] == ancestry[None, :])
    cross = pairs & ~same
    assert same.sum() > 5000 and cross.sum() > 5000
    thr = cuking_amd.pihat.DEFAULT_MIN_PI_HAT
    for name, mask in (("same ancestry", same), ("across", cross)):
        print(f"{name}: {mask.sum()} pairs, PI_HAT mean {pi_hat[mask].mean():.4f}, above {thr}: "
              f"{(pi_hat[mask] > thr).mean():.4f}; 2 x PC-Relate mean {twice_kin[mask].mean():.4f},"
              f" above: {(twice_kin[mask] > thr).mean():.4f}")
    assert (pi_hat[same] > thr).mean() > 0.10 > 0.01 > (twice_kin[same] > thr).mean()
    assert (pi_hat[cross] > thr).mean() < 0.01 and (twice_kin[cross] > thr).mean() < 0.01
    assert pi_hat[same].mean() > 10 * pi_hat[cross].mean() > 0
    assert abs(twice_kin[same].mean()) < pi_hat[same].mean() / 2
