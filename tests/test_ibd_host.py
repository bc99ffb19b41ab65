"""IBD segments for listed pairs without a GPU: the host twin against the naive restatement of
ibd_cases.py (rows and sorted segments, bytewise), the row rules, every refusal with its message,
the overflow rule, genome_length / proportions() / relationship() on hand-made values, the .bim
positions, the stand-alone sanitizer driver, and the end-to-end check on the synthetic cohort."""
import ctypes as C
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

import ibd_cases as ic
from host_driver import run_sanitized_driver

import cuking_amd
from cuking_amd import _lib, ibd, plink
from cuking_amd import pcrelate as pcr

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("case", ic.CASES, ids=lambda c: c.name)
def test_host_twin_equals_the_naive_restatement(case):
    ic.check_case(case)
    rows, segments = ic.run_host(case)
    ic.check_against(case, rows, segments, "host twin")
    # all-ones padding beyond num_sites: the same bytes
    padded_rows, padded_segments = ic.run_host(case, ones_padding=True)
    assert padded_rows.tobytes() == rows.tobytes()
    assert padded_segments.tobytes() == segments.tobytes()


@pytest.mark.parametrize("seed", ic.FUZZ_SEEDS)
def test_host_twin_fuzz(seed):
    case = ic.fuzz_case(seed)
    ic.check_case(case)
    ic.check_against(case, *ic.run_host(case), "host twin")


def test_the_case_list_covers_the_kernel_constants():
    text = (ROOT / "cuking_amd" / "csrc" / "king_ibd.hip").read_text()
    assert "constexpr uint32_t kIbdStepWords = 64;" in text and ic.STEP == 64 * 64
    header = (ROOT / "include" / "cuking_amd.h").read_text()
    assert f"#define CUKING_IBD_MIN_SITES {ic.MIN}" in header and _lib.IBD_MIN_SITES == ic.MIN
    assert {1, 63, 64, 65, ic.STEP, ic.STEP + 1, 2 * ic.STEP + 37} <= {c.sites for c in ic.CASES}
    assert {c.stride for c in ic.CASES} == {8, 24} and {c.tight for c in ic.CASES} == {0, 1}
    assert any(c.pos and c.bounds for c in ic.CASES) and any(c.min_length for c in ic.CASES)
    assert ibd.IBD_PAIR_DTYPE.itemsize == 40 and ibd.IBD_SEGMENT_DTYPE.itemsize == 16
    # the cases have something to find, and the fuzz as well
    found = sum(int(ic.reference(c)[0]["segments1"].sum()) for c in ic.CASES)
    assert found > 60
    fuzz = [ic.fuzz_case(s) for s in ic.FUZZ_SEEDS]
    assert sum(len(ic.reference(c)[1]) for c in fuzz) > 100
    assert any(c.sites > ic.STEP for c in fuzz) and any(c.bounds and c.pos for c in fuzz)


def test_min_length_decides_both_ways():
    case = next(c for c in ic.CASES if c.name.startswith("min_length"))
    inp = ic.inputs(case)
    rows, _ = ic.reference(case)
    loose, _ = ic.naive(inp.code, case.sites, inp.index, inp.group, inp.pos, case.min_sites, 0)
    by_sites, _ = ic.naive(inp.code, case.sites, inp.index, inp.group, inp.pos, ic.MIN,
                           case.min_length)
    # (0, 1): 191 sites pass min_sites, the length fails; (2, 3): both pass; (4, 5): 146 sites
    # fail min_sites though their length would pass
    pos = inp.pos.astype(np.int64)
    assert pos[290] - pos[100] == 190 < case.min_length <= pos[446] - pos[301]
    assert [int(r["segments2"]) for r in rows[:3]] == [0, 1, 0]
    assert [int(r["segments2"]) for r in loose[:3]] == [1, 1, 0]
    assert [int(r["segments2"]) for r in by_sites[:3]] == [0, 1, 1]


def test_a_row_depends_on_its_own_pair_only():
    case = next(c for c in ic.CASES if c.name.startswith("two steps"))
    inp = ic.inputs(case)
    whole, _ = ic.run_host(case)
    args = (inp.bits(), inp.wps, case.sites)
    kw = dict(group=inp.group, pos=inp.pos, min_sites=case.min_sites, min_length=case.min_length)
    order = np.random.default_rng(3).permutation(len(inp.index))[:20]
    moved, _ = ibd.ibd_segments_raw_host(*args, np.ascontiguousarray(inp.index[order]), **kw)
    assert moved.tobytes() == whole[order].tobytes()
    # the indices swapped: everything but sample_i and sample_j is the same bytes
    swapped, _ = ibd.ibd_segments_raw_host(*args, np.ascontiguousarray(inp.index[:, ::-1]), **kw)
    assert np.array_equal(swapped["sample_i"], whole["sample_j"])
    for name in ibd.IBD_PAIR_DTYPE.names[2:]:
        assert swapped[name].tobytes() == whole[name].tobytes(), name
    assert whole["segments1"][:3].all()
    # the other stride, and the first records of a buffer
    other, _ = ibd.ibd_segments_raw_host(*args, inp.index, **kw)
    assert other.tobytes() == whole.tobytes() and case.stride == 24
    words = inp.pairs.view(np.uint32).reshape(-1, 6)
    part, _ = ibd.ibd_segments_raw_host(*args, words, num_records=5, **kw)
    assert part.tobytes() == whole[:5].tobytes()
    # the self pair: every group that satisfies the minimum is one segment of both kinds
    selfs = whole[(whole["sample_i"] == whole["sample_j"]) & (whole["sample_i"] < case.samples)]
    assert len(selfs) == 2 and (selfs["segments1"] == 1).all() and (selfs["segments2"] == 1).all()
    assert (selfs["length1"] == case.sites - 1).all() and (selfs["longest2"] == case.sites - 1).all()
    # an index outside the stored samples: zeros
    outside = whole[(whole["sample_i"] >= case.samples) | (whole["sample_j"] >= case.samples)]
    assert len(outside) == 2
    for name in ibd.IBD_PAIR_DTYPE.names[2:]:
        assert not outside[name].any()


def test_zero_sites_write_zero_rows_and_an_empty_list_is_ok():
    inp = ic.inputs(ic.REFUSAL_CASE)
    rows, segments = ibd.ibd_segments_raw_host(inp.bits(), inp.wps, 0, inp.index, segments=True)
    assert np.array_equal(rows["sample_i"], inp.index[:, 0]) and len(segments) == 0
    for name in ibd.IBD_PAIR_DTYPE.names[2:]:
        assert not rows[name].any()
    rows, segments = ibd.ibd_segments_raw_host(inp.bits(), inp.wps, ic.REFUSAL_CASE.sites,
                                               np.zeros((0, 2), dtype=np.uint32), segments=True)
    assert rows.shape == (0,) and segments.shape == (0,)
    assert ibd.ibd_segments_host(inp.bits(), inp.wps, 0, inp.index).total_length == 0


def _raw_host(inp, **over):
    """cuking_ibd_pairs_host with single arguments replaced; returns (status, out, found)."""
    out = np.full(len(inp.index) * 10, 0xABABABAB, dtype=np.uint32)
    segments = np.zeros(16, dtype=ibd.IBD_SEGMENT_DTYPE)
    found = C.c_uint64(77)
    bits, pairs = inp.bits(), np.ascontiguousarray(inp.pairs)
    pointers = dict(bits=bits.ctypes.data, group=None, pos=None, pairs=pairs.ctypes.data,
                    out=out.ctypes.data, segments=segments.ctypes.data, found=C.byref(found))
    st = _lib.load().cuking_ibd_pairs_host(*ic.raw_arguments(inp, pointers, **over))
    return st, out, found.value


@pytest.mark.parametrize("name", ic.REFUSALS)
def test_host_refusals(name):
    inp = ic.inputs(ic.REFUSAL_CASE)
    st, out, _ = _raw_host(inp, **ic.REFUSALS[name])
    assert st == _lib.ERR_INVALID_ARGUMENT, name
    assert (out == 0xABABABAB).all()
    message = _lib.load().cuking_last_error().decode()
    assert message and any(ch.isdigit() for ch in message) or "null" in message or \
        "num_segments" in message, message
    if name == "min_sites below 64":   # the message says why
        assert "63" in message and "64" in message and "word" in message, message
    st, out, found = _raw_host(inp)
    assert st == _lib.OK and found == len(ic.reference(ic.REFUSAL_CASE)[1])
    assert out.view(ibd.IBD_PAIR_DTYPE).tobytes() == ic.reference(ic.REFUSAL_CASE)[0].tobytes()
    st, out, found = _raw_host(inp, num_pairs=0, pairs=None, out=None, bits=None)
    assert st == _lib.OK and (out == 0xABABABAB).all() and found == 0


def test_positions_must_not_decrease_inside_a_group():
    case = ic.REFUSAL_CASE
    inp = ic.inputs(case)
    pos = np.arange(case.sites, dtype=np.uint32) * 3
    pos[100] = 7
    with pytest.raises(cuking_amd.CukingError, match=r"pos\[100\] = 7 follows pos\[99\] = 297") as e:
        ibd.ibd_segments_raw_host(inp.bits(), inp.wps, case.sites, inp.index, pos=pos)
    assert e.value.status == _lib.ERR_FAILED_PRECONDITION
    # a new group may start below its predecessor; the first offending site is named
    group = (np.arange(case.sites) >= 100).astype(np.int32)
    ibd.ibd_segments_raw_host(inp.bits(), inp.wps, case.sites, inp.index, pos=pos, group=group)
    pos[150], pos[160] = 1, 2
    with pytest.raises(cuking_amd.CukingError, match=r"pos\[150\] = 1 follows"):
        ibd.ibd_segments_raw_host(inp.bits(), inp.wps, case.sites, inp.index, pos=pos, group=group)


def test_the_overflow_rule():
    case = next(c for c in ic.CASES if c.name.startswith("group boundaries"))
    _, want = ic.reference(case)
    total = len(want)
    assert total >= 10
    rows, exact = ic.run_host(case, max_segments=total)
    assert ibd.sort_segments(exact).tobytes() == want.tobytes()
    with pytest.raises(cuking_amd.ResourceExhaustedError, match=f"{total} segments") as e:
        ic.run_host(case, max_segments=total - 1)
    assert e.value.num_segments == total
    with pytest.raises(cuking_amd.ResourceExhaustedError) as e:   # the counting call
        ic.run_host(case, max_segments=0)
    assert e.value.num_segments == total
    # the raw call: nothing past the buffer, every row written, the exact count
    inp = ic.inputs(case)
    out = np.zeros(len(inp.index), dtype=ibd.IBD_PAIR_DTYPE)
    segments = np.full(4 * total, 0xCDCDCDCD, dtype=np.uint32)
    found = C.c_uint64(0)
    bits, pairs = inp.bits(), np.ascontiguousarray(inp.pairs)
    st = _lib.load().cuking_ibd_pairs_host(
        bits.ctypes.data, case.samples, inp.wps, case.sites, inp.group.ctypes.data, None,
        case.min_sites, 0, pairs.ctypes.data, len(inp.index), case.stride, out.ctypes.data,
        segments.ctypes.data, 3, C.byref(found))
    assert st == _lib.ERR_RESOURCE_EXHAUSTED and found.value == total
    assert (segments[12:] == 0xCDCDCDCD).all() and (segments[:12] != 0xCDCDCDCD).any()
    assert out.tobytes() == rows.tobytes()
    # the wrapper grows its default buffer once: more than four segments per pair
    one = np.array([inp.index[0]] * 2, dtype=np.uint32)
    got = ibd.ibd_segments_host(bits, inp.wps, case.sites, one, group=inp.group,
                                min_sites=case.min_sites, segments=True)
    assert len(got.segments) == 16 > 4 * 2 and got.sorted()["pair"].tolist() == [0] * 8 + [1] * 8
    with pytest.raises(ValueError, match="segments=True"):
        ibd.ibd_segments_host(bits, inp.wps, case.sites, one).sorted()


def test_genome_length_proportions_and_relationship_on_hand_made_values():
    assert ibd.genome_length(None, None, 0) == 0 and ibd.genome_length(None, None, 100) == 99
    group = np.array([3, 3, 3, 5, 5, 3, 9], dtype=np.int32)
    pos = np.array([10, 20, 45, 7, 8, 100, 4], dtype=np.uint32)
    assert ibd.genome_length(group, None, 7) == 2 + 1 + 0 + 0
    assert ibd.genome_length(group, pos, 7) == 35 + 1
    assert ibd.genome_length(None, pos[:3], 3) == 35
    with pytest.raises(ValueError):
        ibd.genome_length(group[:3], pos, 7)
    rows = np.zeros(9, dtype=ibd.IBD_PAIR_DTYPE)
    #                 dup   po    sib   sib-edge  po-edge  2nd   3rd   unrel  nothing
    rows["length1"] = [1000, 1000, 750, 1000, 1000, 500, 250, 100, 0]
    rows["length2"] = [1000, 0, 250, 81, 80, 0, 0, 0, 0]
    got = ibd.IBDPairs(rows, 1000, None, 512, 0)
    pi1, pi2, kin = got.proportions()
    assert pi1.dtype == np.float64 and pi1.tolist() == [0, 1, 0.5, 0.919, 0.92, 0.5, 0.25, 0.1, 0]
    assert pi2.tolist() == [1, 0, 0.25, 0.081, 0.08, 0, 0, 0, 0]
    assert np.allclose(kin, [0.5, 0.25, 0.25, 0.27025, 0.27, 0.125, 0.0625, 0.025, 0], atol=1e-15)
    u, t3, t2, fs, po, dup = (pcr.UNRELATED, pcr.THIRD_DEGREE, pcr.SECOND_DEGREE,
                              pcr.FULL_SIBLING, pcr.PARENT_CHILD, pcr.DUPLICATE)
    assert got.relationship().tolist() == [dup, po, fs, fs, po, t2, t3, u, u]
    assert got.relationship().dtype == np.uint8
    assert got.relationship(sibling_ibd2=0.3).tolist()[:5] == [dup, po, po, po, po]
    assert got.relationship(thresholds=(0.01, 0.02, 0.03, 0.6)).tolist()[0] == fs
    # strict comparisons: kin equal to a cut-off is below it
    rows["length1"], rows["length2"] = 354, 354
    edge = ibd.IBDPairs(rows, 500, None, 512, 0)     # kin = 0.354
    assert edge.relationship(thresholds=(0.0442, 0.0884, 0.177, np.float32(0.354)))[0] == fs
    with pytest.raises(ValueError):
        got.relationship(thresholds=(0.1, 0.05, 0.2, 0.3))
    empty = ibd.IBDPairs(rows, 0, None, 512, 0)      # no genome: NaN, unrelated
    assert np.isnan(empty.proportions()[2]).all() and not empty.relationship().any()


def test_bim_positions_round_trip(tmp_path):
    geno = np.zeros((3, 5), dtype=np.int8)
    plink.write_plink(tmp_path / "a", geno)
    assert plink.read_bim_positions(tmp_path / "a").tolist() == [1, 2, 3, 4, 5]
    positions = [100, 250, 250, 7, 4_000_000_000]
    plink.write_plink(tmp_path / "b", geno, chromosomes=["1", "1", "1", "2", "2"],
                      positions=positions)
    got = plink.read_bim_positions(tmp_path / "b")
    assert got.dtype == np.uint32 and got.tolist() == positions
    assert plink.read_bim_chromosomes(tmp_path / "b").tolist() == [0, 0, 0, 1, 1]
    with pytest.raises(ValueError, match="positions"):
        plink.write_plink(tmp_path / "c", geno, positions=[1, 2, 3])
    with pytest.raises(ValueError, match="positions"):
        plink.write_plink(tmp_path / "c", geno, positions=[1, 2, 3, 4, -1])
    (tmp_path / "d.bim").write_text("1\tv0\t0\t12\tA\tC\n1\tv1\t0\tx\tA\tC\n")
    with pytest.raises(ValueError, match="d.bim:2"):
        plink.read_bim_positions(tmp_path / "d")


def test_host_side_under_asan_ubsan(tmp_path):
    """csrc/king_host.cc and a stand-alone driver (tests/ibd_host_driver.cc) built with
    AddressSanitizer + UBSan.  A program of its own on the CPU: nothing is loaded into Python."""
    run_sanitized_driver(tmp_path, "ibd_host_driver")


def test_the_test_encoder_is_the_library_layout():
    from site_qc_cases import pack
    rng = np.random.default_rng(5)
    code = ic.draw_codes(rng, 5, 300, missing=0.1)
    geno = np.where(code == 3, -1, code).astype(np.int8)
    bits = pack(geno)
    # (the library pads with missing: both bits set)
    assert ic.pack_codes(code, bits.shape[1] // 2, ones_padding=True).tobytes() == bits.tobytes()


# ---- the end-to-end check on the synthetic cohort ----------------------------------------------
E2E = (333, 5000, 7)   # samples, sites, seed: the cohort of smoke()


@lru_cache(maxsize=None)
def e2e_cohort():
    """(cohort, planted pairs uint32 [P, 2] with founder pairs behind them, labels)."""
    from cuking_amd.synth import plan_cohort
    n, _, seed = E2E
    cohort = plan_cohort(n, seed)
    planted = [(a, b, what) for a, b, what in cohort.planted if what in ("po", "dup")]
    others = [(k, k + 1, "none") for k in range(0, 40, 2)]
    labels = np.array([p[2] for p in planted + others])
    index = np.array([p[:2] for p in planted + others], dtype=np.uint32)
    return cohort, index, labels


def check_e2e(got, labels):
    """An IBDPairs of the end-to-end pairs: a child is one kind-1 segment with each parent, a
    duplicate one kind-2 segment; the founders share nothing at 512 sites."""
    n, m, _ = E2E
    po, dup, none = labels == "po", labels == "dup", labels == "none"
    assert po.sum() >= 6 and dup.sum() >= 1 and got.total_length == m - 1
    pi1, pi2, kin = got.proportions()
    assert (got.segments1[po] == 1).all() and (got.length1[po] == m - 1).all()
    assert (pi1[po] + pi2[po] == 1.0).all() and (pi2[po] < 0.08).all()
    assert (pi2[dup] == 1.0).all() and (got.segments2[dup] == 1).all()
    assert not got.segments1[none].any() and (kin[none] == 0).all()
    codes = got.relationship()
    assert (codes[po] == pcr.PARENT_CHILD).all() and (codes[dup] == pcr.DUPLICATE).all()
    assert (codes[none] == pcr.UNRELATED).all()


def test_end_to_end_on_the_host(oracle):
    n, m, seed = E2E
    cohort, index, labels = e2e_cohort()
    bits = oracle.synth_bitset(seed, cohort.kind, cohort.pa, cohort.pb, 0, n, m)
    wps = bits.shape[1]
    got = cuking_amd.ibd_segments_host(bits, wps, m, index)
    check_e2e(got, labels)
    # teeth: one planted genotype flipped to the opposite homozygote changes the row
    at = int(np.flatnonzero(labels == "po")[0])
    parent, child = (int(x) for x in index[at])
    row = bits[parent].copy()
    plane = wps // 2
    site = next(s for s in range(2000, m)
                if not (bits[child, s >> 6] >> np.uint64(s & 63)) & np.uint64(1)
                and not (bits[parent, s >> 6] >> np.uint64(s & 63)) & np.uint64(1))
    # (both are homozygous or missing there; make the pair (0, 2))
    flipped = bits.copy()
    bit = np.uint64(1) << np.uint64(site & 63)
    flipped[parent, plane + (site >> 6)] &= ~bit
    flipped[child, plane + (site >> 6)] |= bit
    assert not np.array_equal(flipped[parent], row) or not np.array_equal(flipped[child],
                                                                          bits[child])
    broken = cuking_amd.ibd_segments_host(flipped, wps, m, index[at:at + 1], segments=True)
    assert broken.segments1[0] == 2 and broken.length1[0] == m - 3
    assert broken.sorted()[["first_site", "last_site"]].tolist() == [(0, site - 1),
                                                                     (site + 1, m - 1)]
    assert broken.rows.tobytes() != got.rows[at:at + 1].tobytes()
