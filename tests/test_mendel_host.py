"""Mendelian errors without a GPU: the host twin against the naive walk of mendel_cases.py (rows,
error masks and site counts, bytewise), the disjointness of the eight masks, what the case list
covers, the chunked wrapper, per_sample, candidate_trios on a hand-built pedigree,
read_fam_parents on written .fam files, the refusals with their messages and the stand-alone
sanitizer driver."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import mendel_cases as mc
from host_driver import run_sanitized_driver

import cuking_amd
from cuking_amd import _lib, mendel, pcrelate, plink
from cuking_amd.mendel import NO_PARENT


@pytest.mark.parametrize("case", mc.CASES, ids=lambda c: c.name)
def test_host_twin_equals_the_naive_walk(case):
    got = mc.run_host(case)
    mc.check_against(case, *got, "host twin")
    # all-ones padding beyond num_sites: the same bytes
    mc.check_against(case, *mc.run_host(case, ones_padding=True), "host twin, ones padding")


@pytest.mark.parametrize("seed", mc.FUZZ_SEEDS)
def test_host_twin_fuzz(seed):
    case = mc.fuzz_case(seed)
    mc.check_against(case, *mc.run_host(case), "host twin")
    mc.check_against(case, *mc.run_host(case, ones_padding=True), "host twin, ones padding")


def test_the_case_list_covers_the_table():
    """The minimum counts below were fixed after running the naive reference on the CPU: over
    the case list the full trios show between 1952 (code 2) and 9512 (code 4) errors of each of
    the eight codes, the duos with a father 7157 and 6920 of codes 3 and 6, the duos with a mother
    9031 and 8949 of codes 4 and 7, and no duo shows any other code; the 30 fuzz seeds between
    1532 and 6030 per code in full trios and between 4465 and 4614 per possible code in duos."""
    assert mc.STEP == 64 * 64 and mc.SITE_COUNTS <= {c.sites for c in mc.CASES}
    assert max(c.samples for c in mc.CASES) <= 24 and max(c.trios for c in mc.CASES) <= 20
    assert all(len(mc.inputs(c).trios) <= 20 for c in mc.CASES)
    assert {c.kind for c in mc.CASES} == {"random", "rows", "family", "planted"}
    assert any(c.extra for c in mc.CASES)
    fuzz = [mc.fuzz_case(s) for s in mc.FUZZ_SEEDS]
    assert max(c.samples for c in fuzz) <= 24 and max(c.trios for c in fuzz) <= 20
    for cases, least_full, least_duo in ((mc.CASES, 1500, 5000), (fuzz, 1000, 3000)):
        full, father, mother = mc.form_counts(cases)
        print("full", full.tolist(), "father", father.tolist(), "mother", mother.tolist())
        assert (full >= least_full).all()
        assert (father[[2, 5]] >= least_duo).all() and not father[[0, 1, 3, 4, 6, 7]].any()
        assert (mother[[3, 6]] >= least_duo).all() and not mother[[0, 1, 2, 4, 5, 7]].any()


def test_the_reference_reads_the_table():
    """One genotype triple per code by hand, and the triples without an error."""
    for k, (f, m, c) in enumerate(mc.PLANT_GENOTYPES):
        assert mc.classify(f, m, c) == k + 1
    R, H, V, N = mc.R, mc.H, mc.V, mc.MISSING
    assert mc.classify(N, N, R) == mc.classify(N, N, V) == mc.classify(N, N, H) == 0
    assert mc.classify(V, N, R) == 3 and mc.classify(N, V, R) == 4
    assert mc.classify(R, N, V) == 6 and mc.classify(N, R, V) == 7
    assert mc.classify(R, R, N) == mc.classify(V, V, N) == 0
    assert mc.classify(H, H, R) == mc.classify(H, H, H) == mc.classify(H, H, V) == 0
    assert mc.classify(R, V, H) == mc.classify(V, R, H) == 0 and mc.classify(R, N, H) == 0
    assert sum(bool(mc.classify(f, m, c)) for f in range(4) for m in range(4)
               for c in range(4)) == 2 + 14     # (het children: 2; homozygous children: 7 each)


@pytest.mark.parametrize("case", [c for c in mc.CASES if c.kind in ("family", "planted")],
                         ids=lambda c: c.name)
def test_transmission_gives_no_error_and_planted_errors_are_found(case):
    rows, mask, counts = mc.run_host(case)
    if case.kind == "family":
        assert not rows["errors"].any() and not mask.any() and not counts.any()
        assert (rows["called"] > 0.85 * case.sites).all()
        return
    planted = mc.planted_sites(case)
    row = rows[mc.PLANTED_TRIO]
    want = np.bincount(list(planted.values()), minlength=9)[1:]
    assert row["errors"].tolist() == want.tolist() and want.sum() == len(planted)
    sites = np.flatnonzero(np.unpackbits(mask[mc.PLANTED_TRIO].view(np.uint8), bitorder="little"))
    assert sites.tolist() == sorted(planted)
    # the two duos of the same child: a father shows 3 and 6 only, a mother 4 and 7 only
    father_duo, mother_duo = rows[3], rows[4]
    assert (father_duo["child"], father_duo["mother"]) == (row["child"], NO_PARENT)
    assert not father_duo["errors"][[0, 1, 3, 4, 6, 7]].any()
    assert not mother_duo["errors"][[0, 1, 2, 4, 5, 7]].any()
    assert father_duo["errors"][2] == want[2] + want[4] and \
        father_duo["errors"][5] == want[5] + want[7]
    assert mother_duo["errors"][3] == want[3] + want[4] and \
        mother_duo["errors"][6] == want[6] + want[7]
    # the other family is untouched
    assert not rows["errors"][[1, 2, 5, 6]].any()


def test_the_eight_masks_are_disjoint():
    """mendel_code_masks through the host twin on random words: every site has at most one code,
    so the population count of the error mask is the sum of the eight counts."""
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 1 << 64, size=(9, 2 * 40), dtype=np.uint64)
    trios = rng.integers(0, 9, size=(60, 3)).astype(np.uint32)
    trios[::7, 1] = NO_PARENT
    trios[::5, 2] = NO_PARENT
    for sites in (40 * 64, 40 * 64 - 17):
        rows, mask = mendel.mendel_errors_raw_host(bits, 80, sites, trios, error_bits=True)
        in_mask = np.unpackbits(mask.view(np.uint8), axis=1).sum(axis=1)
        assert in_mask.tolist() == rows["errors"].sum(axis=1).tolist() and in_mask.sum() > 10000


def test_the_wrapper_and_its_chunks():
    case = next(c for c in mc.CASES if c.name == "24 samples, 20 trios")
    inp = mc.inputs(case)
    want_rows, _, want_counts = mc.reference(case)
    whole = cuking_amd.mendel_errors_host(inp.bits(), inp.wps, case.sites, inp.trios,
                                          site_counts=True)
    assert isinstance(whole, cuking_amd.MendelErrors)
    assert whole.rows.dtype == cuking_amd.MENDEL_TRIO_DTYPE
    assert whole.rows.tobytes() == want_rows.tobytes()
    assert whole.site_errors.dtype == np.uint32 and whole.site_errors.shape == (case.sites,)
    assert whole.site_errors.tobytes() == want_counts[:case.sites].tobytes()
    for chunk in (1, 7, 20, 1000):
        got = cuking_amd.mendel_errors_host(inp.bits(), inp.wps, case.sites, inp.trios,
                                            site_counts=True, _chunk_trios=chunk)
        assert got.rows.tobytes() == whole.rows.tobytes()
        assert got.site_errors.tobytes() == whole.site_errors.tobytes()
    rows_only = cuking_amd.mendel_errors_host(inp.bits(), inp.wps, case.sites, inp.trios)
    assert rows_only.site_errors is None and rows_only.rows.tobytes() == want_rows.tobytes()
    assert whole.errors.shape == (20, 8) and whole.total().tolist() == \
        want_rows["errors"].sum(axis=1).tolist()
    assert whole.site_errors.sum() == whole.total().sum()
    # the default chunk keeps the mask within 64 MB
    assert mendel._chunk_rows(1564, None) * 1564 * 8 <= mendel.MASK_BYTES == 64 << 20
    assert mendel._chunk_rows(1 << 30, None) == 1


def test_total_rate_and_per_sample_on_hand_made_rows():
    rows = np.zeros(4, dtype=mendel.MENDEL_TRIO_DTYPE)
    rows["child"], rows["father"], rows["mother"] = [4, 5, 4, 9], [0, 0, NO_PARENT, 1], \
        [1, 2, 1, NO_PARENT]
    rows["called"] = [100, 0, 50, 10]
    rows["errors"] = [[1, 2, 3, 4, 5, 6, 7, 8], [0] * 8, [0, 0, 0, 10, 0, 0, 20, 0],
                      [0, 0, 5, 0, 0, 1, 0, 0]]
    got = mendel.MendelErrors(rows)
    assert got.total().tolist() == [36, 0, 30, 6]
    rate = got.rate()
    assert rate.dtype == np.float64 and np.isnan(rate[1])
    assert rate[[0, 2, 3]].tolist() == [36 / 100, 30 / 50, 6 / 10]
    # codes 1, 2, 5, 8: everyone; 3, 6: child and father; 4, 7: child and mother
    everyone, with_father, with_mother = 1 + 2 + 5 + 8, 3 + 6, 4 + 7
    per = got.per_sample(10)
    assert per.dtype == np.int64 and per.shape == (10,)
    assert per[4] == 36 + 30 and per[9] == 6 and per[5] == 0
    assert per[0] == everyone + with_father
    assert per[1] == everyone + with_mother + 30 + 6    # mother of rows 0 and 2, father of row 3
    assert per[2] == 0 and per[[3, 6, 7, 8]].tolist() == [0, 0, 0, 0]
    # samples beyond num_samples are left out
    assert got.per_sample(5).tolist() == per[:5].tolist()


def test_trios_from_parents():
    parents = np.array([[-1, -1], [-1, -1], [0, 1], [0, -1], [-1, 1], [-1, -1]])
    got = cuking_amd.trios_from_parents(parents)
    assert got.dtype == np.uint32
    assert got.tolist() == [[2, 0, 1], [3, 0, NO_PARENT], [4, NO_PARENT, 1]]
    assert cuking_amd.NO_PARENT == 0xFFFFFFFF
    assert cuking_amd.trios_from_parents(np.zeros((0, 2), dtype=np.int64)).shape == (0, 3)
    with pytest.raises(ValueError, match=r"\[n, 2\]"):
        cuking_amd.trios_from_parents(np.zeros((3, 3), dtype=np.int64))
    with pytest.raises(ValueError, match="-1"):
        cuking_amd.trios_from_parents(np.array([[-2, 0]]))


# ---- candidate_trios ------------------------------------------------------------------------------
PC, FS, D2, D3 = (pcrelate.PARENT_CHILD, pcrelate.FULL_SIBLING, pcrelate.SECOND_DEGREE,
                  pcrelate.THIRD_DEGREE)
# A pedigree by hand:
#   0 x 1 -> 2, 3                    a trio with two full siblings
#   4 x 5 -> 6;  4 x 7 -> 8          half siblings 6 and 8 through 4
#   9 x 10 -> 11;  11 x 12 -> 13;  13 x 14 -> 15     three generations below 9 x 10
PEDIGREE = [
    (0, 2, PC), (1, 2, PC), (0, 3, PC), (1, 3, PC), (2, 3, FS),
    (4, 6, PC), (5, 6, PC), (4, 8, PC), (7, 8, PC), (6, 8, D2),
    (9, 11, PC), (10, 11, PC), (11, 13, PC), (12, 13, PC), (13, 15, PC), (14, 15, PC),
    (9, 13, D2), (10, 13, D2), (11, 15, D2), (12, 15, D2), (9, 15, D3), (10, 15, D3),
]
PEDIGREE_TRIOS = [[2, 0, 1], [3, 0, 1], [6, 4, 5], [8, 4, 7], [11, 9, 10], [13, 11, 12],
                  [15, 13, 14]]


def test_candidate_trios_on_a_pedigree():
    pairs = np.array([(i, j) for i, j, _ in PEDIGREE], dtype=np.uint32)
    codes = np.array([c for _, _, c in PEDIGREE], dtype=np.uint8)
    got = cuking_amd.candidate_trios(pairs, codes)
    assert got.dtype == np.uint32 and got.tolist() == PEDIGREE_TRIOS
    # neither the order of the pairs, nor the order inside a pair, nor repeats matter
    rng = np.random.default_rng(2)
    for _ in range(5):
        order = rng.permutation(np.concatenate([np.arange(len(pairs)), np.arange(0, 9)]))
        shuffled = pairs[order].copy()
        flip = rng.random(len(order)) < 0.5
        shuffled[flip] = shuffled[flip][:, ::-1]
        again = cuking_amd.candidate_trios(shuffled, codes[order])
        assert again.tobytes() == got.tobytes()
    # `related` decides who may be a couple: without the sibling and grandparent pairs a parent
    # and its two children, or a grandparent and a grandchild's other parent, would pass
    only_pc = pairs[codes == PC]
    loose = cuking_amd.candidate_trios(pairs, codes, related=only_pc)
    assert [0, 2, 3] in loose.tolist() and [11, 9, 13] in loose.tolist()
    assert {tuple(t) for t in PEDIGREE_TRIOS} < {tuple(t) for t in loose.tolist()}
    # no pair, and no parent-child pair
    assert cuking_amd.candidate_trios(np.zeros((0, 2), dtype=np.uint32), []).shape == (0, 3)
    assert cuking_amd.candidate_trios(pairs, np.full(len(pairs), D2)).shape == (0, 3)
    with pytest.raises(ValueError, match="relationship codes"):
        cuking_amd.candidate_trios(pairs, codes[:-1])
    assert "mendel_errors" in cuking_amd.candidate_trios.__doc__


# ---- read_fam_parents ------------------------------------------------------------------------------
def write_fam(path, lines):
    Path(str(path) + ".fam").write_text("".join(line + "\n" for line in lines))


def test_read_fam_parents(tmp_path):
    # distinct IIDs: matched by IID, whatever the FID; "0" and an id that is not in the file
    write_fam(tmp_path / "a", ["F1 dad 0 0 1 -9", "F1 mum 0 0 2 -9", "F1 kid dad mum 1 -9",
                               "F2 solo 0 ghost 1 -9", "F2 half 0 mum 2 -9", "",
                               "F3 far dad nobody 0 -9"])
    got = plink.read_fam_parents(tmp_path / "a")
    assert got.dtype == np.int64
    assert got.tolist() == [[-1, -1], [-1, -1], [0, 1], [-1, -1], [-1, 1], [0, -1]]
    assert plink.read_fam(tmp_path / "a") == ["dad", "mum", "kid", "solo", "half", "far"]
    assert cuking_amd.trios_from_parents(got).tolist() == \
        [[2, 0, 1], [4, NO_PARENT, 1], [5, 0, NO_PARENT]]
    # repeated IIDs across FIDs: matched within the FID
    write_fam(tmp_path / "b", ["F1 1 0 0 1 -9", "F1 2 0 0 2 -9", "F1 3 1 2 1 -9",
                               "F2 1 0 0 1 -9", "F2 2 0 0 2 -9", "F2 3 1 2 1 -9",
                               "F3 3 1 2 1 -9"])
    got = plink.read_fam_parents(tmp_path / "b")
    assert got.tolist() == [[-1, -1], [-1, -1], [0, 1], [-1, -1], [-1, -1], [3, 4], [-1, -1]]
    assert plink.read_fam(tmp_path / "b")[5] == "F2_3"
    # no parent at all, a short line, ids that are not distinct
    write_fam(tmp_path / "c", ["F1 a 0 0 1 -9", "F1 b 0 0 1 -9"])
    assert plink.read_fam_parents(tmp_path / "c").tolist() == [[-1, -1], [-1, -1]]
    assert len(cuking_amd.trios_from_parents(plink.read_fam_parents(tmp_path / "c"))) == 0
    write_fam(tmp_path / "d", ["F1 a 0"])
    with pytest.raises(ValueError, match="father"):
        plink.read_fam_parents(tmp_path / "d")
    write_fam(tmp_path / "e", ["F1 a 0 0 1 -9", "F1 a 0 0 1 -9"])
    with pytest.raises(ValueError, match="not distinct"):
        plink.read_fam_parents(tmp_path / "e")


# ---- refusals ------------------------------------------------------------------------------------
def raw_trios(inp, **over):
    """cuking_mendel_trios_host with single arguments replaced: (status, out, error_bits)."""
    out = np.full(len(inp.trios) * 12, 0xABABABAB, dtype=np.uint32)
    mask = np.full((len(inp.trios), inp.plane), 0xCDCDCDCD, dtype=np.uint64)
    bits = inp.bits()
    pointers = dict(bits=bits.ctypes.data, trios=inp.trios.ctypes.data, out=out.ctypes.data,
                    error_bits=mask.ctypes.data)
    st = _lib.load().cuking_mendel_trios_host(*mc.trio_arguments(inp, pointers, **over))
    return st, out, mask


def raw_sites(inp, mask, **over):
    counts = np.full(64 * inp.plane, 7, dtype=np.uint32)
    pointers = dict(error_bits=mask.ctypes.data, counts=counts.ctypes.data)
    st = _lib.load().cuking_mendel_site_counts_host(*mc.site_arguments(inp, pointers, **over))
    return st, counts


@pytest.mark.parametrize("name", mc.TRIO_REFUSALS)
def test_every_refusal_with_its_message(name):
    over, word = mc.TRIO_REFUSALS[name]
    st, out, mask = raw_trios(mc.inputs(mc.REFUSAL_CASE), **over)
    assert st == _lib.ERR_INVALID_ARGUMENT, name
    assert (out == 0xABABABAB).all() and (mask == 0xCDCDCDCD).all()
    message = _lib.load().cuking_last_error().decode()
    assert word in message, message


@pytest.mark.parametrize("name", mc.SITE_REFUSALS)
def test_every_site_count_refusal_with_its_message(name):
    over, word = mc.SITE_REFUSALS[name]
    inp = mc.inputs(mc.REFUSAL_CASE)
    st, counts = raw_sites(inp, mc.reference(mc.REFUSAL_CASE)[1], **over)
    assert st == _lib.ERR_INVALID_ARGUMENT, name
    assert (counts == 7).all()
    message = _lib.load().cuking_last_error().decode()
    assert message.startswith("mendel site counts") and word in message, message


def test_the_raw_calls_and_the_calls_without_work():
    inp = mc.inputs(mc.REFUSAL_CASE)
    want = mc.reference(mc.REFUSAL_CASE)
    st, out, mask = raw_trios(inp)
    assert st == _lib.OK and out.view(mendel.MENDEL_TRIO_DTYPE).tobytes() == want[0].tobytes()
    assert mask.tobytes() == want[1].tobytes() and want[0]["errors"].sum() > 0
    # the site counts ADD: twice the call is twice the counts on top of what was there
    st, counts = raw_sites(inp, mask)
    assert st == _lib.OK and (counts - 7).tobytes() == want[2].tobytes()
    again = mendel.site_counts_host(mask, mendel.site_counts_host(mask))
    assert again.tolist() == (2 * want[2]).tolist()
    # without the mask: the same rows
    st, out, mask = raw_trios(inp, error_bits=None)
    assert st == _lib.OK and out.view(mendel.MENDEL_TRIO_DTYPE).tobytes() == want[0].tobytes()
    assert (mask == 0xCDCDCDCD).all()
    # no trio: no work, whatever the pointers; no site: zero rows with the indices echoed
    st, out, mask = raw_trios(inp, num_trios=0, trios=None, out=None, bits=None, error_bits=None)
    assert st == _lib.OK and (out == 0xABABABAB).all()
    st, counts = raw_sites(inp, mask, num_trios=0, error_bits=None, counts=None)
    assert st == _lib.OK and (counts == 7).all()
    rows, mask = mendel.mendel_errors_raw_host(inp.bits(), inp.wps, 0, inp.trios, error_bits=True)
    assert rows["child"].tolist() == inp.trios[:, 0].tolist() and not rows["called"].any()
    assert not rows["errors"].any() and not mask.any()
    assert len(mendel.mendel_errors_raw_host(inp.bits(), inp.wps, 180, [])[0]) == 0
    assert np.isnan(cuking_amd.mendel_errors_host(inp.bits(), inp.wps, 0, inp.trios).rate()).all()


def test_the_wrappers_refuse_too():
    inp = mc.inputs(mc.REFUSAL_CASE)
    args = (inp.bits(), inp.wps, mc.REFUSAL_CASE.sites)
    with pytest.raises(ValueError, match=r"\[T, 3\]"):
        mendel.mendel_errors_raw_host(*args, np.zeros((2, 2), dtype=np.uint32))
    with pytest.raises(ValueError, match="uint32"):
        mendel.mendel_errors_raw_host(*args, [[0, -1, 1]])
    with pytest.raises(ValueError, match=r"\[T, 3\]"):
        mendel.mendel_errors_raw_host(*args, np.zeros((2, 3)))
    with pytest.raises(cuking_amd.CukingError, match="do not fit"):
        mendel.mendel_errors_raw_host(inp.bits(), inp.wps, 193, inp.trios)
    with pytest.raises(ValueError, match="_chunk_trios"):
        cuking_amd.mendel_errors_host(*args, inp.trios, site_counts=True, _chunk_trios=0)


def test_host_side_under_asan_ubsan(tmp_path):
    """csrc/king_host.cc and a stand-alone driver (tests/mendel_host_driver.cc) built with
    AddressSanitizer + UBSan.  A program of its own on the CPU: nothing is loaded into Python."""
    run_sanitized_driver(tmp_path, "mendel_host_driver")
