"""PCA, CPU side (the host backend: geno_matmul_host and numpy): hwe_table against the float64
formula bit for bit, the float64 twin of the iteration against eigh, the result against the
dense reference at the tolerance of the reference's data, fitting on a subset with the rest
projected, the separation of the three populations, the refusals and the driver's usage
errors.  No GPU."""
import numpy as np
import pytest

from pca_cases import (ITERATIONS, K, MONOMORPHIC, SITES, TWIN_BOUND, bits_of_cohort,
                       check_result, check_separation, cohort, fit_mask, reference, twin_error)
from site_qc_cases import site_counts_numpy

import cuking_amd
from cuking_amd.pca import host_site_counts, hwe_table


def test_hwe_table_is_the_formula_rounded_once():
    counts = np.array([[10, 20, 30, 5], [0, 0, 0, 7], [9, 0, 0, 1], [0, 0, 8, 0], [1, 1, 0, 0],
                       [4, 4, 4, 4], [0, 3, 0, 2], [2 ** 20, 3, 5, 0]], dtype=np.uint32)
    table, used, p = hwe_table(counts, len(counts))
    assert used.tolist() == [True, False, False, False, True, True, True, True]
    assert table.dtype == np.float32 and table.shape == (8, 4)
    for row, (c, u) in enumerate(zip(counts.astype(np.int64), used)):
        called, alt = c[0] + c[1] + c[2], c[1] + 2 * c[2]
        if called == 0:
            assert np.isnan(p[row])
        else:
            assert p[row] == alt / (2.0 * called)
        if not u:
            assert (table[row] == 0).all()
            continue
        s = np.sqrt(2.0 * p[row] * (1.0 - p[row]))
        want = np.float32([(0 - 2.0 * p[row]) / s, (1 - 2.0 * p[row]) / s, (2 - 2.0 * p[row]) / s, 0])
        assert table[row].tobytes() == want.tobytes(), row
    # int32 views of uint32 counts (what the device tensors hold) and more rows than sites
    again, _, _ = hwe_table(counts.view(np.int32), 5)
    assert again.tobytes() == table[:5].tobytes()
    with pytest.raises(ValueError, match="site_counts"):
        hwe_table(counts, 9)


def test_host_site_counts_are_the_counts():
    geno, _ = cohort()
    bits, wps = bits_of_cohort()
    assert np.array_equal(host_site_counts(bits), site_counts_numpy(np.asarray(geno), wps // 2))


@pytest.mark.parametrize("fit", ("all", "some"))
def test_twin_of_the_iteration_agrees_with_eigh(fit):
    eig_err, gap = twin_error(reference(fit))
    print(f"twin at {ITERATIONS} iterations, fit {fit}: eigenvalue error {eig_err:.3g}, "
          f"subspace gap {gap:.3g}")
    assert eig_err <= TWIN_BOUND and gap <= TWIN_BOUND


@pytest.mark.parametrize("fit", ("all", "some"))
def test_host_backend_against_the_dense_reference(fit):
    bits, wps = bits_of_cohort()
    ref = reference(fit)
    got = cuking_amd.pca_host(bits, wps, SITES, k=K, fit=None if fit == "all" else fit_mask(fit),
                              iterations=ITERATIONS)
    assert isinstance(got, cuking_amd.PCAResult)
    check_result(got, ref, twin_error(ref)[1])
    check_separation(got.scores.astype(np.float64))
    assert not got.sites_used[list(MONOMORPHIC)].any()
    # the same seed gives the same bytes; another start matrix the same answer within tolerance
    again = cuking_amd.pca_host(bits, wps, SITES, k=K, fit=got.fit, iterations=ITERATIONS)
    assert again.scores.tobytes() == got.scores.tobytes()
    other = cuking_amd.pca_host(bits, wps, SITES, k=K, fit=got.fit, iterations=ITERATIONS, seed=5)
    check_result(other, ref, twin_error(ref)[1])


def test_refusals_name_the_numbers():
    bits, wps = bits_of_cohort()
    one = np.zeros(120, dtype=bool)
    one[3] = True
    with pytest.raises(ValueError, match="1 fit samples"):
        cuking_amd.pca_host(bits, wps, SITES, k=1, fit=one)
    with pytest.raises(ValueError, match="k = 0"):
        cuking_amd.pca_host(bits, wps, SITES, k=0)
    with pytest.raises(ValueError, match=r"60 \+ 10 = 70 exceeds min\(64, 120 fit samples\)"):
        cuking_amd.pca_host(bits, wps, SITES, k=60)
    few = np.arange(120) < 8
    with pytest.raises(ValueError, match=r"2 \+ 10 = 12 exceeds min\(64, 8 fit samples\)"):
        cuking_amd.pca_host(bits, wps, SITES, k=2, fit=few)
    with pytest.raises(ValueError, match="fit must hold one entry per stored sample \\(120\\)"):
        cuking_amd.pca_host(bits, wps, SITES, k=2, fit=np.ones(7, dtype=bool))
    blank = cuking_amd.new_host_bitset(cuking_amd.Submatrix(20), 64)       # all missing
    with pytest.raises(ValueError, match="no used site"):
        cuking_amd.pca_host(blank, blank.shape[1], 64, k=2)


def test_driver_usage_errors_need_no_gpu(tmp_path, capsys, monkeypatch):
    from cuking_amd import run
    base = ["--synthetic", "8,9", "--output-uri", str(tmp_path / "out")]
    pca = ["--pca-uri", str(tmp_path / "pca.npz")]
    for flags, word in ((["--pca-components", "2"], "--pca_uri"), (["--pca-fit", "all"], "--pca_uri"),
                        (pca + ["--split-factor", "3"], "--split_factor 1"),
                        (pca + ["--pca-fit", "related"], "all or unrelated"),
                        (pca + ["--pca-fit", "unrelated"], "--unrelated_uri"),
                        (pca + ["--pca_components", "0"], "at least 1")):
        assert run.main(base + flags) == 1
        err = capsys.readouterr().err
        assert "Error: INVALID_ARGUMENT" in err and word in err, err
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert run.main(base + pca) == 1
    assert "one process" in capsys.readouterr().err
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(SystemExit):
        run.parse_args(["--help"])
    text = capsys.readouterr().out
    for name in ("pca-uri", "pca_components", "pca-fit"):
        assert f"--{name}" in text, name
