"""PCA on the GPU (the device backend: site_counts, transpose_sites and geno_matmul): the result
against the dense float64 reference at the tolerance of the reference's data, fitting on a
subset with the rest projected, agreement with the host backend, the refusals, and one run of
the driver with --pca-uri against KingContext.pca on the same bitset."""
import numpy as np
import pytest
import torch

from pca_cases import (ITERATIONS, K, SITES, bits_of_cohort, check_result, check_separation,
                       fit_mask, reference, twin_error)

import cuking_amd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device_bits():
    bits, wps = bits_of_cohort()
    return torch.from_numpy(bits.view(np.int64)).to("cuda:0"), wps


@pytest.mark.parametrize("fit", ("all", "some"))
def test_device_backend_against_the_dense_reference(ctx, device_bits, fit):
    bits, wps = device_bits
    ref = reference(fit)
    mask = None if fit == "all" else fit_mask(fit)
    got = ctx.pca(bits, wps, SITES, k=K, fit=mask, iterations=ITERATIONS)
    check_result(got, ref, twin_error(ref)[1])
    check_separation(got.scores.astype(np.float64))
    # a device mask (UnrelatedSet.keep is one) and the same bytes on a second call
    if mask is not None:
        keep = torch.from_numpy(mask.astype(np.uint8)).to("cuda:0")
        again = ctx.pca(bits, wps, SITES, k=K, fit=keep, iterations=ITERATIONS)
        assert again.scores.tobytes() == got.scores.tobytes()
        assert again.eigenvalues.tobytes() == got.eigenvalues.tobytes()
    # the host backend computes the same thing: both within the tolerance of the reference
    host = cuking_amd.pca_host(bits.cpu().numpy().view(np.uint64), wps, SITES, k=K, fit=mask,
                               iterations=ITERATIONS)
    scale = np.abs(ref.scores).max(axis=0)
    assert (np.abs(host.scores - got.scores) / scale).max() <= 2 * ref.tolerance
    assert np.array_equal(host.sites_used, got.sites_used)
    assert np.array_equal(host.allele_freq, got.allele_freq, equal_nan=True)


def test_refusals_name_the_numbers(ctx, device_bits):
    bits, wps = device_bits
    with pytest.raises(ValueError, match="k = 0"):
        ctx.pca(bits, wps, SITES, k=0)
    with pytest.raises(ValueError, match=r"60 \+ 10 = 70 exceeds min\(64, 120 fit samples\)"):
        ctx.pca(bits, wps, SITES, k=60)
    one = np.zeros(120, dtype=bool)
    one[3] = True
    with pytest.raises(ValueError, match="1 fit samples"):
        ctx.pca(bits, wps, SITES, k=1, fit=one)
    blank = torch.full((20, cuking_amd.words_per_sample(64)), -1, dtype=torch.int64, device="cuda:0")
    with pytest.raises(ValueError, match="no used site"):
        ctx.pca(blank, blank.shape[1], 64, k=2)


def test_driver_writes_the_components(ctx, tmp_path):
    """--synthetic 192,640 --synthetic-model admixed --pca-components 2: the keys and shapes of
    the .npz, and its scores against KingContext.pca on the same bitset."""
    from cuking_amd import run
    from cuking_amd.synth import cohort_to_device, plan_cohort
    n, m, seed = 192, 640, 20240229
    path = tmp_path / "pca.npz"
    assert run.main(["--synthetic", f"{n},{m}", "--synthetic-model", "admixed", "--output-uri",
                     str(tmp_path / "out"), "--pca-uri", str(path), "--pca-components", "2"]) == 0
    with np.load(path) as f:
        got = {name: f[name] for name in f.files}
    assert set(got) == {"eigenvalues", "scores", "loadings", "allele_freq", "sites_used", "fit",
                        "samples"}
    assert got["eigenvalues"].shape == (2,) and got["scores"].shape == (n, 2)
    assert got["loadings"].shape == (m, 2) and got["allele_freq"].shape == (m,)
    assert got["sites_used"].shape == (m,) and got["fit"].shape == (n,) and got["fit"].all()
    assert got["samples"].tolist() == [f"S{k:07d}" for k in range(n)]
    kind, pa, pb = cohort_to_device(plan_cohort(n, seed), 0)
    bits = ctx.synth_bitset(seed, kind, pa, pb, 0, n, m, model="admixed")
    want = ctx.pca(bits, cuking_amd.words_per_sample(m), m, k=2)
    assert want.scores.tobytes() == got["scores"].tobytes()
    assert want.eigenvalues.tobytes() == got["eigenvalues"].tobytes()
    assert want.loadings.tobytes() == got["loadings"].tobytes()
    # fitted on the unrelated set of the same run: `fit` is its `keep`, everybody is projected
    path2, unrelated = tmp_path / "pca_unrelated.npz", tmp_path / "unrelated.npz"
    assert run.main(["--synthetic", f"{n},{m}", "--synthetic-model", "admixed", "--output-uri",
                     str(tmp_path / "out2"), "--unrelated-uri", str(unrelated), "--pca-uri",
                     str(path2), "--pca-components", "2", "--pca-fit", "unrelated"]) == 0
    with np.load(path2) as f, np.load(unrelated) as u:
        fit, scores, keep = f["fit"], f["scores"], u["keep"]
    assert fit.dtype == bool and np.array_equal(fit, keep == 1) and 12 <= fit.sum() < n
    assert scores.shape == (n, 2)
    want = ctx.pca(bits, cuking_amd.words_per_sample(m), m, k=2, fit=keep == 1)
    assert want.scores.tobytes() == scores.tobytes()
    assert not np.array_equal(scores, got["scores"])
