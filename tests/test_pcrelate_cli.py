"""`python -m cuking_amd.run --pcrelate-uri`: every usage error (no GPU), and one run of the
driver on a synthetic admixed cohort against KingContext.pca -> KingContext.pcrelate on the same
bitset (GPU)."""
import numpy as np
import pytest

import cuking_amd


def test_driver_usage_errors_need_no_gpu(tmp_path, capsys, monkeypatch):
    from cuking_amd import run
    base = ["--synthetic", "8,9", "--output-uri", str(tmp_path / "out")]
    pca = ["--pca-uri", str(tmp_path / "pca.npz")]
    rel = pca + ["--pcrelate-uri", str(tmp_path / "kin.npy")]
    cases = (
        (["--pcrelate-components", "2"], "--pcrelate_uri"),
        (["--pcrelate-min-maf", "0.02"], "--pcrelate_uri"),
        (["--pcrelate-uri", str(tmp_path / "kin.npy")], "--pca_uri"),
        (rel + ["--split-factor", "3"], "--split_factor 1"),
        (rel + ["--pcrelate-components", "0"], "between 1 and --pca_components (10)"),
        (rel + ["--pca-components", "3", "--pcrelate-components", "4"],
         "between 1 and --pca_components (3)"),
        (rel + ["--pca-components", "40"], "at most 31"),
        (rel + ["--pcrelate-min-maf", "0.5"], "[0, 0.5)"),
        (rel + ["--pcrelate-min-maf", "-0.1"], "[0, 0.5)"),
        (rel + ["--pcrelate-min-maf", "nan"], "[0, 0.5)"),
    )
    for flags, word in cases:
        assert run.main(base + flags) == 1, flags
        err = capsys.readouterr().err
        assert "Error: INVALID_ARGUMENT" in err and word in err, err
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert run.main(base + rel) == 1
    assert "one process" in capsys.readouterr().err
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(SystemExit):
        run.parse_args(["--help"])
    text = capsys.readouterr().out
    for name in ("pcrelate-uri", "pcrelate_components", "pcrelate-min-maf"):
        assert f"--{name}" in text, name


@pytest.mark.gpu
def test_driver_writes_the_whole_cohort_matrix(ctx, tmp_path):
    import torch
    from cuking_amd import run
    from cuking_amd.synth import cohort_to_device, plan_cohort
    n, m, seed = 300, 640, 20240229
    path, pca_path = tmp_path / "kin.npy", tmp_path / "pca.npz"
    assert run.main(["--synthetic", f"{n},{m}", "--synthetic-model", "admixed", "--output-uri",
                     str(tmp_path / "out"), "--pca-uri", str(pca_path), "--pca-components", "3",
                     "--pcrelate-uri", str(path), "--pcrelate-components", "2",
                     "--pcrelate-min-maf", "0.02"]) == 0
    kin = np.load(path)
    assert kin.dtype == np.float32 and kin.shape == (n, n)
    assert np.array_equal(kin.view(np.uint32), kin.view(np.uint32).T)   # bytewise symmetric
    assert np.isfinite(kin).all()
    kind, pa, pb = cohort_to_device(plan_cohort(n, seed), 0)
    bits = ctx.synth_bitset(seed, kind, pa, pb, 0, n, m, model="admixed")
    wps = cuking_amd.words_per_sample(m)
    pca = ctx.pca(bits, wps, m, k=3)
    with np.load(pca_path) as f:
        assert f["scores"].tobytes() == pca.scores.tobytes()
    want = ctx.pcrelate(bits, wps, m, np.ascontiguousarray(pca.scores[:, :2]), fit=pca.fit,
                        min_maf=0.02)
    torch.cuda.synchronize()
    assert want.kin.cpu().numpy().tobytes() == kin.tobytes()
    # the diagonal is an entry like any other: a sample's kinship with itself is near 0.5
    assert np.abs(np.median(np.diagonal(kin)) - 0.5) < 0.1
