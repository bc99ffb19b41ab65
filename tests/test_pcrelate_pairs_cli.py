"""`python -m cuking_amd.run --pcrelate-pairs-uri`: every usage error (no GPU), and one run of the
driver on a synthetic admixed cohort against KingContext.pca -> KingContext.pcrelate_pairs on the
same bitset and records (GPU)."""
import numpy as np
import pytest

import cuking_amd


def test_driver_usage_errors_need_no_gpu(tmp_path, capsys, monkeypatch):
    from cuking_amd import run
    base = ["--synthetic", "8,9", "--output-uri", str(tmp_path / "out")]
    pca = ["--pca-uri", str(tmp_path / "pca.npz")]
    rel = pca + ["--pcrelate-pairs-uri", str(tmp_path / "pairs.npz")]
    cases = (
        (["--pcrelate-components", "2"], "--pcrelate_uri or --pcrelate_pairs_uri"),
        (["--pcrelate-min-maf", "0.02"], "--pcrelate_uri or --pcrelate_pairs_uri"),
        (["--pcrelate-pairs-uri", str(tmp_path / "pairs.npz")], "--pca_uri"),
        (rel + ["--split-factor", "3"], "--split_factor 1"),
        (rel + ["--pcrelate-components", "0"], "between 1 and --pca_components (10)"),
        (rel + ["--pca-components", "3", "--pcrelate-components", "4"],
         "between 1 and --pca_components (3)"),
        (rel + ["--pca-components", "40"], "at most 31"),
        (rel + ["--pcrelate-min-maf", "0.5"], "[0, 0.5)"),
        (rel + ["--pcrelate-min-maf", "nan"], "[0, 0.5)"),
    )
    for flags, word in cases:
        assert run.main(base + flags) == 1, flags
        err = capsys.readouterr().err
        assert "Error: INVALID_ARGUMENT" in err and word in err, err
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert run.main(base + rel) == 1
    assert "one process" in capsys.readouterr().err
    assert run.main(base + ["--pcrelate-pairs-uri", str(tmp_path / "pairs.npz")]) == 1
    assert "--pcrelate_pairs_uri needs one process" in capsys.readouterr().err
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(SystemExit):
        run.parse_args(["--help"])
    text = capsys.readouterr().out
    for name in ("pcrelate-pairs-uri", "pcrelate_components", "pcrelate-min-maf"):
        assert f"--{name}" in text, name


@pytest.mark.gpu
def test_driver_rescores_its_records(ctx, tmp_path):
    from cuking_amd import pcrelate as pcr
    from cuking_amd import run
    from cuking_amd.synth import cohort_to_device, plan_cohort
    n, m, seed = 300, 640, 20240229
    path, pca_path = tmp_path / "pairs.npz", tmp_path / "pca.npz"
    assert run.main(["--synthetic", f"{n},{m}", "--synthetic-model", "admixed", "--output-uri",
                     str(tmp_path / "out"), "--pca-uri", str(pca_path), "--pca-components", "3",
                     "--pcrelate-pairs-uri", str(path), "--pcrelate-components", "2",
                     "--pcrelate-min-maf", "0.02", "--kin-threshold", "0.0884"]) == 0
    kind, pa, pb = cohort_to_device(plan_cohort(n, seed), 0)
    bits = ctx.synth_bitset(seed, kind, pa, pb, 0, n, m, model="admixed")
    wps = cuking_amd.words_per_sample(m)
    recs = ctx.run(cuking_amd.Submatrix(n), wps, bits, 0.0884, 10 << 20)
    pca = ctx.pca(bits, wps, m, k=3)
    want = ctx.pcrelate_pairs(bits, wps, m, recs, fit=pca.fit, min_maf=0.02,
                              scores=np.ascontiguousarray(pca.scores[:, :2]))
    with np.load(path) as f:
        assert len(recs) > 0 and f["kin"].shape == (len(recs),)
        got = {name: f[name] for name in f.files}
    # (the driver's records are the same set; both lists are in the order they were produced)
    assert sorted(zip(got["sample_i"], got["sample_j"])) == sorted(zip(want.sample_i,
                                                                       want.sample_j))
    at = {(int(i), int(j)): k for k, (i, j) in enumerate(zip(want.sample_i, want.sample_j))}
    order = np.array([at[(int(i), int(j))] for i, j in zip(got["sample_i"], got["sample_j"])])
    for name in ("kin", "k0", "k1", "k2", "ibs0", "sites"):
        assert got[name].tobytes() == getattr(want, name)[order].tobytes(), name
    assert got["relationship"].tobytes() == want.relationship()[order].tobytes()
    assert got["relationship"].dtype == np.uint8 and got["relationship"].max() <= pcr.DUPLICATE
    assert got["inbreeding"].tobytes() == want.inbreeding.tobytes()
    assert got["samples"].shape == (n,) and got["samples"][0] == "S0000000"
