"""`python -m cuking_amd.run --pcrelate-records-uri`: every usage error (no GPU), and one small
run of the driver on a synthetic admixed cohort whose .npz is held against KingContext.pca ->
KingContext.pcrelate_records -> KingContext.pcrelate_pairs on the same bitset (GPU)."""
import numpy as np
import pytest

import cuking_amd


def test_driver_usage_errors_need_no_gpu(tmp_path, capsys, monkeypatch):
    from cuking_amd import run
    base = ["--synthetic", "8,9", "--output-uri", str(tmp_path / "out")]
    pca = ["--pca-uri", str(tmp_path / "pca.npz")]
    rel = pca + ["--pcrelate-records-uri", str(tmp_path / "rel.npz")]
    cases = (
        (["--pcrelate-min-kinship", "0.1"], "--pcrelate_min_kinship needs --pcrelate_records_uri"),
        (pca + ["--pcrelate-min-kinship", "0.1"], "--pcrelate_records_uri"),
        (["--pcrelate-records-uri", str(tmp_path / "rel.npz")], "--pca_uri"),
        (rel + ["--split-factor", "3"], "--split_factor 1"),
        (rel + ["--pcrelate-min-kinship", "nan"], "must not be NaN"),
        (rel + ["--pcrelate-components", "0"], "between 1 and --pca_components (10)"),
        (rel + ["--pca-components", "3", "--pcrelate-components", "4"],
         "between 1 and --pca_components (3)"),
        (rel + ["--pca-components", "40"], "at most 31"),
        (rel + ["--pcrelate-min-maf", "0.5"], "[0, 0.5)"),
    )
    for flags, word in cases:
        assert run.main(base + flags) == 1, flags
        err = capsys.readouterr().err
        assert "Error: INVALID_ARGUMENT" in err and word in err, err
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert run.main(base + ["--pcrelate-records-uri", str(tmp_path / "rel.npz")]) == 1
    assert "--pcrelate_records_uri needs one process" in capsys.readouterr().err
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(SystemExit):
        run.parse_args(["--help"])
    text = capsys.readouterr().out
    for name in ("pcrelate-records-uri", "pcrelate-min-kinship"):
        assert f"--{name}" in text, name


@pytest.mark.gpu
def test_driver_writes_the_records_and_their_pairs(ctx, tmp_path):
    from cuking_amd import pcrelate as pcr
    from cuking_amd import run
    from cuking_amd.synth import cohort_to_device, plan_cohort
    n, m, seed = 300, 640, 20240229
    path, pca_path = tmp_path / "rel.npz", tmp_path / "pca.npz"
    assert run.main(["--synthetic", f"{n},{m}", "--synthetic-model", "admixed", "--output-uri",
                     str(tmp_path / "out"), "--pca-uri", str(pca_path), "--pca-components", "3",
                     "--pcrelate-records-uri", str(path), "--pcrelate-components", "2",
                     "--pcrelate-min-maf", "0.02", "--pcrelate-min-kinship", "0.0884"]) == 0
    with np.load(path) as f:
        got = {name: f[name] for name in f.files}
    assert set(got) == {"sample_i", "sample_j", "kin", "k0", "k1", "k2", "ibs0", "sites",
                        "kin_pairs", "relationship", "samples", "min_kinship", "num_records"}
    count = int(got["num_records"])
    assert count > 0 and got["min_kinship"] == np.float32(0.0884)
    for name in ("sample_i", "sample_j", "kin", "k0", "k1", "k2", "ibs0", "sites", "kin_pairs",
                 "relationship"):
        assert got[name].shape == (count,), name
    assert (got["sample_i"] < got["sample_j"]).all() and got["sample_j"].max() < n
    order = np.lexsort((got["sample_j"], got["sample_i"]))
    assert np.array_equal(order, np.arange(count))          # sorted by (sample_i, sample_j)
    assert (got["kin"] > np.float32(0.0884)).all()
    assert got["relationship"].dtype == np.uint8 and got["relationship"].max() <= pcr.DUPLICATE
    assert got["samples"].shape == (n,) and got["samples"][0] == "S0000000"
    # against the calls the driver is made of, on the same bitset
    kind, pa, pb = cohort_to_device(plan_cohort(n, seed), 0)
    bits = ctx.synth_bitset(seed, kind, pa, pb, 0, n, m, model="admixed")
    wps = cuking_amd.words_per_sample(m)
    pca = ctx.pca(bits, wps, m, k=3)
    want = ctx.pcrelate_records(bits, wps, m, scores=np.ascontiguousarray(pca.scores[:, :2]),
                                fit=pca.fit, min_maf=0.02, min_kinship=0.0884)
    rows = want.sorted()
    assert want.num_records == count
    assert np.array_equal(got["sample_i"], rows["sample_i"])
    assert np.array_equal(got["sample_j"], rows["sample_j"])
    assert got["kin"].tobytes() == rows["kin"].tobytes()
    pairs = ctx.pcrelate_pairs(bits, wps, m, rows, model=want, min_maf=0.02)
    for name, field in (("kin_pairs", "kin"), ("k0", "k0"), ("k1", "k1"), ("k2", "k2"),
                        ("ibs0", "ibs0"), ("sites", "sites")):
        assert got[name].tobytes() == getattr(pairs, field).tobytes(), name
    assert got["relationship"].tobytes() == pairs.relationship().tobytes()
