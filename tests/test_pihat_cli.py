"""`python -m cuking_amd.run --pihat-uri`: every usage error (no GPU), and one small run of the
driver on a synthetic cohort whose .npz is held against KingContext.pi_hat_records on the same
bitset (GPU)."""
import numpy as np
import pytest

import cuking_amd


def test_driver_usage_errors_need_no_gpu(tmp_path, capsys, monkeypatch):
    from cuking_amd import run
    base = ["--synthetic", "8,9", "--output-uri", str(tmp_path / "out")]
    uri = ["--pihat-uri", str(tmp_path / "pihat.npz")]
    cases = (
        (["--pihat-min", "0.1"], "--pihat_min and --pihat_unbounded need --pihat_uri"),
        (["--pihat-unbounded"], "--pihat_min and --pihat_unbounded need --pihat_uri"),
        (uri + ["--split-factor", "3"], "--pihat_uri needs --split_factor 1"),
        (uri + ["--pihat-min", "nan"], "--pihat_min must not be NaN"),
    )
    for flags, word in cases:
        assert run.main(base + flags) == 1, flags
        err = capsys.readouterr().err
        assert "Error: INVALID_ARGUMENT" in err and word in err, err
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert run.main(base + uri) == 1
    assert "--pihat_uri needs one process" in capsys.readouterr().err
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(SystemExit):
        run.parse_args(["--help"])
    text = capsys.readouterr().out
    for name in ("pihat-uri", "pihat-min", "pihat-unbounded"):
        assert f"--{name}" in text, name


@pytest.mark.gpu
@pytest.mark.parametrize("flags,min_pi_hat,bounded", [
    ((), cuking_amd.pihat.DEFAULT_MIN_PI_HAT, True),
    (("--pihat-min", "0.03", "--pihat-unbounded"), 0.03, False)])
def test_driver_writes_the_records(ctx, tmp_path, flags, min_pi_hat, bounded):
    from cuking_amd import run
    from cuking_amd.synth import cohort_to_device, plan_cohort
    n, m, seed = 300, 640, 20240229
    path = tmp_path / "pihat.npz"
    assert run.main(["--synthetic", f"{n},{m}", "--output-uri", str(tmp_path / "out"),
                     "--pihat-uri", str(path), *flags]) == 0
    with np.load(path) as f:
        got = {name: f[name] for name in f.files}
    assert set(got) == {"sample_i", "sample_j", "pi_hat", "z0", "z1", "z2", "ibs0", "ibs1", "ibs2",
                        "samples", "model", "sites_used", "min_pi_hat", "bounded", "num_records"}
    count = int(got["num_records"])
    assert count > 0 and got["min_pi_hat"] == np.float32(min_pi_hat)
    assert bool(got["bounded"]) is bounded and int(got["sites_used"]) <= m
    for name in ("sample_i", "sample_j", "pi_hat", "z0", "z1", "z2", "ibs0", "ibs1", "ibs2"):
        assert got[name].shape == (count,), name
    assert (got["sample_i"] < got["sample_j"]).all() and got["sample_j"].max() < n
    order = np.lexsort((got["sample_j"], got["sample_i"]))
    assert np.array_equal(order, np.arange(count))          # sorted by (sample_i, sample_j)
    assert (got["pi_hat"] > np.float32(min_pi_hat)).all() and got["pi_hat"].dtype == np.float32
    assert got["samples"].shape == (n,) and got["model"].shape == (5,)
    # against the call the driver is made of, on the same bitset
    kind, pa, pb = cohort_to_device(plan_cohort(n, seed), 0)
    bits = ctx.synth_bitset(seed, kind, pa, pb, 0, n, m)
    wps = cuking_amd.words_per_sample(m)
    want = ctx.pi_hat_records(cuking_amd.Submatrix(n), wps, bits, m, min_pi_hat, bounded=bounded)
    rows, z = want.sorted(), want.z()
    assert count == want.num_records
    assert got["model"].tolist() == list(want.model.as_tuple()[:5])
    for name, col in (("sample_i", "sample_i"), ("sample_j", "sample_j"), ("pi_hat", "kin"),
                      ("ibs0", "ibs0"), ("ibs1", "ibs1"), ("ibs2", "ibs2")):
        assert got[name].tobytes() == np.ascontiguousarray(rows[col]).tobytes(), name
    for k, name in enumerate(("z0", "z1", "z2")):
        assert got[name].tobytes() == np.ascontiguousarray(z[:, k]).tobytes(), name
    assert (np.float32(z[:, 3]) == rows["kin"]).all()
