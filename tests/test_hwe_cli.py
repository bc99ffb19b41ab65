"""`python -m cuking_amd.run --site-hwe-p`: the usage errors and the help text (no GPU), and the
driver on `--synthetic` with the site QC report, whose p-values must be the host twin's on the
report's own site counts (GPU)."""
import numpy as np
import pytest

import cuking_amd

import hwe_cases as hc


def test_driver_usage_errors_need_no_gpu(tmp_path, capsys, monkeypatch):
    from cuking_amd import run
    base = ["--synthetic", "8,9", "--output-uri", str(tmp_path / "out")]
    cases = (
        (["--site-hwe-midp"], "--site_hwe_midp needs --site_hwe_p"),
        (["--site-hwe-p", "-0.001"], "--site_hwe_p must be in [0, 1]"),
        (["--site-hwe-p", "1.5"], "--site_hwe_p must be in [0, 1]"),
        (["--site-hwe-p", "nan"], "--site_hwe_p must be in [0, 1]"),
        # it turns site filtering on: the refusals of the other site flags apply
        (["--site-hwe-p", "1e-6", "--split-factor", "2"], "need --split_factor 1"),
        (["--site_hwe_p", "1e-6", "--site_hwe_midp", "--split-factor", "2"],
         "need --split_factor 1"),
    )
    for flags, word in cases:
        assert run.main(base + flags) == 1, flags
        err = capsys.readouterr().err
        assert "Error: INVALID_ARGUMENT" in err and word in err, err
        assert "--site_hwe_p" in err
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert run.main(base + ["--site-hwe-p", "1e-6"]) == 1
    err = capsys.readouterr().err
    assert "need one process" in err and "--site_hwe_p" in err
    monkeypatch.delenv("WORLD_SIZE")
    # the flags as the run sees them
    args = run.parse_args(base + ["--site-hwe-p", "1e-6"])
    assert run.site_filtering(args) and run.hwe_rule(args) == (1e-6, False)
    args = run.parse_args(base + ["--site_hwe_p", "0.05", "--site-hwe-midp"])
    assert run.hwe_rule(args) == (0.05, True)
    args = run.parse_args(base)
    assert not run.site_filtering(args) and run.hwe_rule(args) == (None, False)
    with pytest.raises(SystemExit):
        run.parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    for name in ("site-hwe-p", "site-hwe-midp"):
        assert f"--{name}" in text, name
    assert "Hardy-Weinberg exact test" in text and "hwe_p" in text and "mid-p" in text


def load(path):
    with np.load(path) as f:
        return {name: f[name] for name in f.files}


@pytest.mark.gpu
def test_driver_filters_by_hwe_and_reports(ctx, tmp_path):
    from cuking_amd import run
    n, m = 200, 700
    path = tmp_path / "qc.npz"
    assert run.main(["--synthetic", f"{n},{m}", "--output-uri", str(tmp_path / "out"),
                     "--site-hwe-p", "1e-6", "--site-qc-uri", str(path)]) == 0
    got = load(path)
    assert got["site_counts"].shape == (m, 4) and got["site_counts"].sum() == n * m
    assert got["hwe_p"].dtype == np.float64 and got["hwe_p"].shape == (m,)
    want = cuking_amd.hwe_sites_host(got["site_counts"], m)
    assert hc.bits(got["hwe_p"]).tolist() == hc.bits(want).tolist()
    assert float(got["min_hwe_p"]) == 1e-6 and not bool(got["hwe_midp"])
    plane = cuking_amd.words_per_sample(m) // 2
    counts = np.zeros((plane * 64, 4), dtype=np.uint32)
    counts[:m] = got["site_counts"]
    counts[m:, 3] = n
    keep, _ = cuking_amd.site_mask_host(counts, m, also=cuking_amd.hwe_site_mask(want, 1e-6))
    assert got["keep"].tolist() == cuking_amd.site_mask_bool(keep, m).tolist()
    # a threshold that bites, mid-p form: the report says which form, the mask follows it
    assert run.main(["--synthetic", f"{n},{m}", "--output-uri", str(tmp_path / "out2"),
                     "--site-hwe-p", "0.2", "--site-hwe-midp", "--site-qc-uri", str(path)]) == 0
    got = load(path)
    want = cuking_amd.hwe_sites_host(got["site_counts"], m, midp=True)
    assert hc.bits(got["hwe_p"]).tolist() == hc.bits(want).tolist() and bool(got["hwe_midp"])
    keep, kept = cuking_amd.site_mask_host(counts, m, also=cuking_amd.hwe_site_mask(want, 0.2))
    assert got["keep"].tolist() == cuking_amd.site_mask_bool(keep, m).tolist() and 0 < kept < m
    # without the flag the report has no p-values
    assert run.main(["--synthetic", f"{n},{m}", "--output-uri", str(tmp_path / "out3"),
                     "--site-qc-uri", str(path)]) == 0
    assert "hwe_p" not in load(path)
