"""`python -m cuking_amd.run --ibd-scan-uri`: every usage error (no GPU), and one run of the
driver on a small `.bed` with two chromosomes and real positions against ibd_scan_host on the
same bitset (GPU)."""
import numpy as np
import pytest

from test_ibd_cli import small_bed

import cuking_amd


def test_driver_usage_errors_need_no_gpu(tmp_path, capsys, monkeypatch):
    from cuking_amd import run
    base = ["--synthetic", "8,9", "--output-uri", str(tmp_path / "out")]
    scan = ["--ibd-scan-uri", str(tmp_path / "scan.npz")]
    cases = (
        (["--ibd-scan-min-sites", "100"], "need --ibd_scan_uri"),
        (["--ibd-scan-min-length", "5"], "need --ibd_scan_uri"),
        (["--ibd-scan-min-total", "5"], "need --ibd_scan_uri"),
        (scan + ["--split-factor", "3"], "--split_factor 1"),
        (scan + ["--ibd-scan-min-sites", "63"], "at least 64"),
        (scan + ["--ibd-scan-min-length", "-1"], "[0, 2^32)"),
        (scan + ["--ibd-scan-min-length", str(1 << 32)], "[0, 2^32)"),
        (scan + ["--ibd-scan-min-total", "-1"], "[0, 2^64)"),
    )
    for flags, word in cases:
        assert run.main(base + flags) == 1, flags
        err = capsys.readouterr().err
        assert "Error: INVALID_ARGUMENT" in err and word in err, err
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert run.main(base + scan) == 1
    assert "--ibd_scan_uri needs one process" in capsys.readouterr().err
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(SystemExit):
        run.parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    for name in ("ibd-scan-uri", "ibd-scan-min-sites", "ibd-scan-min-length",
                 "ibd-scan-min-total"):
        assert f"--{name}" in text, name


@pytest.mark.gpu
def test_driver_scans_every_pair(ctx, tmp_path):
    from site_qc_cases import pack
    from cuking_amd import run
    from cuking_amd.pcrelate import UNRELATED
    prefix, path = tmp_path / "cohort", tmp_path / "scan.npz"
    geno, group, pos = small_bed(prefix)
    m = geno.shape[1]
    # (the default kinship threshold: the scan does not depend on this run's records)
    assert run.main(["--bed-uri", str(prefix), "--output-uri", str(tmp_path / "out"),
                     "--ibd-scan-uri", str(path), "--ibd-scan-min-sites", "200",
                     "--ibd-scan-min-length", "150000", "--ibd-scan-min-total", "300000"]) == 0
    with np.load(path) as f:
        got = {name: f[name] for name in f.files}
    bits = pack(geno)
    want = cuking_amd.ibd_scan_host(bits, bits.shape[1], m, group=group, pos=pos, min_sites=200,
                                    min_length=150000, min_total=300000)
    assert want.num_records >= 2
    for name in ("sample_i", "sample_j", "segments1", "segments2", "length1", "length2",
                 "longest1", "longest2"):
        assert got[name].tobytes() == getattr(want, name).tobytes(), name
    pi1, pi2, kin = want.proportions()
    assert got["pi1"].tobytes() == pi1.tobytes() and got["pi2"].tobytes() == pi2.tobytes()
    assert got["kin_ibd"].tobytes() == kin.tobytes()
    assert got["relationship"].tobytes() == want.relationship().tobytes()
    assert int(got["total_length"]) == want.total_length == \
        int(pos[699]) - int(pos[0]) + int(pos[-1]) - int(pos[700])
    assert int(got["min_sites"]) == 200 and int(got["min_length"]) == 150000
    assert int(got["min_total"]) == 300000 and got["samples"].shape == (12,)
    # the planted pairs: two segments of (0, 1), split by the chromosome boundary
    at = {pair: k for k, pair in enumerate(zip(got["sample_i"].tolist(),
                                               got["sample_j"].tolist()))}
    assert got["segments2"][at[(0, 1)]] == 2 and got["segments1"][at[(2, 3)]] == 1
    assert got["relationship"][at[(0, 1)]] != UNRELATED
    assert (got["length1"] >= 300000).all()
