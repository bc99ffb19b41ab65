"""`python -m cuking_amd.run --mendel-uri`: every usage error (no GPU), and the driver on a small
`.bed` whose `.fam` declares parents and on `--synthetic` with `--mendel-trios`, against
mendel_errors_host on the same bitset (GPU)."""
from pathlib import Path

import numpy as np
import pytest

import mendel_cases as mc

import cuking_amd
from cuking_amd import plink

ROW_ARRAYS = ("called", "errors")


def write_fam(prefix, lines):
    Path(str(prefix) + ".fam").write_text("".join(line + "\n" for line in lines))


def test_driver_usage_errors_need_no_gpu(tmp_path, capsys, monkeypatch):
    from cuking_amd import run
    base = ["--synthetic", "8,9", "--output-uri", str(tmp_path / "out")]
    uri = ["--mendel-uri", str(tmp_path / "mendel.npz")]
    good = tmp_path / "good.npy"
    np.save(good, np.array([[2, 0, 1], [3, -1, 1]]))
    listed = uri + ["--mendel-trios", str(good)]

    def saved(name, array):
        np.save(tmp_path / name, array)
        return uri + ["--mendel-trios", str(tmp_path / name)]
    plink.write_plink(tmp_path / "plain", np.zeros((4, 5), dtype=np.int8))
    cases = (
        (["--mendel-trios", str(good)], "need --mendel_uri"),
        (["--mendel-site-counts"], "need --mendel_uri"),
        (listed + ["--split-factor", "2"], "--mendel_uri needs --split_factor 1"),
        (uri, "--mendel_uri needs --mendel_trios"),
        (uri + ["--mendel-trios", str(tmp_path / "nowhere.npy")], "cannot read"),
        (saved("flat.npy", np.arange(6)), "integer [T, 3]"),
        (saved("float.npy", np.zeros((2, 3))), "integer [T, 3]"),
        (saved("beyond.npy", np.array([[2, 0, 8]])), "below the cohort's size (8)"),
        (saved("minus.npy", np.array([[2, 0, -2]])), "-1 for an absent parent only"),
        (saved("child.npy", np.array([[-1, 0, 1]])), "-1 for an absent parent only"),
    )
    for flags, word in cases:
        assert run.main(base + flags) == 1, flags
        err = capsys.readouterr().err
        assert "Error: INVALID_ARGUMENT" in err and word in err, err
    # a .fam that declares no parent
    assert run.main(["--bed-uri", str(tmp_path / "plain"), "--output-uri", str(tmp_path / "out")]
                    + uri) == 1
    err = capsys.readouterr().err
    assert "Error: INVALID_ARGUMENT" in err and "declares no parent" in err, err
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert run.main(base + listed) == 1
    assert "--mendel_uri needs one process" in capsys.readouterr().err
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(SystemExit):
        run.parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    for name in ("mendel-uri", "mendel-trios", "mendel-site-counts"):
        assert f"--{name}" in text, name
    assert "hl.mendel_errors" in text


def load(path):
    with np.load(path) as f:
        return {name: f[name] for name in f.files}


def check_file(got, want, trios, samples):
    for name in ROW_ARRAYS:
        assert got[name].tobytes() == getattr(want, name).tobytes(), name
    signed = np.where(trios == cuking_amd.NO_PARENT, -1, trios.astype(np.int64))
    for column, name in enumerate(("child", "father", "mother")):
        assert got[name].dtype == np.int64 and got[name].tolist() == signed[:, column].tolist()
    assert got["rate"].dtype == np.float64 and got["rate"].tobytes() == want.rate().tobytes()
    assert got["per_sample"].tolist() == want.per_sample(samples).tolist()
    assert got["samples"].shape == (samples,)


@pytest.mark.gpu
def test_driver_counts_the_trios_of_a_fam(ctx, tmp_path):
    """The family cohort of mendel_cases.py with planted errors as a .bed; the .fam declares the
    three children's parents, one of them with a mother that is not in the file."""
    from site_qc_cases import pack
    from cuking_amd import run
    case = next(c for c in mc.CASES if c.name == "planted, 4097 sites")
    code = mc.inputs(case).code
    geno = np.where(code == mc.MISSING, -1, code).astype(np.int8)
    n, m = geno.shape
    prefix, path = tmp_path / "cohort", tmp_path / "mendel.npz"
    plink.write_plink(prefix, geno)
    ids = plink.read_fam(prefix)
    parents = {6: (ids[0], ids[1]), 7: (ids[0], "stranger"), 8: (ids[2], ids[3])}
    write_fam(prefix, [f"{s} {s} {parents.get(k, ('0', '0'))[0]} {parents.get(k, ('0', '0'))[1]} "
                       "0 -9" for k, s in enumerate(ids)])
    trios = np.array([[6, 0, 1], [7, 0, cuking_amd.NO_PARENT], [8, 2, 3]], dtype=np.uint32)
    bits = pack(geno)
    base = ["--bed-uri", str(prefix), "--output-uri", str(tmp_path / "out"), "--mendel-uri",
            str(path)]
    assert run.main(base) == 0
    got = load(path)
    assert set(got) == {"child", "father", "mother", "called", "errors", "rate", "per_sample",
                        "samples"}
    want = cuking_amd.mendel_errors_host(bits, bits.shape[1], m, trios, site_counts=True)
    check_file(got, want, trios, n)
    planted = mc.planted_sites(case)
    assert got["errors"][:2].sum() == 0 and got["errors"][2].sum() == len(planted)
    assert got["per_sample"][8] == len(planted) and got["per_sample"][[0, 1, 6, 7]].sum() == 0
    # with the site counts, and a list that overrides the .fam
    listed = tmp_path / "trios.npy"
    np.save(listed, np.array([[8, 2, 3], [8, -1, 3], [8, 2, 3]]))
    assert run.main(base + ["--mendel-site-counts", "--mendel-trios", str(listed)]) == 0
    got = load(path)
    trios = np.array([[8, 2, 3], [8, cuking_amd.NO_PARENT, 3], [8, 2, 3]], dtype=np.uint32)
    want = cuking_amd.mendel_errors_host(bits, bits.shape[1], m, trios, site_counts=True)
    check_file(got, want, trios, n)
    assert got["site_errors"].dtype == np.uint32 and \
        got["site_errors"].tobytes() == want.site_errors.tobytes()
    assert got["site_index"].tolist() == list(range(m))
    assert np.flatnonzero(got["site_errors"]).tolist() == sorted(planted)
    assert set(got["site_errors"][sorted(planted)].tolist()) <= {2, 3}


@pytest.mark.gpu
def test_driver_counts_listed_trios_of_the_synthetic_cohort(ctx, tmp_path):
    from cuking_amd import run
    from cuking_amd.synth import cohort_to_device, plan_cohort
    n, m, seed = 40, 3000, 5
    path, listed = tmp_path / "mendel.npz", tmp_path / "trios.npy"
    rng = np.random.default_rng(4)
    signed = rng.integers(0, n, size=(25, 3))
    signed[::4, 1] = -1
    signed[::5, 2] = -1
    np.save(listed, signed)
    assert run.main(["--synthetic", f"{n},{m},{seed}", "--output-uri", str(tmp_path / "out"),
                     "--mendel-uri", str(path), "--mendel-trios", str(listed),
                     "--mendel-site-counts"]) == 0
    got = load(path)
    kind, pa, pb = cohort_to_device(plan_cohort(n, seed))
    bits = ctx.synth_bitset(seed, kind, pa, pb, 0, n, m).cpu().numpy().view(np.uint64)
    trios = np.where(signed < 0, cuking_amd.NO_PARENT, signed).astype(np.uint32)
    want = cuking_amd.mendel_errors_host(bits, bits.shape[1], m, trios, site_counts=True)
    check_file(got, want, trios, n)
    assert got["site_errors"].tobytes() == want.site_errors.tobytes() and want.total().sum() > 0
    assert got["site_index"].tolist() == list(range(m))
