"""`python -m cuking_amd.run --roh-uri`: every usage error (no GPU), and the driver on a small
`.bed` with two chromosomes and real positions and on `--synthetic`, against roh_segments_host on
the same bitset (GPU)."""
import numpy as np
import pytest

import roh_cases as rc

import cuking_amd
from cuking_amd import plink

ROW_ARRAYS = ("sample", "segments", "length", "longest", "bridged")


def test_driver_usage_errors_need_no_gpu(tmp_path, capsys, monkeypatch):
    from cuking_amd import run
    base = ["--synthetic", "8,9", "--output-uri", str(tmp_path / "out")]
    roh = ["--roh-uri", str(tmp_path / "roh.npz")]
    cases = (
        (["--roh-min-sites", "100"], "need --roh_uri"),
        (["--roh-min-length", "5"], "need --roh_uri"),
        (["--roh-bridge-sites", "64"], "need --roh_uri"),
        (["--roh-segment-list"], "need --roh_uri"),
        (roh + ["--split-factor", "2"], "--roh_uri needs --split_factor 1"),
        (roh + ["--roh-min-sites", "63"], "at least 64"),
        (roh + ["--roh-bridge-sites", "63"], "0 or at least 64"),
        (roh + ["--roh-bridge-sites", "-1"], "0 or at least 64"),
        (roh + ["--roh-min-length", "-1"], "[0, 2^32)"),
        (roh + ["--roh-min-length", str(1 << 32)], "[0, 2^32)"),
    )
    for flags, word in cases:
        assert run.main(base + flags) == 1, flags
        err = capsys.readouterr().err
        assert "Error: INVALID_ARGUMENT" in err and word in err, err
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert run.main(base + roh) == 1
    assert "--roh_uri needs one process" in capsys.readouterr().err
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(SystemExit):
        run.parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    for name in ("roh-uri", "roh-min-sites", "roh-min-length", "roh-bridge-sites",
                 "roh-segment-list"):
        assert f"--{name}" in text, name
    assert "F_ROH" in text


def small_bed(prefix):
    """12 samples x 1500 sites on two chromosomes with base-pair positions; sample 0 has no het
    in 100 .. 1099, across the chromosome boundary at 700, sample 2 none in 800 .. 1400 but for
    one at 1100, sample 4 none in 200 .. 390.  Returns (geno int8, group, pos)."""
    rng = np.random.default_rng(11)
    code = rc.draw_codes(rng, 12, 1500)
    rc.plant(code, 0, 100, 1099, rng)
    rc.plant(code, 2, 800, 1400, rng)
    code[2, 1100] = 1
    rc.plant(code, 4, 200, 390, rng)
    geno = np.where(code == 3, -1, code).astype(np.int8)
    chromosomes = ["1"] * 700 + ["2"] * 800
    steps = rng.integers(1, 2000, size=1500)
    pos = np.concatenate([1000 + np.cumsum(steps[:700]), 500 + np.cumsum(steps[700:])])
    plink.write_plink(prefix, geno, chromosomes=chromosomes, positions=pos.tolist())
    return geno, np.array([0] * 700 + [1] * 800, dtype=np.int32), pos.astype(np.uint32)


def load(path):
    with np.load(path) as f:
        return {name: f[name] for name in f.files}


def check_file(got, want, min_sites, min_length, bridge_sites, samples):
    for name in ROW_ARRAYS:
        assert got[name].tobytes() == getattr(want, name).tobytes(), name
    assert got["froh"].dtype == np.float64 and got["froh"].tobytes() == want.froh().tobytes()
    assert int(got["total_length"]) == want.total_length
    assert (int(got["min_sites"]), int(got["min_length"]), int(got["bridge_sites"])) == \
        (min_sites, min_length, bridge_sites)
    assert got["samples"].shape == (samples,)
    assert got["sample"].tolist() == list(range(samples))


@pytest.mark.gpu
def test_driver_scans_a_bed(ctx, tmp_path):
    from site_qc_cases import pack
    from cuking_amd import run
    prefix, path = tmp_path / "cohort", tmp_path / "roh.npz"
    geno, group, pos = small_bed(prefix)
    m = geno.shape[1]
    bits = pack(geno)
    base = ["--bed-uri", str(prefix), "--output-uri", str(tmp_path / "out"), "--roh-uri",
            str(path), "--roh-min-sites", "200", "--roh-min-length", "150000"]
    # strictly, without the list
    assert run.main(base) == 0
    got = load(path)
    assert set(got) == {*ROW_ARRAYS, "froh", "total_length", "samples", "min_sites",
                        "min_length", "bridge_sites"}
    want = cuking_amd.roh_segments_host(bits, bits.shape[1], m, group=group, pos=pos,
                                        min_sites=200, min_length=150000)
    check_file(got, want, 200, 150000, 0, 12)
    assert int(got["total_length"]) == \
        int(pos[699]) - int(pos[0]) + int(pos[-1]) - int(pos[700])
    # sample 0: two runs, split by the chromosome boundary; sample 2: the het at 1100 splits
    # its run; sample 4: 191 sites are too few
    assert got["segments"][[0, 2, 4]].tolist() == [2, 2, 0] and not got["bridged"].any()
    # bridged, with the list
    assert run.main(base + ["--roh-bridge-sites", "64", "--roh-segment-list"]) == 0
    got = load(path)
    want = cuking_amd.roh_segments_host(bits, bits.shape[1], m, group=group, pos=pos,
                                        min_sites=200, min_length=150000, bridge_sites=64,
                                        segments=True)
    check_file(got, want, 200, 150000, 64, 12)
    segs = want.sorted()
    assert got["seg_sample"].tobytes() == segs["pair"].tobytes()
    assert np.array_equal(got["seg_first_site"], segs["first_site"])
    assert np.array_equal(got["seg_last_site"], segs["last_site"])
    assert got["segments"][[0, 2]].tolist() == [2, 1] and got["bridged"][2] == 1
    mine = np.stack([got["seg_first_site"], got["seg_last_site"]], axis=1)
    assert mine[got["seg_sample"] == 0].tolist() == [[100, 699], [700, 1099]]
    assert mine[got["seg_sample"] == 2].tolist() == [[800, 1400]]
    assert got["froh"][0] > got["froh"][2] > 0 == got["froh"][1]


@pytest.mark.gpu
def test_driver_scans_the_synthetic_cohort(ctx, tmp_path):
    from cuking_amd import run
    from cuking_amd.synth import cohort_to_device, plan_cohort
    n, m, seed = 40, 3000, 5
    path = tmp_path / "roh.npz"
    assert run.main(["--synthetic", f"{n},{m},{seed}", "--output-uri", str(tmp_path / "out"),
                     "--roh-uri", str(path), "--roh-min-sites", "64", "--roh-bridge-sites", "64",
                     "--roh-segment-list"]) == 0
    got = load(path)
    kind, pa, pb = cohort_to_device(plan_cohort(n, seed))
    bits = ctx.synth_bitset(seed, kind, pa, pb, 0, n, m).cpu().numpy().view(np.uint64)
    want = cuking_amd.roh_segments_host(bits, bits.shape[1], m, min_sites=64, bridge_sites=64,
                                        segments=True)
    check_file(got, want, 64, 0, 64, n)
    assert int(got["total_length"]) == m - 1
    segs = want.sorted()
    assert got["seg_sample"].tobytes() == segs["pair"].tobytes()
    assert np.array_equal(got["seg_first_site"], segs["first_site"])
    assert np.array_equal(got["seg_last_site"], segs["last_site"])
