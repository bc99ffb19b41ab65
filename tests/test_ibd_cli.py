"""`python -m cuking_amd.run --ibd-segments-uri`: every usage error (no GPU), and one run of the
driver on a small `.bed` with two chromosomes and real positions against ibd_segments_host on
the same bitset (GPU)."""
import numpy as np
import pytest

import ibd_cases as ic

import cuking_amd
from cuking_amd import plink


def test_driver_usage_errors_need_no_gpu(tmp_path, capsys, monkeypatch):
    from cuking_amd import run
    base = ["--synthetic", "8,9", "--output-uri", str(tmp_path / "out")]
    seg = ["--ibd-segments-uri", str(tmp_path / "ibd.npz")]
    cases = (
        (["--ibd-min-sites", "100"], "need --ibd_segments_uri"),
        (["--ibd-min-length", "5"], "need --ibd_segments_uri"),
        (["--ibd-segment-list"], "need --ibd_segments_uri"),
        (seg + ["--split-factor", "3"], "--split_factor 1"),
        (seg + ["--ibd-min-sites", "63"], "at least 64"),
        (seg + ["--ibd-min-length", "-1"], "[0, 2^32)"),
        (seg + ["--ibd-min-length", str(1 << 32)], "[0, 2^32)"),
    )
    for flags, word in cases:
        assert run.main(base + flags) == 1, flags
        err = capsys.readouterr().err
        assert "Error: INVALID_ARGUMENT" in err and word in err, err
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert run.main(base + seg) == 1
    assert "--ibd_segments_uri needs one process" in capsys.readouterr().err
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(SystemExit):
        run.parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    for name in ("ibd-segments-uri", "ibd-min-sites", "ibd-min-length", "ibd-segment-list"):
        assert f"--{name}" in text, name
    assert "LD pruning thins the markers a segment is counted in" in text


def small_bed(prefix):
    """12 samples x 1500 sites on two chromosomes with base-pair positions; (0, 1) share sites
    100 .. 1099 across the chromosome boundary at 700 (kind 2), (2, 3) sites 800 .. 1400 (kind
    1).  Returns (geno int8, group, pos)."""
    rng = np.random.default_rng(11)
    code = ic.draw_codes(rng, 12, 1500)
    ic.plant(code, 0, 1, 100, 1099, 2)
    ic.plant(code, 2, 3, 800, 1400, 1)
    geno = np.where(code == 3, -1, code).astype(np.int8)
    chromosomes = ["1"] * 700 + ["2"] * 800
    steps = rng.integers(1, 2000, size=1500)
    pos = np.concatenate([1000 + np.cumsum(steps[:700]), 500 + np.cumsum(steps[700:])])
    plink.write_plink(prefix, geno, chromosomes=chromosomes, positions=pos.tolist())
    return geno, np.array([0] * 700 + [1] * 800, dtype=np.int32), pos.astype(np.uint32)


@pytest.mark.gpu
def test_driver_scans_its_records(ctx, tmp_path):
    from site_qc_cases import pack
    from cuking_amd import run
    from cuking_amd.pcrelate import UNRELATED
    prefix, path = tmp_path / "cohort", tmp_path / "ibd.npz"
    geno, group, pos = small_bed(prefix)
    m = geno.shape[1]
    assert run.main(["--bed-uri", str(prefix), "--output-uri", str(tmp_path / "out"),
                     "--kin-threshold=-10", "--ibd-segments-uri", str(path),   # (every pair)
                     "--ibd-min-sites", "200", "--ibd-min-length", "150000",
                     "--ibd-segment-list"]) == 0
    with np.load(path) as f:
        got = {name: f[name] for name in f.files}
    index = np.stack([got["sample_i"], got["sample_j"]], axis=1).astype(np.uint32)
    listed = {(int(i), int(j)) for i, j in index}
    assert {(0, 1), (2, 3)} <= listed
    bits = pack(geno)
    want = cuking_amd.ibd_segments_host(bits, bits.shape[1], m, index, group=group, pos=pos,
                                        min_sites=200, min_length=150000, segments=True)
    for name in ("segments1", "segments2", "length1", "length2", "longest1", "longest2"):
        assert got[name].tobytes() == getattr(want, name).tobytes(), name
    pi1, pi2, kin = want.proportions()
    assert got["pi1"].tobytes() == pi1.tobytes() and got["pi2"].tobytes() == pi2.tobytes()
    assert got["kin_ibd"].tobytes() == kin.tobytes()
    assert got["relationship"].tobytes() == want.relationship().tobytes()
    assert int(got["total_length"]) == want.total_length == \
        int(pos[699]) - int(pos[0]) + int(pos[-1]) - int(pos[700])
    assert int(got["min_sites"]) == 200 and int(got["min_length"]) == 150000
    assert got["samples"].shape == (12,)
    segs = want.sorted()
    assert got["segment_pair"].tobytes() == segs["pair"].tobytes()
    assert got["segment_kind"].tobytes() == segs["kind"].tobytes()
    assert np.array_equal(got["segment_first_site"], segs["first_site"])
    assert np.array_equal(got["segment_last_site"], segs["last_site"])
    # the planted pairs: two segments of (0, 1), split by the chromosome boundary
    at = {pair: k for k, pair in enumerate(map(tuple, index.tolist()))}
    assert got["segments2"][at[(0, 1)]] == 2 and got["segments1"][at[(2, 3)]] == 1
    assert got["relationship"][at[(0, 1)]] != UNRELATED
    mine = segs[(segs["pair"] == at[(0, 1)]) & (segs["kind"] == 2)]
    assert mine[["first_site", "last_site"]].tolist() == [(100, 699), (700, 1099)]
