"""`python -m cuking_amd.run --ibd-segments-uri ... --ibd-bridge-sites N`: the usage errors (no
GPU), and one run of the driver on a small `.bed` with one genotyping error inside a planted
segment: the flag round-trips into the `.npz`, without it the keys are absent (GPU)."""
import numpy as np
import pytest

import ibd_cases as ic

import cuking_amd
from cuking_amd import plink


def test_driver_usage_errors_need_no_gpu(tmp_path, capsys):
    from cuking_amd import run
    base = ["--synthetic", "8,9", "--output-uri", str(tmp_path / "out")]
    seg = ["--ibd-segments-uri", str(tmp_path / "ibd.npz")]
    cases = (
        (["--ibd-bridge-sites", "64"], "--ibd_bridge_sites needs --ibd_segments_uri"),
        (seg + ["--ibd-bridge-sites", "10"], "0 or at least 64"),
        (seg + ["--ibd-bridge-sites", "63"], "0 or at least 64"),
        (seg + ["--ibd-bridge-sites", "-1"], "0 or at least 64"),
        (seg + ["--ibd-bridge-sites", str(1 << 32)], "below 2^32"),
    )
    for flags, word in cases:
        assert run.main(base + flags) == 1, flags
        err = capsys.readouterr().err
        assert "Error: INVALID_ARGUMENT" in err and word in err, err
    with pytest.raises(SystemExit):
        run.parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--ibd-bridge-sites" in text and "bridged1" in text


def noisy_bed(prefix):
    """12 samples x 1500 sites on two chromosomes; (0, 1) share sites 100 .. 1099 across the
    chromosome boundary at 700 (kind 2) but for one opposite homozygote at site 400.  Returns
    (geno int8, group, pos)."""
    rng = np.random.default_rng(11)
    code = ic.draw_codes(rng, 12, 1500)
    ic.plant(code, 0, 1, 100, 1099, 2)
    ic.make_opp(code, 0, 1, 400)
    geno = np.where(code == 3, -1, code).astype(np.int8)
    steps = rng.integers(1, 2000, size=1500)
    pos = np.concatenate([1000 + np.cumsum(steps[:700]), 500 + np.cumsum(steps[700:])])
    plink.write_plink(prefix, geno, chromosomes=["1"] * 700 + ["2"] * 800,
                      positions=pos.tolist())
    return geno, np.array([0] * 700 + [1] * 800, dtype=np.int32), pos.astype(np.uint32)


@pytest.mark.gpu
def test_the_flag_round_trips(ctx, tmp_path):
    from site_qc_cases import pack
    from cuking_amd import run
    prefix = tmp_path / "cohort"
    geno, group, pos = noisy_bed(prefix)
    m = geno.shape[1]
    files = {}
    for name, flags in (("strict", []), ("bridged", ["--ibd-bridge-sites", "64"]),
                        ("zero", ["--ibd-bridge-sites", "0"])):
        path = tmp_path / f"{name}.npz"
        assert run.main(["--bed-uri", str(prefix), "--output-uri", str(tmp_path / "out"),
                         "--kin-threshold=-10", "--ibd-segments-uri", str(path),
                         "--ibd-min-sites", "200", "--ibd-segment-list"] + flags) == 0
        with np.load(path) as f:
            files[name] = {key: f[key] for key in f.files}
    strict, bridged, zero = files["strict"], files["bridged"], files["zero"]
    # without the flag the file is what it was
    assert not {"bridge_sites", "bridged1", "bridged2"} & set(strict)
    assert set(bridged) == set(strict) | {"bridge_sites", "bridged1", "bridged2"} == set(zero)
    assert int(bridged["bridge_sites"]) == 64 and int(zero["bridge_sites"]) == 0
    for key in strict:   # bridge_sites 0: the strict file, and nothing bridged
        assert zero[key].tobytes() == strict[key].tobytes(), key
    assert not zero["bridged1"].any() and not zero["bridged2"].any()
    index = np.stack([bridged["sample_i"], bridged["sample_j"]], axis=1).astype(np.uint32)
    bits = pack(geno)
    want = cuking_amd.ibd_segments_host(bits, bits.shape[1], m, index, group=group, pos=pos,
                                        min_sites=200, segments=True, bridge_sites=64)
    for name in ("segments1", "segments2", "length1", "length2", "longest1", "longest2"):
        assert bridged[name].tobytes() == getattr(want, name).tobytes(), name
    assert bridged["bridged1"].dtype == np.uint32
    assert bridged["bridged1"].tobytes() == want.bridged[:, 0].tobytes()
    assert bridged["bridged2"].tobytes() == want.bridged[:, 1].tobytes()
    assert bridged["relationship"].tobytes() == want.relationship().tobytes()
    segs = want.sorted()
    assert np.array_equal(bridged["segment_first_site"], segs["first_site"])
    assert np.array_equal(bridged["segment_last_site"], segs["last_site"])
    # the planted pair: the error splits the first chromosome's segment, the bridge mends it
    at = {pair: k for k, pair in enumerate(map(tuple, index.tolist()))}[(0, 1)]
    assert strict["segments2"][at] == 3 and bridged["segments2"][at] == 2
    assert bridged["bridged1"][at] == 1 and bridged["bridged2"][at] == 1
    mine = segs[(segs["pair"] == at) & (segs["kind"] == 2)]
    assert mine[["first_site", "last_site"]].tolist() == [(100, 699), (700, 1099)]
