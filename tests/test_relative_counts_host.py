"""Relative counts, what can be checked without a GPU: the C ABI declares and exports the
three symbols; cuking_rel_band follows the band rule of include/cuking_amd.h (restated here in
numpy float32, exact comparison); both entry points validate their arguments before they
touch a device; the Python driver knows the flags and refuses them for more than one
process."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import cuking_amd
from cuking_amd import _lib, api, run

ROOT = Path(__file__).resolve().parent.parent
ENTRY_POINTS = ("cuking_compute_relative_counts", "cuking_compute_relative_counts_tiles")
KING = (0.0442, 0.0884, 0.177, 0.354)
THRESHOLD_SETS = [(0.05,), KING, (-0.5, -0.1, 0.0, 0.0442, 0.0884, 0.177, 0.354, 0.45)]
NONE = 0xFFFFFFFF
f32 = np.float32


def c_thresholds(values):
    return (C.c_float * max(len(values), 1))(*[float(v) for v in values])


def test_header_declares_and_library_exports():
    header = (ROOT / "include" / "cuking_amd.h").read_text()
    assert re.search(r"#define\s+CUKING_REL_THRESHOLDS_MAX\s+8u?\b", header)
    assert re.search(r"#define\s+CUKING_ABI_VERSION\s+2\b", header)
    lib = _lib.load()
    for name in ("cuking_rel_band",) + ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    assert re.search(r"uint32_t\s+cuking_rel_band\s*\(", header)
    for name in ENTRY_POINTS:
        assert re.search(r"cuking_status\s+" + name + r"\s*\(", header), name
    assert _lib.REL_THRESHOLDS_MAX == 8 and _lib.REL_NO_BAND == NONE
    assert lib.cuking_abi_version() == 2


def band_rule(thresholds, kin):
    """The largest t with kin > thresholds[t], a strict float32 comparison; NONE otherwise."""
    kin = f32(kin)
    band = NONE
    for t, thr in enumerate(thresholds):
        if kin > f32(thr):      # (False for NaN)
            band = t
    return band


def band_values(thresholds):
    values = [f32("nan"), f32("inf"), f32("-inf"), f32(0.5), f32(0.0), f32(-0.0)]
    for thr in thresholds:
        t = f32(thr)
        values += [t, np.nextafter(t, f32("-inf")), np.nextafter(t, f32("inf"))]
    rng = np.random.default_rng(len(thresholds))
    values += list(rng.uniform(-1.0, 0.75, size=10000).astype(f32))
    return values


@pytest.mark.parametrize("thresholds", THRESHOLD_SETS, ids=lambda t: f"T{len(t)}")
def test_band_follows_the_rule(thresholds):
    lib = _lib.load()
    cthr, n = c_thresholds(thresholds), len(thresholds)
    seen = set()
    for kin in band_values(thresholds):
        got = lib.cuking_rel_band(cthr, n, float(kin))
        assert got == band_rule(thresholds, kin), (thresholds, float(kin))
        seen.add(got)
    assert seen == set(range(n)) | {NONE}       # every band and "none" occur
    for t, thr in enumerate(thresholds):
        x = f32(thr)
        # strict: a kinship equal to a threshold stays below it; the next float is above
        assert lib.cuking_rel_band(cthr, n, float(x)) == (t - 1 if t else NONE)
        assert lib.cuking_rel_band(cthr, n, float(np.nextafter(x, f32("inf")))) == t
    assert lib.cuking_rel_band(cthr, n, float("nan")) == NONE
    assert lib.cuking_rel_band(cthr, n, float("-inf")) == NONE
    assert lib.cuking_rel_band(cthr, n, float("inf")) == n - 1


def test_band_of_refused_thresholds():
    lib = _lib.load()
    for bad in ((), tuple(0.01 * k for k in range(9)), (0.1, 0.1), (0.2, 0.1), (float("nan"),),
                (0.1, float("inf")), (float("-inf"), 0.1)):
        assert lib.cuking_rel_band(c_thresholds(bad), len(bad), 0.4) == NONE, bad
    assert lib.cuking_rel_band(None, 1, 0.4) == NONE


def call(lib, sm, wps=2, bits=1 << 12, thresholds=KING, num=None, counts=1 << 13, ctx=None,
         tiles=None):
    """One of the two entry points with made-up (never dereferenced) device addresses."""
    smp = C.byref(sm.c) if sm is not None else None
    thr = c_thresholds(thresholds) if thresholds is not None else None
    num = (len(thresholds) if thresholds is not None else 1) if num is None else num
    if tiles is None:
        return lib.cuking_compute_relative_counts(ctx, smp, wps, bits, thr, num, counts, None)
    return lib.cuking_compute_relative_counts_tiles(ctx, smp, wps, bits, tiles[0], tiles[1], thr,
                                                    num, counts, None)


@pytest.mark.parametrize("tiles", [None, (0, 1)])
def test_invalid_arguments_are_refused_before_any_device(tiles):
    lib = _lib.load()
    sm = cuking_amd.Submatrix(10)

    def refused(expect, **kw):
        kw.setdefault("tiles", tiles)
        assert call(lib, kw.pop("sm", sm), **kw) == _lib.ERR_INVALID_ARGUMENT
        message = lib.cuking_last_error().decode()
        assert expect in message, message

    refused("null context")
    refused("null submatrix", sm=None)
    refused("null bitset pointer", bits=None)
    refused("words_per_sample", wps=3)
    refused("null thresholds", thresholds=None)
    refused("null counts", counts=None)
    refused("num_thresholds 0", num=0)
    refused("num_thresholds 9", thresholds=tuple(0.01 * k for k in range(9)))
    refused("strictly ascending", thresholds=(0.1, 0.1))
    refused("strictly ascending", thresholds=(0.0884, 0.0442))
    refused("finite", thresholds=(float("nan"),))
    refused("finite", thresholds=(0.1, float("inf")))
    refused("finite", thresholds=(float("-inf"), 0.1))
    if tiles is not None:
        refused("tile range", tiles=(2, 1))


def test_run_parses_both_spellings():
    base = ["--input-uri", "in", "--output-uri", "out"]
    for spelling in ("--relative-counts-uri", "--relative_counts_uri"):
        args = run.parse_args(base + [spelling, "c.npz"])
        assert args.relative_counts_uri == "c.npz" and args.relative_thresholds == ""
    for spelling in ("--relative-thresholds", "--relative_thresholds"):
        args = run.parse_args(base + ["--relative-counts-uri", "c.npz", spelling + "=-0.1,0.1"])
        assert args.relative_thresholds == "-0.1,0.1"
        assert run.relative_thresholds(args.relative_thresholds) == \
            (float(f32(-0.1)), float(f32(0.1)))
    assert run.parse_args(base).relative_counts_uri == ""
    assert run.relative_thresholds("") == KING == api.KING_CUTOFFS
    for bad in ("0.2,0.1", "0.1,0.1", "a", "nan", "0.1,inf", ",".join(["0.1"] * 9),
                ",".join(str(0.01 * k) for k in range(9))):
        with pytest.raises(run.UsageError):
            run.relative_thresholds(bad)
    args = run.parse_args(base + ["--relative-thresholds=0.1"])
    with pytest.raises(run.UsageError):
        run.validate(args)          # thresholds without the file to write


def test_run_refuses_several_processes_before_touching_a_device(monkeypatch, capsys, tmp_path):
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    import torch

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    monkeypatch.setattr(torch.distributed, "init_process_group", no_device)
    rc = run.main(["--synthetic", "64,100", "--output-uri", str(tmp_path),
                   "--relative-counts-uri", str(tmp_path / "counts.npz")])
    assert rc == 1
    err = capsys.readouterr().err
    assert "INVALID_ARGUMENT" in err and "relative_counts_uri" in err and "one process" in err
    assert not (tmp_path / "counts.npz").exists()


def test_relative_counts_is_exported():
    assert "relative_counts" in api.__all__ and "RelativeCounts" in api.__all__
    assert callable(api.relative_counts) and callable(cuking_amd.relative_counts)
    assert callable(cuking_amd.KingContext.relative_counts)
    assert callable(cuking_amd.KingContext.count_records)
    assert cuking_amd.RelativeCounts is api.RelativeCounts
