"""Kinship summary, what can be checked without a GPU: the C ABI declares and exports the six
symbols; the host helpers follow the slot rule and the key rule of include/cuking_amd.h
(restated here in numpy float32 operations, exact comparison); both entry points validate
their arguments before they touch a device; the Python driver knows the flags and refuses
them for more than one process."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import cuking_amd
from cuking_amd import _lib, api, run

ROOT = Path(__file__).resolve().parent.parent
HELPERS = ("cuking_kin_hist_slots", "cuking_kin_bin_slot", "cuking_kin_best_key",
           "cuking_kin_best_decode")
ENTRY_POINTS = ("cuking_compute_kin_summary", "cuking_compute_kin_summary_tiles")
BIN_SETS = [(-1.0, 0.5, 1536), (-0.25, 0.25, 7), (0.0, 0.5001, 4096), (0.0442, 0.0884, 1)]


def test_header_declares_and_library_exports():
    header = (ROOT / "include" / "cuking_amd.h").read_text()
    assert re.search(r"#define\s+CUKING_KIN_BINS_MAX\s+4096u?\b", header)
    assert re.search(r"#define\s+CUKING_ABI_VERSION\s+2\b", header)
    assert re.search(r"typedef\s+struct\s+cuking_kin_bins\s*\{\s*float\s+lo,\s*hi;\s*"
                     r"uint32_t\s+num_bins;\s*\}\s*cuking_kin_bins;", header)
    lib = _lib.load()
    for name in HELPERS + ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    for name in ENTRY_POINTS:
        assert re.search(r"cuking_status\s+" + name + r"\s*\(", header), name
    assert _lib.KIN_BINS_MAX == 4096
    assert lib.cuking_abi_version() == 2
    for n in (1, 7, 4096):
        assert lib.cuking_kin_hist_slots(n) == n + 3


def slot_rule(lo, hi, num_bins, kin):
    """The rule of include/cuking_amd.h in explicit float32 operations, one rounding each."""
    lo, hi, kin = np.float32(lo), np.float32(hi), np.float32(kin)
    nb = np.float32(num_bins)
    scale = np.float32(nb / np.float32(hi - lo))
    if np.isnan(kin):
        return num_bins + 2
    if kin < lo:
        return 0
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.float32(np.float32(kin - lo) * scale)
    if not t < nb:
        return num_bins + 1
    return 1 + int(np.uint32(t))


def slot_values(lo, hi, num_bins):
    f32 = np.float32
    values = [f32("nan"), f32("inf"), f32("-inf"), f32(lo), f32(hi), f32(0.5)]
    for b in range(num_bins + 1):
        edge = f32(lo + b * (hi - lo) / num_bins)
        values += [edge, np.nextafter(edge, f32("-inf")), np.nextafter(edge, f32("inf"))]
    rng = np.random.default_rng(num_bins)
    values += list(rng.uniform(-2.0, 1.0, size=10000).astype(f32))
    return values


@pytest.mark.parametrize("lo,hi,num_bins", BIN_SETS)
def test_bin_slot_follows_the_rule(lo, hi, num_bins):
    lib = _lib.load()
    bins = _lib.CKinBins(lo, hi, num_bins)
    seen = set()
    for kin in slot_values(lo, hi, num_bins):
        got = lib.cuking_kin_bin_slot(C.byref(bins), float(kin))
        assert got == slot_rule(lo, hi, num_bins, kin), (lo, hi, num_bins, float(kin))
        assert got < num_bins + 3
        seen.add(got)
    # UNDER, OVER, NAN and bins at both ends all occur
    assert {0, 1, num_bins, num_bins + 1, num_bins + 2} <= seen
    assert lib.cuking_kin_bin_slot(C.byref(bins), float(np.float32(lo))) == 1
    assert lib.cuking_kin_bin_slot(C.byref(bins), float(np.float32(hi))) == num_bins + 1
    if hi == 0.5:
        assert lib.cuking_kin_bin_slot(C.byref(bins), 0.5) == num_bins + 1    # duplicates: OVER


def test_bin_slot_of_refused_bins():
    lib = _lib.load()
    for lo, hi, n in ((0.0, 0.5, 0), (0.0, 0.5, 4097), (0.5, 0.5, 8), (float("nan"), 0.5, 8),
                      (0.0, float("inf"), 8)):
        assert lib.cuking_kin_bin_slot(C.byref(_lib.CKinBins(lo, hi, n)), 0.1) == 0xFFFFFFFF
    assert lib.cuking_kin_bin_slot(None, 0.1) == 0xFFFFFFFF


def key_rule(kin, partner):
    bits = int(np.float32(kin).view(np.uint32))
    ordered = (~bits & 0xFFFFFFFF) if bits & 0x80000000 else bits ^ 0x80000000
    return (ordered << 32) | (~partner & 0xFFFFFFFF)


def test_best_keys():
    lib = _lib.load()
    f32 = np.float32
    tiny = np.nextafter(f32(0), f32(1))            # the smallest denormal
    ordered = [f32("-inf"), f32(-3.0e38), f32(-1.5), f32(-0.25), -f32(1.2e-38), -tiny,
               f32(-0.0), f32(0.0), tiny, f32(1.0e-39), f32(1.2e-38), f32(0.0442), f32(0.25),
               np.nextafter(f32(0.5), f32(0)), f32(0.5), f32(1.0), f32(3.0e38), f32("inf")]
    assert all(a <= b for a, b in zip(ordered, ordered[1:]))
    for partner in (0, 5, 0xFFFFFFFF):
        keys = [lib.cuking_kin_best_key(float(k), partner) for k in ordered]
        assert keys == [key_rule(k, partner) for k in ordered]
        assert all(a < b for a, b in zip(keys, keys[1:])), "not strictly increasing"
        assert all(k != 0 for k in keys)
    assert lib.cuking_kin_best_key(float("-inf"), 0xFFFFFFFF) == 0x007FFFFF << 32
    # equal kinship: the lower partner gives the larger key
    for kin in (f32("-inf"), f32(-0.1), f32(0.5)):
        assert lib.cuking_kin_best_key(float(kin), 3) > lib.cuking_kin_best_key(float(kin), 4)
        assert lib.cuking_kin_best_key(float(kin), 0) > lib.cuking_kin_best_key(float(kin), 0xFFFFFFFF)
    # ... but any larger kinship beats any partner
    assert lib.cuking_kin_best_key(0.25, 0xFFFFFFFF) > lib.cuking_kin_best_key(0.125, 0)
    assert lib.cuking_kin_best_key(float("nan"), 7) == 0
    # decode(key(k, p)) = (k, p), bit for bit
    for kin in ordered:
        for partner in (0, 1, 123456, 0xFFFFFFFF):
            k, p = C.c_float(), C.c_uint32()
            key = lib.cuking_kin_best_key(float(kin), partner)
            assert lib.cuking_kin_best_decode(key, C.byref(k), C.byref(p)) == 1
            assert np.float32(k.value).view(np.uint32) == kin.view(np.uint32)
            assert p.value == partner
    k, p = C.c_float(-7.0), C.c_uint32(99)
    assert lib.cuking_kin_best_decode(0, C.byref(k), C.byref(p)) == 0
    assert (k.value, p.value) == (-7.0, 99)


def call(lib, sm, wps=2, bits=1 << 12, bins=(-1.0, 0.5, 1536), hist=1 << 13, best=1 << 14,
         ctx=None, tiles=None):
    """One of the two entry points with made-up (never dereferenced) device addresses."""
    smp = C.byref(sm.c) if sm is not None else None
    binp = C.byref(_lib.CKinBins(*bins)) if bins is not None else None
    if tiles is None:
        return lib.cuking_compute_kin_summary(ctx, smp, wps, bits, binp, hist, best, None)
    return lib.cuking_compute_kin_summary_tiles(ctx, smp, wps, bits, tiles[0], tiles[1], binp,
                                                hist, best, None)


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
    refused("null context", hist=None, bins=None)       # bins may be null when the histogram is
    refused("null context", best=None)
    refused("null submatrix", sm=None)
    refused("null bitset pointer", bits=None)
    refused("words_per_sample", wps=3)
    refused("both outputs", hist=None, best=None)
    refused("needs bins", bins=None)
    refused("num_bins 0", bins=(-1.0, 0.5, 0))
    refused("num_bins 4097", bins=(-1.0, 0.5, 4097))
    refused("finite", bins=(float("nan"), 0.5, 8))
    refused("finite", bins=(-1.0, float("inf"), 8))
    refused("finite", bins=(float("-inf"), 0.5, 8))
    refused("lo < hi", bins=(0.5, 0.5, 8))
    refused("lo < hi", bins=(0.5, -1.0, 8))
    if tiles is not None:
        refused("tile range", tiles=(2, 1))


def test_run_parses_both_spellings():
    base = ["--input-uri", "in", "--output-uri", "out"]
    for spelling in ("--kin-summary-uri", "--kin_summary_uri"):
        args = run.parse_args(base + [spelling, "s.npz"])
        assert args.kin_summary_uri == "s.npz" and args.kin_summary_bins == ""
    for spelling in ("--kin-summary-bins", "--kin_summary_bins"):
        # (a value that starts with a minus sign needs the = form)
        args = run.parse_args(base + ["--kin-summary-uri", "s.npz", spelling + "=-0.25,0.25,7"])
        assert args.kin_summary_bins == "-0.25,0.25,7"
        assert run.summary_bins(args.kin_summary_bins) == (-0.25, 0.25, 7)
    assert run.parse_args(base).kin_summary_uri == ""
    assert run.summary_bins("") == (-1.0, 0.5, 1536)
    for bad in ("1,2", "0.5,0.5,8", "0,0.5,0", "0,0.5,4097", "a,b,c", "nan,0.5,8"):
        with pytest.raises(run.UsageError):
            run.summary_bins(bad)


def test_run_refuses_several_processes_before_touching_a_device(monkeypatch, capsys, tmp_path):
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    import torch

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    monkeypatch.setattr(torch.distributed, "init_process_group", no_device)
    rc = run.main(["--synthetic", "64,100", "--output-uri", str(tmp_path),
                   "--kin-summary-uri", str(tmp_path / "summary.npz")])
    assert rc == 1
    err = capsys.readouterr().err
    assert "INVALID_ARGUMENT" in err and "kin_summary_uri" in err and "one process" in err
    assert not (tmp_path / "summary.npz").exists()


def test_kin_summary_is_exported():
    assert "kin_summary" in api.__all__ and "KinSummary" in api.__all__
    assert callable(api.kin_summary) and callable(cuking_amd.kin_summary)
    assert callable(cuking_amd.KingContext.kin_summary)
    assert cuking_amd.KinSummary is api.KinSummary
    s = api.KinSummary(None, None, -1.0, 0.5, 6, None, 0)
    assert np.array_equal(s.edges(), [-1.0, -0.75, -0.5, -0.25, 0.0, 0.25, 0.5])
