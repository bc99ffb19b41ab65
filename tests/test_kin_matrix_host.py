"""Dense kinship matrix, what can be checked without a GPU: the C ABI declares and exports
both entry points and validates its arguments before it touches a device; the Python
driver knows the flag and refuses it for more than one process."""
import ctypes as C
import re
import sys
from pathlib import Path

import pytest

import cuking_amd
from cuking_amd import _lib, api, run

ROOT = Path(__file__).resolve().parent.parent
ENTRY_POINTS = ("cuking_compute_kin_matrix", "cuking_compute_kin_matrix_tiles")


def test_header_declares_and_library_exports():
    header = (ROOT / "include" / "cuking_amd.h").read_text()
    assert re.search(r"#define\s+CUKING_KIN_UPPER\s+0u", header)
    assert re.search(r"#define\s+CUKING_KIN_SYMMETRIC\s+1u", header)
    assert re.search(r"#define\s+CUKING_ABI_VERSION\s+2\b", header)
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert re.search(r"cuking_status\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    assert (_lib.KIN_UPPER, _lib.KIN_SYMMETRIC) == (0, 1)
    assert lib.cuking_abi_version() == 2


def call(lib, sm, wps=2, bits=1 << 12, kin=1 << 13, ld=None, flags=0, ctx=None, tiles=None):
    """One of the two entry points with made-up (never dereferenced) device addresses."""
    smp = C.byref(sm.c) if sm is not None else None
    if ld is None:
        ld = sm.NumCols() if sm is not None else 0
    if tiles is None:
        return lib.cuking_compute_kin_matrix(ctx, smp, wps, bits, kin, ld, flags, None)
    return lib.cuking_compute_kin_matrix_tiles(ctx, smp, wps, bits, tiles[0], tiles[1], kin, ld,
                                               flags, None)


@pytest.mark.parametrize("tiles", [None, (0, 1)])
def test_invalid_arguments_are_refused_before_any_device(tiles):
    lib = _lib.load()
    sm = cuking_amd.Submatrix(10)
    off = cuking_amd.Submatrix(10, 2, 1)

    def refused(expect, **kw):
        assert call(lib, kw.pop("sm", sm), tiles=tiles, **kw) == _lib.ERR_INVALID_ARGUMENT
        message = lib.cuking_last_error().decode()
        assert expect in message, message

    refused("null context")
    refused("", sm=None)
    assert lib.cuking_last_error().decode() != ""
    refused("null bitset pointer", bits=None)
    refused("null kinship matrix pointer", kin=None)
    refused("leading dimension", ld=9)
    refused("flags", flags=2)
    refused("diagonal block", sm=off, flags=_lib.KIN_SYMMETRIC)
    if tiles is not None:
        refused("tile range", flags=_lib.KIN_SYMMETRIC)


def test_run_parses_both_spellings():
    for spelling in ("--kin-matrix-uri", "--kin_matrix_uri"):
        args = run.parse_args(["--input-uri", "in", "--output-uri", "out", spelling, "m.npy"])
        assert args.kin_matrix_uri == "m.npy"
    assert run.parse_args(["--input-uri", "in", "--output-uri", "out"]).kin_matrix_uri == ""


def test_run_refuses_several_processes_before_touching_a_device(monkeypatch, capsys, tmp_path):
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    import torch

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    monkeypatch.setattr(torch.distributed, "init_process_group", no_device)
    rc = run.main(["--synthetic", "64,100", "--output-uri", str(tmp_path),
                   "--kin-matrix-uri", str(tmp_path / "kin.npy")])
    assert rc == 1
    err = capsys.readouterr().err
    assert "INVALID_ARGUMENT" in err and "kin_matrix_uri" in err and "one process" in err
    assert not (tmp_path / "kin.npy").exists()


def test_kin_matrix_is_exported():
    assert "kin_matrix" in api.__all__
    assert callable(api.kin_matrix) and callable(cuking_amd.kin_matrix)
    assert callable(cuking_amd.KingContext.kin_matrix)
