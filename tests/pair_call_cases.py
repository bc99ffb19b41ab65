"""The five pair calls that come as X and X_tiles (records, dense kinship matrix, kinship
summary, relative counts, PI_HAT records) through the bare ABI, for the tests of what an
invalid call reports: tests/test_abi_host.py (no device: a null context) and
tests/test_gpu_parity.py (a context).  Output pointers are made-up addresses: every call here
is refused before anything is written."""
import ctypes as C

from cuking_amd import _lib
from cuking_amd.pihat import PiHatModel

CALLS = ("king", "kin_matrix", "kin_summary", "relative_counts", "pihat")
MATRIX_CORE_ONLY = {"kin_summary": ("kinship summary", "summary form"),
                    "relative_counts": ("relative counts", "counting form"),
                    "pihat": ("pi_hat", "PI_HAT form")}
OUT = 1 << 13                    # a made-up output address
NO_RESULT = {"king": "null result pointer", "kin_matrix": "null kinship matrix pointer",
             "kin_summary": "kinship summary: both outputs (histogram and nearest relatives) "
                            "are null",
             "relative_counts": "relative counts: null counts pointer",
             "pihat": "null result pointer"}


def refused(lib, name, ctx, sm, bits, tiles=None, wps=2, out=OUT):
    """Calls X (tiles None) or X_tiles of `name`; the call must be refused as an invalid
    argument; -> the message."""
    head = (ctx, C.byref(sm.c), wps, bits)
    rng = () if tiles is None else tuple(tiles)
    suffix = "" if tiles is None else "_tiles"
    if name == "king":
        tail = (0.05, 4, out, out, out, None)
    elif name == "kin_matrix":
        tail = (out, max(sm.NumCols(), 1), _lib.KIN_UPPER, None)
    elif name == "kin_summary":
        tail = (C.byref(_lib.CKinBins(-1.0, 0.5, 16)), out, out, None)
    elif name == "relative_counts":
        tail = ((C.c_float * 2)(0.05, 0.1), 2, out, None)
    else:
        model = PiHatModel(0.1, 0.4, 0.5, 0.4, 0.6, 10)
        tail = (C.byref(model.c), 0.1, 0, 4, out, out, out, None)
    status = getattr(lib, f"cuking_compute_{name}{suffix}")(*head, *rng, *tail)
    assert status == _lib.ERR_INVALID_ARGUMENT, (name, tiles, status)
    return lib.cuking_last_error().decode()
