"""The byte-wide site gather without a GPU: its arithmetic (csrc/king_site_gather.h: the
per-site interleave, the nibble pack, the 8 x 8 bit transposes and the byte routing) replayed
lane by lane by a stand-alone program against a plain bit loop, under AddressSanitizer + UBSan;
the option's accepted values; the test entry point's refusals."""
from host_driver import run_sanitized_driver

from cuking_amd import _lib


def test_gather_arithmetic_under_asan_ubsan(tmp_path):
    """tests/site_gather_host_driver.cc: G = 2 and 4 over 1, 2, 3, 5, 9 samples, planes of 1, 3,
    7, 65 and 320 words and an odd words_per_sample, four orders each.  A program of its own on
    the CPU: nothing is loaded into Python."""
    run_sanitized_driver(tmp_path, "site_gather_host_driver", link_host=False,
                         expect="240 cases, 0 failures")


def test_the_entry_point_checks_its_arguments_before_it_touches_a_device():
    lib = _lib.load()
    assert lib.cuking_test_site_gather(None, 1, 1, 2, 1, 4, 1, 0, None, 0, None, None) == \
        _lib.ERR_INVALID_ARGUMENT
    assert "null context" in lib.cuking_last_error().decode()
    # (the other refusals need a context: tests/test_gpu_site_gather.py)
