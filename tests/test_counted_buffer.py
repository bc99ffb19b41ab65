"""The buffer rule of every call with a counted output (cuking_amd.api._counted_buffer) and the
``out`` / ``max_records`` check (_out_capacity), driven with a fake library call: no GPU."""
import ctypes as C

import numpy as np
import pytest

from cuking_amd import _lib
from cuking_amd.api import ResourceExhaustedError, _counted_buffer, _out_capacity


class FakeCall:
    """A library call that finds ``total`` items: counts them all into ``found``, reports
    RESOURCE_EXHAUSTED when they do not fit the capacity, and remembers the capacities."""

    def __init__(self, total, counted=True):
        self.total, self.counted = total, counted
        self.found = C.c_uint64(0)
        self.capacities = []

    def __call__(self, capacity):
        self.capacities.append(capacity)
        if not self.counted:            # (no counter given to the library: nothing to overflow)
            return ("buffer", capacity), _lib.OK
        self.found.value = self.total
        status = _lib.ERR_RESOURCE_EXHAUSTED if self.total > capacity else _lib.OK
        return ("buffer", capacity), status


def run(call, default, max_items, attr="num_records"):
    name = "max_records" if attr == "num_records" else "max_segments"
    return _counted_buffer(call, default, max_items, name, call.found, attr)


def test_default_capacity_suffices_one_call():
    call = FakeCall(7)
    assert run(call, 8, None) == ("buffer", 8)
    assert call.capacities == [8] and call.found.value == 7


def test_default_overflow_repeats_once_with_the_exact_count():
    call = FakeCall(21)
    assert run(call, 8, None) == ("buffer", 21)
    assert call.capacities == [8, 21]


@pytest.mark.parametrize("attr", ["num_records", "num_segments"])
def test_explicit_max_overflow_raises_with_the_count(attr):
    call = FakeCall(21)
    with pytest.raises(ResourceExhaustedError) as e:
        run(call, 8, 20, attr)
    assert getattr(e.value, attr) == 21
    assert call.capacities == [20]
    # (a max that fits is one call, whatever the default)
    call = FakeCall(21)
    assert run(call, 8, 21, attr) == ("buffer", 21) and call.capacities == [21]


def test_capacity_zero_counts_only():
    call = FakeCall(5)
    with pytest.raises(ResourceExhaustedError) as e:
        run(call, 8, 0, "num_segments")
    assert e.value.num_segments == 5 and call.capacities == [0]
    call = FakeCall(0)
    assert run(call, 8, 0) == ("buffer", 0) and call.capacities == [0]


def test_a_list_that_is_not_wanted_has_capacity_zero_and_no_retry():
    call = FakeCall(5, counted=False)
    assert run(call, 0, None, "num_segments") == ("buffer", 0)
    assert call.capacities == [0]


def test_a_bad_max_is_refused_before_any_call():
    call = FakeCall(5)
    with pytest.raises(ValueError, match="max_records"):
        run(call, 8, -1)
    assert call.capacities == []


def test_out_gives_the_default_max_and_bounds_it():
    out = np.zeros((12, 6), dtype=np.int32)
    assert _out_capacity(out, None) == 12
    assert _out_capacity(out, 12) == 12 and _out_capacity(out, 3) == 3
    with pytest.raises(ValueError, match="out holds 12 records, max_records is 13"):
        _out_capacity(out, 13)
