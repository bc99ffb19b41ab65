"""Unrelated set and families from the records, what can be checked without a GPU: the host
implementation of the contract (cuking_unrelated_set_host) against the pure-Python sequential
greedy and union-find of unrelated_cases.py -- exact equality of `keep` and `family` --, the
key helper against the key rule restated here, the argument checks that fail before a device
is touched, and the driver's usage errors."""
import ctypes as C
import re
import types
from pathlib import Path

import numpy as np
import pytest

import cuking_amd
from cuking_amd import _lib, api, run
from unrelated_cases import (check_properties, degrees, family_graph, hand_made, records,
                             yardstick)

ROOT = Path(__file__).resolve().parent.parent
f32 = np.float32
CASES = hand_made()


def host(recs, n, threshold=-np.inf, priority=None):
    return api.unrelated_set_host(recs, n, threshold, priority=priority)


def check_case(recs, n, threshold, priority):
    keep, family = host(recs, n, threshold, priority)
    exp_keep, exp_family = yardstick(recs, n, threshold, priority)
    assert keep.dtype == np.uint8 and family.dtype == np.uint32
    assert np.array_equal(keep, exp_keep), np.flatnonzero(keep != exp_keep)[:8]
    assert np.array_equal(family, exp_family), np.flatnonzero(family != exp_family)[:8]
    check_properties(recs, n, threshold, keep)
    return keep, family


def test_header_declares_and_library_exports():
    header = (ROOT / "include" / "cuking_amd.h").read_text()
    lib = _lib.load()
    for name in ("cuking_unrelated_key", "cuking_unrelated_set_host", "cuking_unrelated_set"):
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert lib.cuking_abi_version() == 2
    for name in ("unrelated_set", "unrelated_set_host", "UnrelatedSet"):
        assert name in api.__all__ and hasattr(cuking_amd, name)
    assert callable(cuking_amd.KingContext.unrelated_set) and callable(cuking_amd.KingContext.prune)


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_made_graph(name):
    check_case(*CASES[name])


def test_known_answers():
    keep, family = host(*CASES["one_edge"][:3])
    assert keep.tolist() == [1, 1, 1, 1, 1, 0, 1, 1] and family.tolist() == [0, 1, 2, 3, 4, 2, 6, 7]
    keep, _ = host(*CASES["empty"][:3])
    assert keep.tolist() == [1] * 7
    p9, n, thr, _ = CASES["path9_ascending"]
    assert host(p9, n, thr, np.arange(9, dtype=f32))[0].tolist() == [1, 0, 1, 0, 1, 0, 1, 0, 1]
    assert host(p9, n, thr, -np.arange(9, dtype=f32))[0].tolist() == [1, 0, 1, 0, 1, 0, 1, 0, 1]
    assert host(p9, n, thr, (np.arange(9) % 2).astype(f32))[0].tolist() == [0, 1, 0, 1, 0, 1, 0, 1, 0]
    # equal priorities: the lower index wins
    assert host(*CASES["equal_priorities"])[0].tolist() == [1, 0, 1, 0, 1, 0]
    # the star by default keeps its leaves, with the centre first only the centre
    assert host(*CASES["star_default"][:3])[0].tolist() == [1] * 4 + [0] + [1] * 11
    star, n, thr, prio = CASES["star_centre_first"]
    assert host(star, n, thr, prio)[0].tolist() == [1] * 5 + [0] * 11
    # a clique keeps exactly one sample; all of it is one family
    keep, family = host(*CASES["clique70"][:3])
    assert keep[3:73].sum() == 1 and keep[3] == 1 and set(family[3:73]) == {3}
    # a record below the threshold joins nothing; one AT the threshold neither (strict)
    _, family = host(*CASES["bridge_below_threshold"][:3])
    assert family.tolist() == [0, 0, 0, 3, 4, 4, 4]
    _, family = host(*CASES["bridge_at_threshold"][:3])
    assert family.tolist() == [0, 0, 2, 2]
    # NaN priorities come last, among themselves by index; +0.0 beats -0.0
    assert host(*CASES["all_nan_priorities"])[0].tolist() == [1, 0, 1, 0, 1, 0, 1]
    assert host(records([0], [1]), 2, priority=np.array([-0.0, 0.0], dtype=f32))[0].tolist() == [0, 1]
    assert host(records([0], [1]), 2, priority=np.array([np.nan, -np.inf], dtype=f32))[0].tolist() == [0, 1]


def test_repeated_edges_count_once():
    three, once = CASES["edge_three_times"], CASES["edge_once"]
    a, b = host(*three[:3]), host(*once[:3])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert a[0].tolist() == [1, 0, 1, 0, 0, 1]       # {0, 2}: every degree of the cycle is 2
    assert degrees(three[0], 6).tolist() == [2, 2, 2, 2, 2, 0]
    # and the default IS the explicit -degree over distinct partners
    explicit = host(three[0], 6, priority=-degrees(three[0], 6).astype(f32))
    assert np.array_equal(a[0], explicit[0])


@pytest.mark.parametrize("name", ["clique70_priority", "special_priorities_clique",
                                  "bridge_below_threshold", "edge_three_times"])
def test_record_order_does_not_matter(name):
    recs, n, thr, prio = CASES[name]
    first = host(recs, n, thr, prio)
    for seed in range(3):
        shuffled = recs[np.random.default_rng(seed).permutation(len(recs))]
        again = host(shuffled, n, thr, prio)
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])


@pytest.mark.parametrize("seed", range(20))
def test_family_like_random_graph(seed):
    i, j, kin = family_graph(seed)
    recs, n = records(i, j, kin), 3000
    assert len(recs) == 6000
    prio = np.random.default_rng(1000 + seed).normal(size=n).astype(f32)
    prio[::97] = prio[1]                                   # ties
    check_case(recs, n, -np.inf, prio)
    check_case(recs, n, -np.inf, None)
    check_case(recs, n, 0.2, None)                         # part of the records are no edges


def test_structured_and_word_records_agree():
    i, j, kin = family_graph(3, n=200, num_edges=300)
    recs = records(i, j, kin)
    words = recs.view(np.uint32).reshape(-1, 6)
    a, b, c = host(recs, 200), host(words, 200), host(words.view(np.int32), 200)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[0], c[0])
    keep, family = api.unrelated_set_host(recs, 200, families=False)
    assert family is None and np.array_equal(keep, a[0])
    members = api.family_members(a[1])
    assert all(len(m) >= 2 and m.min() == root for root, m in members.items())
    assert sum(len(m) for m in members.values()) == int((np.bincount(a[1], minlength=200)[a[1]] > 1).sum())


@pytest.mark.parametrize("i,j,n", [(3, 3, 8), (5, 2, 8), (2, 8, 8), (2, 0xFFFFFFFF, 8), (0, 1, 1)])
def test_invalid_records_are_refused(i, j, n):
    lib = _lib.load()
    recs = records([0, i, 1], [1, j, 2], [0.3, -5.0, 0.3])   # (not an edge: refused all the same)
    keep = np.full(n, 7, dtype=np.uint8)
    family = np.zeros(n, dtype=np.uint32)
    for threshold in (-np.inf, 0.0):
        st = lib.cuking_unrelated_set_host(recs.ctypes.data, len(recs), n, threshold, None,
                                           keep.ctypes.data, family.ctypes.data)
        assert st == _lib.ERR_INVALID_ARGUMENT
        assert "sample_i < sample_j < num_samples" in lib.cuking_last_error().decode()
    with pytest.raises(cuking_amd.CukingError) as e:
        host(recs, n)
    assert e.value.status == _lib.ERR_INVALID_ARGUMENT


def key_rule(priority, s):
    """The key restated: the order-preserving map of the float32 bits in the high word (0 for
    NaN), ~s in the low word."""
    bits = int(np.array([priority], dtype=f32).view(np.uint32)[0])
    if np.isnan(f32(priority)):
        high = 0
    else:
        high = (~bits & 0xFFFFFFFF) if bits & 0x80000000 else bits ^ 0x80000000
    return (high << 32) | (~s & 0xFFFFFFFF)


def test_key_follows_the_rule():
    lib = _lib.load()
    table = [np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, 0.5, 1e-45, -1e-45, 3.4e38,
             -3.4e38, 16777216.0, -16777217.0]
    table += list(np.random.default_rng(0).normal(size=200).astype(f32))
    samples = [0, 1, 2, 1000, 0x7FFFFFFE]
    for p in table:
        for s in samples:
            assert lib.cuking_unrelated_key(float(p), s) == key_rule(p, s), (p, s)
            if not np.isnan(p):      # a number's key IS the nearest-relative key
                assert lib.cuking_unrelated_key(float(p), s) == lib.cuking_kin_best_key(float(p), s)
    key = lambda p, s: lib.cuking_unrelated_key(float(p), s)     # noqa: E731
    # higher priority wins; among equals the lower index; NaN below -inf; no key is 0
    assert key(1.0, 9) > key(0.5, 0) > key(0.0, 0) > key(-0.0, 0) > key(-1.0, 0)
    assert key(0.25, 3) > key(0.25, 4)
    assert key(-np.inf, 5) > key(np.nan, 0) > key(np.nan, 1) > 0
    assert api.unrelated_key(np.nan, 7) == 0xFFFFFFF8
    numbers = sorted(set(float(f32(p)) for p in table if not np.isnan(p)))
    keys = [key(p, 11) for p in numbers]
    assert all(a < b for a, b in zip(keys, keys[1:]))      # order-preserving, strictly


def test_abi_refuses_bad_arguments_before_any_device():
    lib = _lib.load()
    recs = records([0], [1])
    keep = np.zeros(4, dtype=np.uint8)
    nan = float("nan")

    def refused(expect, status):
        assert status == _lib.ERR_INVALID_ARGUMENT
        assert expect in lib.cuking_last_error().decode()
    refused("NaN", lib.cuking_unrelated_set_host(recs.ctypes.data, 1, 4, nan, None,
                                                 keep.ctypes.data, None))
    refused("null records", lib.cuking_unrelated_set_host(None, 1, 4, 0.0, None,
                                                          keep.ctypes.data, None))
    refused("null keep", lib.cuking_unrelated_set_host(recs.ctypes.data, 1, 4, 0.0, None, None,
                                                       None))
    rounds = C.c_uint32(5)
    # the device entry point, with made-up (never dereferenced) device addresses
    refused("null context", lib.cuking_unrelated_set(None, 1 << 12, 1, 4, 0.0, None, 1 << 13,
                                                     None, C.byref(rounds), None))
    assert rounds.value == 0
    assert lib.cuking_unrelated_set_host(None, 0, 0, 0.0, None, None, None) == _lib.OK


def test_wrapper_checks_its_arguments_before_any_device():
    import torch
    fake = types.SimpleNamespace(device=0)      # no context: every check below comes first
    call = cuking_amd.KingContext.unrelated_set
    good = torch.zeros((4, 6), dtype=torch.int32)
    for bad, expect in ((np.zeros((4, 6), dtype=np.int32), "device tensor"),
                        (good, "this context's GPU")):
        with pytest.raises(ValueError, match=expect):
            call(fake, bad, 4, 10)
    with pytest.raises(ValueError, match="NaN"):
        call(fake, good, 4, 10, prune_threshold=float("nan"))
    for n_rec, n_samp in ((-1, 10), (4, -2), (1.5, 10), (True, 10)):
        with pytest.raises(ValueError, match="non-negative integer"):
            call(fake, good, n_rec, n_samp)
    # the whole-cohort form refuses every other block before it looks at anything else
    for sm in (cuking_amd.Submatrix(100, 2, 1), cuking_amd.Submatrix(100, 2, 2),
               cuking_amd.Submatrix.from_ranges(0, 50, 0, 60)):
        with pytest.raises(ValueError, match="unrelated_set"):
            cuking_amd.KingContext.prune(fake, sm, 2, None, 0.0442)
    # the host form
    recs = records([0], [1])
    with pytest.raises(ValueError, match="NaN"):
        api.unrelated_set_host(recs, 4, float("nan"))
    with pytest.raises(ValueError, match="records must be"):
        api.unrelated_set_host(np.zeros((3, 5), dtype=np.int32), 4)
    with pytest.raises(ValueError, match="records must be"):
        api.unrelated_set_host(np.zeros((3, 6), dtype=np.float32), 4)
    with pytest.raises(ValueError, match="priority"):
        api.unrelated_set_host(recs, 4, priority=np.zeros(3, dtype=f32))
    with pytest.raises(ValueError, match="non-negative"):
        api.unrelated_set_host(recs, -4)
    with pytest.raises(ValueError, match="families=False"):
        api.UnrelatedSet(None, None, 0, 0.0, 0).families()


BASE = ["--synthetic", "64,100", "--output-uri", "out"]


def test_run_parses_both_spellings_and_validates():
    for spelling in ("--unrelated-uri", "--unrelated_uri"):
        args = run.parse_args(BASE + [spelling, "u.npz"])
        assert args.unrelated_uri == "u.npz" and args.unrelated_threshold is None
        run.validate(args)
        assert run.unrelated_threshold(args) == float(f32(0.0884))
    args = run.parse_args(BASE + ["--unrelated_uri", "u.npz", "--unrelated_threshold", "0.177",
                                  "--unrelated_priority", "p.npy", "--kin_threshold", "0.0442"])
    run.validate(args)
    assert run.unrelated_threshold(args) == float(f32(0.177)) and args.unrelated_priority == "p.npy"
    assert run.parse_args(BASE).unrelated_uri == ""
    # equal to --kin-threshold is fine; below it is not, NaN is not
    run.validate(run.parse_args(BASE + ["--unrelated-uri", "u.npz", "--unrelated-threshold",
                                        "0.0884"]))
    for bad in (["--unrelated-uri", "u.npz", "--unrelated-threshold", "0.05"],
                ["--unrelated-uri", "u.npz", "--unrelated-threshold", "nan"],
                ["--unrelated-threshold", "0.2"],                 # without the file to write
                ["--unrelated-priority", "p.npy"],
                ["--unrelated-uri", "u.npz", "--split-factor", "2"],
                ["--unrelated-uri", "u.npz", "--split-factor", "2", "--shard-index", "1"]):
        with pytest.raises(run.UsageError):
            run.validate(run.parse_args(BASE + bad))


@pytest.mark.parametrize("extra,world,words", [
    ([], "2", ("unrelated_uri", "one process")),
    (["--split-factor", "2"], "1", ("unrelated_uri", "split_factor 1")),
    (["--unrelated-threshold", "0.01"], "1", ("unrelated_threshold", "kin_threshold")),
])
def test_run_refuses_before_touching_a_device(monkeypatch, capsys, tmp_path, extra, world, words):
    monkeypatch.setenv("WORLD_SIZE", world)
    monkeypatch.setenv("RANK", "0")
    import torch

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    monkeypatch.setattr(torch.distributed, "init_process_group", no_device)
    rc = run.main(["--synthetic", "64,100", "--output-uri", str(tmp_path),
                   "--unrelated-uri", str(tmp_path / "u.npz")] + extra)
    assert rc == 1
    err = capsys.readouterr().err
    assert "INVALID_ARGUMENT" in err and all(w in err for w in words), err
    assert not (tmp_path / "u.npz").exists()
