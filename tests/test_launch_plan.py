"""Launch planning (csrc/king_launch_plan.h) is plain integer arithmetic: a host compiler
builds a small driver against the header alone, and the plans it makes for a grid of tile
counts, block limits, workgroup counts and switches are pinned by a recorded table: a
readable selection row by row, the whole grid (1.2 million plans: every tile count up to
4,200 and the benchmark configurations', three k-step counts, four switch sets) as one hash
of its rows per kernel, workgroup count and block limit.  `launch_plan_driver --all` prints
the hashed rows, to diff two trees when a hash changes.

tests/golden/launch_plans.txt was recorded from the launchers' arithmetic as it stood
inside king_mfma.hip and king_filter.hip before it moved into the header; a change of the
launch arithmetic shows up here as a changed row (and is then a change of behaviour, to be
measured on the GPU, not a refactor)."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "cuking_amd" / "csrc"
HEADER = CSRC / "king_launch_plan.h"
GOLDEN = ROOT / "tests" / "golden" / "launch_plans.txt"


def _plans(tmp_path, *args):
    exe = tmp_path / "launch_plan_driver"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-pedantic", f"-I{CSRC}",
                    str(ROOT / "tests" / "launch_plan_driver.cc"), "-o", str(exe)], check=True)
    return subprocess.run([str(exe), *args], check=True, capture_output=True, text=True).stdout


def test_header_needs_no_hip():
    """The planner includes nothing of HIP (the driver below is built by g++ without any
    ROCm include path) and nothing of the project but itself."""
    includes = [l.split()[1] for l in HEADER.read_text().splitlines() if l.startswith("#include")]
    assert includes == ["<stdint.h>"]


def test_plans_match_recorded_table(tmp_path):
    got = _plans(tmp_path).splitlines()
    want = GOLDEN.read_text().splitlines()
    assert len(got) == len(want)
    diff = [(g, w) for g, w in zip(got, want) if g != w]
    assert not diff, f"{len(diff)} plans changed, first: got {diff[0][0]!r}, recorded {diff[0][1]!r}"


def test_hand_derived_rows():
    """Derived by hand from the launchers (256 CUs, default switches, 100k sites = 391
    k-steps of 256 sites)."""
    rows = {l.split(" |")[0]: l.split("| ")[1] for l in GOLDEN.read_text().splitlines()}
    assert sum(k.startswith("hash ") for k in rows) == 24
    # filter kernel, configs[2] (76,636 tiles of 256 samples): one chunk; no forecast, rotated,
    # no remainder pieces; 71,680 static tiles in patches, 4,956 through the counter with
    # 7,434 workgroups; grid 79,114
    assert rows["f 76636 256 0 391 default"] == \
        "c 76636 0 81921 1 0 0 71680 1 4956 7434 79114 76636 79114 79114"
    # filter kernel, configs[1] (820 tiles): forecast on, not rotated, 52 tiles in 4 pieces
    # each behind 768 whole tiles in patches; pieces from workgroup 768; grid 976
    assert rows["f 820 256 0 391 default"] == "c 820 1 81921 0 52 4 768 1 0 0 768 768 768 976"
    # four-product kernel, configs[1] (3,160 tiles of 128 samples): one split launch of
    # 3,072 whole tiles in patches and 88 tiles in 256 pieces taken by 384 workgroups
    assert rows["m 3160 256 0 391 2 16384"] == "s 0 3072 88 3072 1 256 384 3456"


def test_call_form_table(tmp_path):
    """The rules of the six call forms (kCallForms), row by row and column by column, as the
    host path had them when every layer still worked them out from the output pointers
    (king_abi.hip run_tiled and check_reducing_args, king_mfma.hip launch_form):
    k loop | layout unsorted | filter's bound may apply | VALU variants and stream kernel serve
    it | the matrix-core kernel's <KIN, FULL> and its slot for the lean and the full k loop."""
    got = _plans(tmp_path, "--forms").splitlines()
    assert got == [
        # records: lean or full by the threshold; KIN kRecords (0) has both k loops
        "0 records | either 0 1 1 | lean 0 0 0 full 0 1 1",
        # counts: the records kind's full k loop, with a counts pointer
        "1 counts | full 0 0 1 | lean refused full 0 1 1",
        # matrix (KIN 1) and summary (KIN 2): lean, on a layout that is never sorted
        "2 kinship matrix | lean 1 0 1 | lean 1 0 2 full refused",
        "3 kinship summary | lean 1 0 0 | lean 2 0 3 full refused",
        # relative counts (KIN 3): the thresholded call's lean form, sorted, filter and all
        "4 relative counts | lean 0 1 0 | lean 3 0 4 full refused",
        # PI_HAT (KIN 4): full only, no filter (its bound is one on KING kinship)
        "5 pi_hat | full 0 0 0 | lean refused full 4 1 5",
        "outside -1 -1",
    ]
    # every allowed (form, k loop) has a <KIN, FULL> of its own -- except counts, which IS the
    # records kind's full form (the kernel tells them apart by TiledArgs::dense_counts) -- and
    # the slots are 0 .. 5 without a gap: a table of 6 x nibble x split has no empty entry
    kernels, slots = {}, set()
    for line in got[:6]:
        form = int(line.split()[0])
        words = line.split(" | ")[2].split()
        i = 0
        while i < len(words):
            if words[i + 1] == "refused":
                i += 2
                continue
            kin, full, slot = (int(w) for w in words[i + 1:i + 4])
            assert full == (words[i] == "full")
            kernels.setdefault((kin, full), []).append(form)
            slots.add(slot)
            assert slot == (full if kin == 0 else kin + 1)
            i += 4
    assert slots == set(range(6))
    shared = {k: f for k, f in kernels.items() if len(f) > 1}
    assert shared == {(0, 1): [0, 1]}
    assert len(kernels) == 6
