"""The head lap of the filter kernel's tiles on a site-ordered layout (king_filter.hip
`plan_checks`, the segment loop of `filter_tile`, `addr_of` / `addr_next`), restated in Python:
a tile starts at a phase p inside the head [0, 2 H) of the order, runs to the head's end, wraps
to the first site, runs up to p, is checked there, and only then goes on into the tail.  Checked
for every bitset length from the shortest that can lap up to 260 k-steps, every share H = 32 ..
62 and every start phase."""
import pytest

PHASES = 128           # king_common.h kNumPhases
MIN_STEPS = 4          # "filter_rotate_min_steps" as the GPU tests set it
NO_WRAP = 1 << 32


def phase_step(all_steps, x):
    return all_steps * x // PHASES


def plan(all_steps, share, raw_phase, min_steps=MIN_STEPS):
    """plan_checks() for a whole tile of an ordered layout under a test hook (`raw_phase`: the
    hook's phase before its reduction), check 1 automatic, no check 0."""
    head = 2 * share
    k_head = phase_step(all_steps, head)
    lap = share != 0 and min_steps <= k_head < all_steps
    ring, ring_phases = (k_head, head) if lap else (all_steps, PHASES)
    phase = k0 = 0
    if lap:
        phase = (raw_phase & (PHASES - 1)) % ring_phases
        k0 = phase_step(all_steps, phase)
        if phase >= ring_phases or k0 >= ring:
            phase = k0 = 0
    wrap = ring - k0 if k0 != 0 else 0
    chk1 = ring if lap else k_head          # (unrotated: steps_of(share) from phase 0)
    if not 0 < chk1 < all_steps:
        chk1 = 0
    return dict(lap=lap, phase=phase, k0=k0, wrap=wrap, ring=ring, chk1=chk1)


def joined_phase(all_steps, share, xcd_pos):
    """plan_checks(), the real path: the phase boundary nearest to the XCD's position in the ring."""
    head = 2 * share
    ring = phase_step(all_steps, head)
    r = xcd_pos % ring
    phase = (r * PHASES + all_steps // 2) // all_steps
    k0 = phase_step(all_steps, phase)
    if phase >= head or k0 >= ring:
        phase = k0 = 0
    return phase, k0


def segments(p, all_steps):
    """The segment loop: [(first, end)] in the tile's own k-steps, and per segment the runs of
    bitset k-steps [(begin, end)] it requests (seg_k, seg_wrap and the ring)."""
    out, seg_first = [], 0
    while True:
        seg_end = p["chk1"] if p["chk1"] > seg_first else all_steps
        k0, wrap, ring = p["k0"], p["wrap"], p["ring"]
        seg_k = (seg_first if seg_first >= ring
                 else seg_first - wrap if wrap != 0 and seg_first >= wrap
                 else k0 + seg_first)
        seg_wrap = wrap - seg_first if seg_first < wrap < seg_end else NO_WRAP
        steps = seg_end - seg_first
        if seg_wrap == NO_WRAP:
            runs = [(seg_k, seg_k + steps)]
        else:
            runs = [(seg_k, seg_k + seg_wrap), (seg_k + seg_wrap - ring, seg_k + steps - ring)]
        out.append(((seg_first, seg_end), seg_k, seg_wrap, runs))
        if seg_end == all_steps:
            return out
        seg_first = seg_end


def covers_once(runs, lo, hi):
    runs = sorted(r for r in runs if r[0] != r[1])
    at = lo
    for b, e in runs:
        if b != at or e <= b:
            return False
        at = e
    return at == hi


def test_every_lap_visits_the_head_first_and_every_k_step_once():
    laps = 0
    for all_steps in range(MIN_STEPS, 261):
        for share in range(32, 63):
            k_head = phase_step(all_steps, 2 * share)
            for raw in range(2 * share):
                p = plan(all_steps, share, raw)
                if k_head < MIN_STEPS:
                    # a head shorter than rotate_min_steps: the unrotated plan
                    assert (p["lap"], p["k0"], p["wrap"], p["ring"]) == (False, 0, 0, all_steps)
                    continue
                assert p["lap"] and p["ring"] == k_head and p["chk1"] == k_head
                assert p["phase"] < 2 * share and p["k0"] < k_head
                segs = segments(p, all_steps)
                # two segments: the lap in front of the check, the tail behind it
                assert [s[0] for s in segs] == [(0, k_head), (k_head, all_steps)]
                lap_runs, tail_runs = segs[0][3], segs[1][3]
                # the first kH k-steps of the tile are exactly the head, in the order
                # [k0, kH), [0, k0); the tail starts at kH, not at k0
                want = [(p["k0"], k_head), (0, p["k0"])] if p["k0"] else [(0, k_head)]
                assert lap_runs == want, (all_steps, share, raw)
                assert tail_runs == [(k_head, all_steps)]
                assert covers_once(lap_runs, 0, k_head)
                assert covers_once(lap_runs + tail_runs, 0, all_steps)
                laps += 1
    assert laps > 500000


@pytest.mark.parametrize("share", [32, 48, 62])
def test_a_phase_beyond_the_head_is_reduced_and_the_heads_end_is_its_beginning(share):
    for all_steps in (5, 12, 32, 80, 391):
        if phase_step(all_steps, 2 * share) < MIN_STEPS:
            continue
        assert plan(all_steps, share, 2 * share)["phase"] == 0
        for raw in (77, 127):
            p = plan(all_steps, share, raw)
            same = plan(all_steps, share, raw % (2 * share))
            assert p == same and p["phase"] in (0, raw % (2 * share))
        # the real path: every position of the ring joins a boundary inside the head
        k_head = phase_step(all_steps, 2 * share)
        for pos in range(3 * k_head):
            phase, k0 = joined_phase(all_steps, share, pos)
            assert phase < 2 * share and k0 < k_head
            # ... the nearest one: within a phase's length of the position
            r = pos % k_head
            dist = min(abs(k0 - r), k_head - abs(k0 - r))
            assert dist <= (all_steps + PHASES - 1) // PHASES, (all_steps, pos, phase)


def test_a_short_head_or_a_missing_share_gives_the_unrotated_plan():
    # default rotate_min_steps 128: 80 k-steps never lap; a share of 0: no check at all
    for raw in (0, 1, 77):
        p = plan(80, 48, raw, min_steps=128)
        assert (p["lap"], p["k0"], p["wrap"], p["ring"], p["chk1"]) == (False, 0, 0, 80, 60)
        assert segments(p, 80)[0][3] == [(0, 60)]
        p = plan(80, 0, raw)
        assert (p["lap"], p["k0"], p["chk1"]) == (False, 0, 0)
        assert [s[3] for s in segments(p, 80)] == [[(0, 80)]]
    # 12 k-steps (3,000 sites): too short under the default, long enough with 4
    assert not plan(12, 48, 5, min_steps=128)["lap"] and plan(12, 48, 5)["lap"]


@pytest.mark.parametrize("all_steps", [5, 12, 32, 80, 130, 391])
def test_request_addresses_follow_the_lap(all_steps):
    """addr_of for the first four stages of a segment, addr_next from there on: k-step `step`
    of a segment names seg_k + step, one RING back from seg_wrap on; steps beyond the segment
    repeat its last one.  Every request stays inside the bitset."""
    for share in (32, 41, 48, 62):
        if phase_step(all_steps, 2 * share) < MIN_STEPS:
            continue
        for raw in range(0, 2 * share, 3):
            p = plan(all_steps, share, raw)
            k0, k_head, ring = p["k0"], p["chk1"], p["ring"]
            tile = list(range(k0, k_head)) + list(range(0, k0)) + list(range(k_head, all_steps))
            for (seg_first, seg_end), seg_k, seg_wrap, _ in segments(p, all_steps):
                seg_steps, pos = seg_end - seg_first, None
                for step in range(seg_steps + 4):
                    if step < 4:
                        s = min(step, seg_steps - 1)
                        pos = seg_k + s - (ring if s >= seg_wrap else 0)
                    else:
                        pos += (1 if step < seg_steps else 0) - (ring if step == seg_wrap else 0)
                    assert 0 <= pos < all_steps
                    assert pos == tile[seg_first + min(step, seg_steps - 1)], (share, raw, step)
