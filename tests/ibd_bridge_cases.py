"""IBD segments with bridged breaks: the cases the host and the GPU tests share, and the NAIVE
restatement both are compared with -- the per-site runs of ibd_cases.naive, then the linking of
consecutive runs in plain Python.  It knows no words and nothing of csrc/king_ibd.h.

The builders are those of ibd_cases.py (unrelated pairs meet an opposite homozygote every ten
sites or so, planted intervals are exact runs); errors are put into the plants afterwards: an
``opp`` site (codes 0, 2) breaks both kinds, a ``diff`` site (codes 0, 1) kind 2 only.
``check_case`` states, from the naive walk alone, that unplanted pairs have no segment, that a
case meant to bridge gives another row with its ``bridge_sites`` than with 0, that a case meant
not to gives the same, and that ``length2 <= length1`` still holds.
"""
import dataclasses
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import ibd_cases as ic
from cuking_amd.ibd import IBD_PAIR_DTYPE, IBD_SEGMENT_DTYPE, sort_segments

S = ic.STEP
TWO_STEPS = 2 * S + 37


# ---- the naive restatement -----------------------------------------------------------------------
def runs_of(breaks, num_sites, group):
    """The maximal runs [a, b] of sites of one group without a break, in site order."""
    runs, first = [], None
    for s in range(num_sites):
        if first is not None and group is not None and group[s] != group[s - 1]:
            runs.append((first, s - 1))   # a boundary ends a run, the site stays
            first = None
        if breaks[s]:
            if first is not None:
                runs.append((first, s - 1))
            first = None
        elif first is None:
            first = s
    if first is not None:
        runs.append((first, num_sites - 1))
    return runs


def chains_of(runs, breaks, group, bridge_sites):
    """The chains (A, B, links) of the runs: consecutive runs are linked iff exactly one site
    lies between them (a break), the last site of the first run, the break and the first site of
    the second run lie in one group, and both runs have at least ``bridge_sites`` sites."""
    chains = []
    for k, (a, b) in enumerate(runs):
        linked = False
        if k > 0 and bridge_sites != 0:
            pa, pb = runs[k - 1]
            if a == pb + 2:
                assert breaks[pb + 1]
                one_group = group is None or group[pb] == group[pb + 1] == group[pb + 2]
                linked = one_group and pb - pa + 1 >= bridge_sites and b - a + 1 >= bridge_sites
        if linked:
            first, _, links = chains[-1]
            chains[-1] = (first, b, links + 1)
        else:
            chains.append((a, b, 0))
    return chains


def naive(code, num_sites, index, group, pos, min_sites, min_length, bridge_sites):
    """``(rows, bridged, segments)`` from codes uint8 ``[samples, >= num_sites]``, pairs uint32
    ``[P, 2]``, ``group`` / ``pos`` arrays or None: IBD_PAIR_DTYPE rows, uint32 ``[P, 2]``, the
    sorted IBD_SEGMENT_DTYPE rows."""
    num_stored = code.shape[0]
    rows = np.zeros(len(index), dtype=IBD_PAIR_DTYPE)
    bridged = np.zeros((len(index), 2), dtype=np.uint32)
    segments = []
    for p, (i, j) in enumerate(index):
        rows[p]["sample_i"], rows[p]["sample_j"] = i, j
        if i >= num_stored or j >= num_stored:
            continue
        ci, cj = code[i, :num_sites].astype(int), code[j, :num_sites].astype(int)
        called = (ci != 3) & (cj != 3)
        breaks = {1: called & (np.abs(ci - cj) == 2), 2: called & (ci != cj)}
        for kind in (1, 2):
            count = total = longest = 0
            for a, b, links in chains_of(runs_of(breaks[kind], num_sites, group), breaks[kind],
                                         group, bridge_sites):
                length = int(pos[b]) - int(pos[a]) if pos is not None else b - a
                if b - a + 1 >= min_sites and length >= min_length:
                    count, total, longest = count + 1, total + length, max(longest, length)
                    bridged[p, kind - 1] += links
                    segments.append((p, kind, a, b))
            rows[p][f"segments{kind}"], rows[p][f"length{kind}"] = count, total
            rows[p][f"longest{kind}"] = longest
    return rows, bridged, sort_segments(np.array(segments, dtype=IBD_SEGMENT_DTYPE))


# ---- inputs --------------------------------------------------------------------------------------
def make_diff(code, i, j, s):
    """A site that differs without being an opposite homozygote: codes (0, 1)."""
    code[i, s], code[j, s] = 0, 1


@dataclass(frozen=True)
class BCase(ic.Case):
    """An ibd_cases.Case and: ``bridge``: bridge_sites of the call; ``diffs``: (sample_i,
    sample_j, site) made a diff-only site after the plants and the opps (the case's missing
    sites are put back on top); ``bridges``: the case is built so that the row of list position
    0 differs between ``bridge`` and 0 (True), or so that no row does (False); ``want``: list
    position -> (segments1, segments2, bridged1, bridged2) at ``bridge``."""
    bridge: int = 64
    diffs: tuple = ()
    bridges: bool = True
    want: tuple = ()


def strict(case: BCase) -> ic.Case:
    """The ibd_cases.Case the builders of ibd_cases.py take."""
    return ic.Case(**{f.name: getattr(case, f.name) for f in dataclasses.fields(ic.Case)})


@lru_cache(maxsize=None)
def inputs(case: BCase) -> ic.Inputs:
    inp = ic.inputs(strict(case))
    code = inp.code.copy()
    for i, j, s in case.diffs:
        make_diff(code, i, j, s)
    for sample, s in case.missing:
        code[sample, s] = 3
    return dataclasses.replace(inp, case=case, code=code)


@lru_cache(maxsize=None)
def reference(case: BCase, bridge=None):
    inp = inputs(case)
    return naive(inp.code, case.sites, inp.index, inp.group, inp.pos, case.min_sites,
                 case.min_length, case.bridge if bridge is None else bridge)


def check_case(case: BCase):
    """What the case states about itself, from the naive restatement alone."""
    inp = inputs(case)
    rows, bridged, _ = reference(case)
    plain, none, _ = reference(case, 0)
    quiet = rows[~inp.planted]
    assert not quiet["segments1"].any() and not quiet["segments2"].any(), \
        f"{case.name}: an unplanted pair has a segment at min_sites = {case.min_sites}"
    assert not bridged[~inp.planted].any() and not none.any()
    if case.bridges:
        assert rows[0].tobytes() != plain[0].tobytes() and bridged[0].any(), case.name
    else:
        assert rows.tobytes() == plain.tobytes() and not bridged.any(), case.name
    for at, want in case.want:
        got = (int(rows[at]["segments1"]), int(rows[at]["segments2"]), int(bridged[at, 0]),
               int(bridged[at, 1]))
        assert got == want, (case.name, at, got, want)
    assert (rows["length2"] <= rows["length1"]).all()
    assert (rows["segments1"] >= (bridged[:, 0] > 0)).all()


def run_host(case: BCase, ones_padding=False, max_segments=None):
    """``(rows, segments, bridged)`` of the host twin."""
    from cuking_amd.ibd import ibd_segments_raw_host
    inp = inputs(case)
    return ibd_segments_raw_host(inp.bits(ones_padding), inp.wps, case.sites, inp.pairs,
                                 inp.group, inp.pos, case.min_sites, case.min_length,
                                 segments=True, max_segments=max_segments,
                                 bridge_sites=case.bridge)


def check_against(case: BCase, rows, segments, bridged, what="rows"):
    """A backend's rows, bridged counts and segment list against the naive walk, bytewise."""
    want_rows, want_bridged, want_segments = reference(case)
    assert rows.dtype == IBD_PAIR_DTYPE and bridged.dtype == np.uint32
    for name in IBD_PAIR_DTYPE.names:
        assert np.array_equal(rows[name], want_rows[name]), (case.name, what, name)
    assert rows.tobytes() == want_rows.tobytes(), (case.name, what)
    assert bridged.shape == want_bridged.shape, (case.name, what)
    assert bridged.tobytes() == want_bridged.tobytes(), (case.name, what, bridged, want_bridged)
    assert sort_segments(segments).tobytes() == want_segments.tobytes(), (case.name, what)


def one(first, last, *breaks, pair=(0, 1), kind=2):
    """A plant of ``pair`` with opp sites inside: (plants, opps)."""
    return (pair + (first, last, kind),), tuple(pair + (s,) for s in breaks)


def make(name, samples, sites, planted, **kw):
    """A BCase from a list of ``one(...)`` results."""
    plants = sum((p for p, _ in planted), ())
    opps = sum((o for _, o in planted), ()) + kw.pop("opps", ())
    return BCase(name, samples, sites, plants=plants, opps=opps, **kw)


PAIRS = ((0, 1), (2, 3), (4, 5), (6, 7), (8, 9))


def edge_runs(bridge):
    """Four pairs: the left run exactly ``bridge`` sites and one less, the same on the right."""
    left, right = 100 + bridge, 500 - bridge
    return make(f"runs of exactly {bridge} sites, and one less", 8, 700,
                [one(100, left + 200, left, pair=PAIRS[0]),
                 one(100, left + 199, left - 1, pair=PAIRS[1]),
                 one(250, 500, right, pair=PAIRS[2]),
                 one(251, 500, right + 1, pair=PAIRS[3])],
                min_sites=150, bridge=bridge,
                want=((0, (1, 1, 1, 1)), (1, (1, 1, 0, 0)), (2, (1, 1, 1, 1)), (3, (1, 1, 0, 0))))


def pending(sites):
    """A chain that is still pending when the scan ends: it reaches the last site."""
    return make(f"a chain pending at the end of {sites} sites", 8, sites,
                [one(sites - 300, sites - 1, sites - 150)], min_sites=200,
                want=((0, (1, 1, 1, 1)),))


CASES = [
    # ---- basic bridging
    make("one opp inside a kind-2 plant", 8, 700, [one(100, 600, 300)], min_sites=150,
         want=((0, (1, 1, 1, 1)),)),
    edge_runs(64),
    edge_runs(100),
    make("min_sites met by the chain only: 100 + 1 + 100 sites", 8, 700, [one(100, 300, 200)],
         min_sites=150, want=((0, (1, 1, 1, 1)),)),
    # (positions advance by one over the plants: the runs of (0, 1) span 99 each and the chain
    #  200; the chain of (2, 3) has 141 sites and spans 140)
    make("min_length decided on the chain's span", 8, 900,
         [one(100, 300, 200), one(400, 540, 470, pair=PAIRS[1])],
         min_sites=120, min_length=150, pos=9, slow=((90, 310), (390, 550)),
         want=((0, (1, 1, 1, 1)), (1, (0, 0, 0, 0)))),
    # ---- break positions at word and step edges
    make("breaks at bit 63, at bit 0, at the last site of a step and at the first of the next", 10,
         TWO_STEPS,
         [one(100, 600, 319), one(100, 600, 320, pair=PAIRS[1]),
          one(S - 200, S + 200, S - 1, pair=PAIRS[2]), one(S - 200, S + 200, S, pair=PAIRS[3]),
          one(S - 300, S + 63, S - 1, pair=PAIRS[4])],
         min_sites=200, want=tuple((k, (1, 1, 1, 1)) for k in range(5))),
    # (two links in step 0, then the chain waits through step 1, where this pair has no event)
    make("three runs, pending across a whole step, closed by the end", 8, TWO_STEPS,
         [one(S - 400, TWO_STEPS - 1, S - 200, S - 100)], min_sites=200,
         want=((0, (1, 1, 2, 2)),)),
    # (the run behind the break in step 2 has 36 sites at most: not linked, the chain of step 0
    #  is tested with its one link when that run closes)
    make("a chain carried across a whole step, ended by a run that is not linked", 8, TWO_STEPS,
         [one(S - 400, TWO_STEPS - 1, S - 200, 2 * S + 10)], min_sites=200,
         want=((0, (1, 1, 1, 1)),)),
    # (breaks in step 0 and in step 2, all three runs linked: the run behind the second break
    #  needs 64 sites, so this one shape takes 2 * 4096 + 200 sites)
    make("three runs with breaks in step 0 and in step 2", 8, 2 * S + 200,
         [one(S - 400, 2 * S + 199, S - 200, 2 * S + 100)], min_sites=200, crowd=4,
         want=((0, (1, 1, 2, 2)),)),
    pending(S), pending(S + 1), pending(640), pending(TWO_STEPS),
    # ---- breaks that must not be bridged
    make("adjacent breaks", 8, 700, [one(100, 600, 300, 301)], min_sites=150, bridges=False,
         want=((0, (2, 2, 0, 0)),)),
    make("breaks 40 apart", 8, 700, [one(100, 600, 300, 340)], min_sites=150, bridges=False,
         want=((0, (2, 2, 0, 0)),)),
    make("a break that is the last, and one that is the first site of a group", 8, 700,
         [one(100, 600, 300), one(100, 600, 301, pair=PAIRS[1])], min_sites=150, bounds=(301,),
         bridges=False, want=((0, (2, 2, 0, 0)), (1, (2, 2, 0, 0)))),
    make("breaks at site 0 and at the last site", 8, 700,
         [one(0, 300, 0), one(400, 699, 699, pair=PAIRS[1])], min_sites=150, bridges=False,
         want=((0, (1, 1, 0, 0)), (1, (1, 1, 0, 0)))),
    # (a group that starts right in front of or behind the break's neighbours leaves a run of
    #  one site there: too short to link)
    make("a group starts at the last site in front of a break", 8, 700, [one(100, 600, 300)],
         min_sites=150, bounds=(299,), bridges=False, want=((0, (2, 2, 0, 0)),)),
    make("a group starts one site behind the first site after a break", 8, 700,
         [one(100, 600, 300)], min_sites=150, bounds=(302,), bridges=False,
         want=((0, (2, 2, 0, 0)),)),
    # ---- long chains
    make("five breaks 70 sites apart, 64 sites bridge them", 8, 700,
         [one(100, 600, 200, 270, 340, 410, 480)], min_sites=150, want=((0, (1, 1, 5, 5)),)),
    make("five breaks 70 sites apart, 80 sites link nothing", 8, 700,
         [one(100, 600, 200, 270, 340, 410, 480)], min_sites=150, bridge=80, bridges=False,
         want=((0, (0, 0, 0, 0)),)),
    # ---- missing sites
    # (the left run of (0, 1) is 236 .. 299: exactly 64 sites, two of them missing)
    make("missing beside a break, a missing word inside a chain, a missing would-be break", 8,
         900, [one(236, 600, 300), one(100, 700, 500, 600, pair=PAIRS[1])], min_sites=150,
         missing=((0, 299), (1, 301), (1, 236), (3, 600)) + tuple((2, s) for s in range(192, 256)),
         want=((0, (1, 1, 1, 1)), (1, (1, 1, 1, 1)))),
    # ---- kinds
    BCase("diff-only errors: kind 2 bridges, kind 1 is one untouched run", 8, 700, min_sites=150,
          plants=((0, 1, 100, 600, 2), (2, 3, 100, 600, 1)), diffs=((0, 1, 300), (0, 1, 450)),
          opps=((2, 3, 350),), want=((0, (1, 1, 0, 2)), (1, (1, 0, 1, 0)))),
    # ---- padding and strides
    make("sixteen samples, padded width, records", 16, 3000,
         [one(0, 2999, 1000, 2000, pair=(0, 9)), one(500, 2500, 1500, pair=(2, 11), kind=1),
          one(1000, 1179, 1090, pair=(4, 15))],
         min_sites=180, tight=False, stride=24,
         want=((0, (1, 1, 2, 2)), (1, (1, 0, 1, 0)), (2, (1, 1, 1, 1)))),
]

FUZZ_SEEDS = ic.FUZZ_SEEDS


def fuzz_case(seed: int) -> BCase:
    """ibd_cases.fuzz_case(seed) with random opp and diff sites sprinkled into its plants and a
    bridge_sites drawn from 64 .. 150."""
    base = ic.fuzz_case(seed)
    rng = np.random.default_rng(5000 + seed)
    opps, diffs = [], []
    for i, j, first, last, _ in base.plants:
        for s in rng.integers(first, last + 1, size=int(rng.integers(1, 7))):
            (opps if rng.random() < 0.5 else diffs).append((i, j, int(s)))
    fields = {f.name: getattr(base, f.name) for f in dataclasses.fields(ic.Case)}
    fields.update(opps=tuple(opps), diffs=tuple(diffs), bridge=int(rng.integers(64, 151)))
    return BCase(**fields)


def check_fuzz_case(case: BCase):
    """The fuzz states less about itself: unplanted pairs are quiet, length2 <= length1."""
    inp = inputs(case)
    rows, bridged, _ = reference(case)
    assert not rows[~inp.planted]["segments1"].any() and not bridged[~inp.planted].any()
    assert (rows["length2"] <= rows["length1"]).all()


def bridged_arguments(inp, pointers, bridge_sites, **over):
    """The argument list of cuking_ibd_pairs_bridged_host from that of the strict call
    (ibd_cases.raw_arguments): bridge_sites behind min_length, ``pointers["bridged"]`` behind
    out."""
    a = list(ic.raw_arguments(inp, pointers, **over))
    return (*a[:8], bridge_sites, *a[8:12], pointers["bridged"], *a[12:])
