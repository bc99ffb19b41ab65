"""Runs of homozygosity per sample: the cases the host and the GPU tests share, a seeded fuzz
generator, and the NAIVE reference both backends are compared with -- a walk over the code matrix
site by site in plain Python, with the linking of runs written out.  It knows no words and
nothing of csrc/king_ibd.h.

Genotypes are drawn independently per sample with allele frequencies in 0.2 .. 0.5, so a sample
is het at a third to a half of its sites and its runs stay far below 64 sites (a chance of
0.68^64 per start): every case asserts from the naive walk that a sample without a plant has no
segment (``check_case``).  A plant replaces the hets of ``first .. last`` by homozygotes and makes
the site in front of and behind it het, so the planted run is exactly the interval; single hets
and missing sites are put in afterwards.
"""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import cuking_amd
from cuking_amd.ibd import IBD_SEGMENT_DTYPE
from cuking_amd.roh import ROH_SAMPLE_DTYPE

STEP = 4096            # sites of one wavefront step: 64 lanes x 64 sites (king_ibd.hip)
S = STEP
TWO_STEPS = 2 * S + 37
MIN = 64               # CUKING_IBD_MIN_SITES
SITE_COUNTS = {1, 63, 64, 65, S, S + 1, TWO_STEPS}


def sort_rows(segments):
    return np.sort(segments, order=["pair", "kind", "first_site"])


# ---- the naive reference -------------------------------------------------------------------------
def naive_runs(code, num_sites, group):
    """The maximal runs [a, b] of sites of one group without a het (code 1), in site order."""
    runs, first = [], None
    for s in range(num_sites):
        if first is not None and group is not None and group[s] != group[s - 1]:
            runs.append((first, s - 1))     # a boundary ends a run, the site stays
            first = None
        if code[s] == 1:
            if first is not None:
                runs.append((first, s - 1))
            first = None
        elif first is None:
            first = s
    if first is not None:
        runs.append((first, num_sites - 1))
    return runs


def naive_chains(runs, group, bridge_sites):
    """(A, B, links): consecutive runs [a, b], [a2, b2] are linked iff a2 == b + 2 (one site,
    a het, lies between them), the sites b, b + 1, b + 2 lie in one group and both runs have
    at least ``bridge_sites`` sites; a chain is a maximal sequence of linked runs."""
    chains = []
    for k, (a2, b2) in enumerate(runs):
        linked = False
        if k > 0 and bridge_sites != 0:
            a, b = runs[k - 1]
            if a2 == b + 2:
                one_group = group is None or group[b] == group[b + 1] == group[b + 2]
                linked = one_group and b - a + 1 >= bridge_sites and b2 - a2 + 1 >= bridge_sites
        if linked:
            first, _, links = chains[-1]
            chains[-1] = (first, b2, links + 1)
        else:
            chains.append((a2, b2, 0))
    return chains


def naive(code, num_sites, listed, group, pos, min_sites, min_length, bridge_sites):
    """``(rows, segments)``: ROH_SAMPLE_DTYPE rows in list order and the sorted IBD_SEGMENT_DTYPE
    rows, from codes uint8 ``[samples, >= num_sites]`` (0 hom-ref, 1 het, 2 hom-var, 3 missing)
    and the list of samples (None: all of them)."""
    num_stored = code.shape[0]
    if listed is None:
        listed = range(num_stored)
    rows = np.zeros(len(listed), dtype=ROH_SAMPLE_DTYPE)
    segments = []
    for r, sample in enumerate(listed):
        rows[r]["sample"] = sample
        if sample >= num_stored:
            continue
        count = total = longest = forgiven = 0
        runs = naive_runs(code[int(sample)], num_sites, group)
        for a, b, links in naive_chains(runs, group, bridge_sites):
            length = int(pos[b]) - int(pos[a]) if pos is not None else b - a
            if b - a + 1 >= min_sites and length >= min_length:
                count, total, longest = count + 1, total + length, max(longest, length)
                forgiven += links
                segments.append((r, 0, a, b))
        rows[r]["segments"], rows[r]["length"], rows[r]["longest"] = count, total, longest
        rows[r]["bridged"] = forgiven
    return rows, sort_rows(np.array(segments, dtype=IBD_SEGMENT_DTYPE))


# ---- inputs --------------------------------------------------------------------------------------
def pack_codes(code, plane_words, ones_padding=False):
    """The sample-major bitset uint64 ``[samples, 2 plane_words]`` of codes ``[samples, sites]``:
    het plane then hom plane, site s at bit s & 63 of word s >> 6; the bits from ``sites`` on are
    all clear, or all set."""
    n, m = code.shape
    planes = np.full((n, 2, plane_words * 64), 1 if ones_padding else 0, dtype=np.uint8)
    planes[:, 0, :m] = code & 1
    planes[:, 1, :m] = code >> 1
    packed = np.packbits(planes, axis=2, bitorder="little")
    return np.ascontiguousarray(packed).view("<u8").reshape(n, 2 * plane_words)


@dataclass(frozen=True)
class Case:
    """``plants``: (sample, first, last) made free of hets, with a het in front and behind;
    ``hets`` / ``missing``: (sample, site) made het / missing afterwards, in that order;
    ``all_missing`` / ``all_het``: samples that are nothing else; ``bounds``: the sites that start
    a new group; ``pos``: None (the index) or the largest step between neighbours; ``slow``:
    (first, last) ranges whose positions advance by one; ``tight``: plane_words = ceil(sites /
    64), else the library's padded width; ``listed``: the call gets an explicit list (all
    samples shuffled, repeats, indices >= num_stored), else the null list; ``bridge``:
    bridge_sites of the call; ``want``: sample -> (segments, bridged) at ``bridge``; ``strict``:
    sample -> segments at bridge_sites = 0."""
    name: str
    samples: int
    sites: int
    min_sites: int = MIN
    min_length: int = 0
    bridge: int = 0
    plants: tuple = ()
    hets: tuple = ()
    missing: tuple = ()
    all_missing: tuple = ()
    all_het: tuple = ()
    bounds: tuple = ()
    pos: object = None
    slow: tuple = ()
    tight: bool = True
    listed: bool = True
    seed: int = 1
    want: tuple = ()
    strict: tuple = ()


@dataclass
class Inputs:
    case: Case
    code: np.ndarray
    wps: int
    listed: object        # uint32 [L] or None
    planted: np.ndarray   # bool [samples]: may have segments
    group: object
    pos: object

    def bits(self, ones_padding=False):
        return pack_codes(self.code, self.wps // 2, ones_padding)


def draw_codes(rng, samples, sites, missing=0.02):
    af = rng.uniform(0.2, 0.5, size=sites)
    code = ((rng.random((samples, sites)) < af).astype(np.uint8) +
            (rng.random((samples, sites)) < af).astype(np.uint8))
    code[rng.random((samples, sites)) < missing] = 3
    return code


def plant(code, sample, first, last, rng):
    seg = code[sample, first:last + 1]
    het = seg == 1
    seg[het] = 2 * rng.integers(0, 2, size=int(het.sum()))
    for s in (first - 1, last + 1):
        if 0 <= s < code.shape[1]:
            code[sample, s] = 1


@lru_cache(maxsize=None)
def inputs(case: Case) -> Inputs:
    rng = np.random.default_rng(case.seed)
    code = draw_codes(rng, case.samples, case.sites)
    for sample, first, last in case.plants:
        plant(code, sample, first, last, rng)
    for sample, s in case.hets:
        code[sample, s] = 1
    for sample, s in case.missing:
        code[sample, s] = 3
    for sample in case.all_missing:
        code[sample, :] = 3
    for sample in case.all_het:
        code[sample, :] = 1
    plane_words = max(1, -(-case.sites // 64))
    wps = 2 * plane_words if case.tight else max(cuking_amd.words_per_sample(case.sites),
                                                 2 * plane_words)
    group = pos = None
    if case.bounds:
        group = np.zeros(case.sites, dtype=np.int32)
        for b in case.bounds:
            group[b:] += 7   # (any change of value is a boundary)
    if case.pos is not None:
        steps = rng.integers(0, case.pos + 1, size=case.sites).astype(np.int64)
        for first, last in case.slow:
            steps[first:last + 1] = 1
        pos = np.cumsum(steps)
        for b in case.bounds:   # a new group may start anywhere, below its predecessor too
            pos[b:] -= pos[b] - int(rng.integers(0, 50))
        pos = pos.astype(np.uint32)
    n = case.samples
    listed = None
    if case.listed:   # every sample in shuffled order, three repeats, two indices outside
        order = rng.permutation(n)
        listed = np.concatenate([order[: n // 2], [n, order[0]], order[n // 2:],
                                 [0xFFFFFFFF, order[-1], 0]]).astype(np.uint32)
    planted = np.zeros(n, dtype=bool)
    planted[[p[0] for p in case.plants] + list(case.all_missing)] = True
    return Inputs(case, code, wps, listed, planted, group, pos)


@lru_cache(maxsize=None)
def reference(case: Case, bridge=None):
    inp = inputs(case)
    return naive(inp.code, case.sites, inp.listed, inp.group, inp.pos, case.min_sites,
                 case.min_length, case.bridge if bridge is None else bridge)


def rows_of(inp: Inputs, rows, sample):
    listed = np.arange(inp.case.samples) if inp.listed is None else inp.listed
    return rows[listed == sample]


def check_case(case: Case):
    """What the case states about itself, from the naive walk alone."""
    inp = inputs(case)
    rows, segments = reference(case)
    plain, _ = reference(case, 0)
    assert len(segments) == int(rows["segments"].sum())
    assert not plain["bridged"].any() and (rows["segments"] >= (rows["bridged"] > 0)).all()
    assert (rows["longest"] <= rows["length"]).all()
    for sample in range(case.samples):
        mine = rows_of(inp, rows, sample)
        assert len(mine) >= 1 and all(m.tobytes() == mine[0].tobytes() for m in mine)
        if not inp.planted[sample]:
            assert not mine["segments"].any() and not rows_of(inp, plain, sample)["segments"] \
                .any(), f"{case.name}: sample {sample} has a segment without a plant"
    for sample, want in case.want:
        got = rows_of(inp, rows, sample)[0]
        assert (int(got["segments"]), int(got["bridged"])) == want, (case.name, sample, got)
    for sample, want in case.strict:
        assert int(rows_of(inp, plain, sample)[0]["segments"]) == want, (case.name, sample)
    if inp.listed is not None:   # indices >= num_stored: zeros, echoed
        outside = rows[inp.listed >= case.samples]
        assert len(outside) == 2 and not outside["segments"].any() and \
            not outside["length"].any()
        assert outside["sample"].tolist() == [case.samples, 0xFFFFFFFF]


def run_host(case: Case, ones_padding=False, max_segments=None, bridge=None, listed=True):
    """``(rows, segments)`` of the host twin; ``listed`` False: the null list instead."""
    from cuking_amd.roh import roh_segments_raw_host
    inp = inputs(case)
    return roh_segments_raw_host(inp.bits(ones_padding), inp.wps, case.sites,
                                 inp.listed if listed else None, inp.group, inp.pos,
                                 case.min_sites, case.min_length,
                                 case.bridge if bridge is None else bridge, segments=True,
                                 max_segments=max_segments)


def check_against(case: Case, rows, segments, what="rows", bridge=None):
    """A backend's rows and segment list against the naive walk, bytewise."""
    want_rows, want_segments = reference(case, bridge)
    assert rows.dtype == ROH_SAMPLE_DTYPE
    for name in ROH_SAMPLE_DTYPE.names:
        assert np.array_equal(rows[name], want_rows[name]), (case.name, what, name)
    assert rows.tobytes() == want_rows.tobytes(), (case.name, what)
    assert sort_rows(segments).tobytes() == want_segments.tobytes(), (case.name, what)


CASES = [
    # ---- the shapes: one word, a word edge, one step, the carry between steps
    Case("1 site", 4, 1, all_missing=(1,), all_het=(2,)),
    Case("63 sites", 5, 63, plants=((0, 0, 62),), all_missing=(1,), want=((0, (0, 0)), (1, (0, 0)))),
    Case("64 sites: a run that ends at num_sites, closed beyond the plane", 6, 64,
         plants=((0, 0, 63), (3, 1, 63)), all_missing=(1,), all_het=(2,),
         want=((0, (1, 0)), (1, (1, 0)), (2, (0, 0)), (3, (0, 0)))),
    Case("64 sites, padded planes, the null list", 6, 64, plants=((0, 0, 63),), tight=False,
         listed=False, want=((0, (1, 0)),)),
    Case("65 sites: a het at the first site, a het at the last site", 7, 65,
         plants=((0, 1, 64), (1, 0, 63), (2, 1, 63)),
         want=((0, (1, 0)), (1, (1, 0)), (2, (0, 0)))),
    Case("4096 sites: one step, the close bit in the next", 6, S, min_sites=200,
         plants=((0, 0, S - 1), (1, 3000, S - 1)), all_missing=(2,),
         want=((0, (1, 0)), (1, (1, 0)), (2, (1, 0)))),
    Case("4097 sites: a run crossing the step edge", 6, S + 1, min_sites=200,
         plants=((0, 3800, S), (1, 100, 4000), (2, S - 100, S)), listed=False,
         want=((0, (1, 0)), (1, (1, 0)), (2, (0, 0)))),
    # (sample 3: the chain of step 0 waits through step 1 and is ended in step 2 by a run of 26
    #  sites that is not linked; sample 4: both hets are bridged, the chain is pending at the end;
    #  twelve samples are three workgroups: a launch cap of one splits the launch)
    Case("two steps and 37 sites: the carry, and a chain carried across a step", 12, TWO_STEPS,
         min_sites=200, bridge=64,
         plants=((0, 4000, TWO_STEPS - 1), (1, 17, 2 * S + 5), (2, S - 100, S + 100),
                 (3, S - 400, TWO_STEPS - 1), (4, S - 400, TWO_STEPS - 1)),
         hets=((3, S - 200), (3, 2 * S + 10), (4, S - 200), (4, S - 100)), all_missing=(5,),
         want=((0, (1, 0)), (1, (1, 0)), (2, (1, 0)), (3, (1, 1)), (4, (1, 2)), (5, (1, 0))),
         strict=((3, 2), (4, 2))),
    # ---- groups
    Case("a group boundary inside a run", 6, 700, min_sites=150, bounds=(300,),
         plants=((0, 100, 600),), all_missing=(1,), want=((0, (2, 0)), (1, (2, 0)))),
    Case("every word a group", 6, 640, bounds=tuple(range(64, 640, 64)),
         plants=((0, 0, 639), (1, 64, 300)), want=((0, (10, 0)), (1, (3, 0)))),
    Case("a group boundary on a step edge and on a word edge", 6, S + 900, min_sites=160,
         bounds=(200, 448, S), plants=((0, 10, S + 800),), want=((0, (4, 0)),)),
    # ---- missing sites
    # (200 and 500 are the ends of the run of sample 0; 899, the last site, ends that of sample 1)
    Case("missing inside a run and at its ends, a missing word", 6, 900, min_sites=150,
         plants=((0, 200, 500), (1, 600, 898), (2, 100, 400)),
         missing=((0, 200), (0, 350), (0, 351), (0, 500), (1, 899), (1, 600)) +
         tuple((2, s) for s in range(192, 256)),
         want=((0, (1, 0)), (1, (1, 0)), (2, (1, 0)))),
    Case("a wholly missing and a wholly het sample", 6, 700, min_sites=150, bounds=(300,),
         all_missing=(0,), all_het=(1,), want=((0, (2, 0)), (1, (0, 0)))),
    # ---- positions
    # (positions advance by one over 90 .. 300: the run of sample 0 has 191 sites and spans 190;
    #  that of sample 2 spans more than 500 with 146 sites)
    Case("min_length decides both ways", 6, 1500, min_sites=150, min_length=500, pos=12,
         slow=((90, 300),), plants=((0, 100, 290), (1, 400, 1200), (2, 301, 446)),
         want=((0, (0, 0)), (1, (1, 0)), (2, (0, 0)))),
    Case("positions with groups", 6, 2000, min_sites=150, min_length=300, pos=4,
         bounds=(640, 1301), plants=((0, 500, 900), (1, 1301, 1999))),
    # ---- bridged hets
    Case("100 + het + 100 sites pass min_sites = 150 as a chain only", 6, 700, min_sites=150,
         bridge=64, plants=((0, 100, 300),), hets=((0, 200),), want=((0, (1, 1)),),
         strict=((0, 0),)),
    Case("two adjacent hets are never bridged", 6, 700, min_sites=150, bridge=64,
         plants=((0, 100, 600),), hets=((0, 300), (0, 301)), want=((0, (2, 0)),),
         strict=((0, 2),)),
    Case("a het that is the last, and one that is the first site of a group", 6, 700,
         min_sites=150, bridge=64, bounds=(301,), plants=((0, 100, 600), (1, 100, 600)),
         hets=((0, 300), (1, 301)), want=((0, (2, 0)), (1, (2, 0)))),
    # (sample 0: the run 100 .. 162 has 63 sites; sample 1: 100 .. 163 has 64)
    Case("a run of 63 sites beside a het is not linked, one of 64 is", 6, 700, min_sites=150,
         bridge=64, plants=((0, 100, 400), (1, 100, 400)), hets=((0, 163), (1, 164)),
         want=((0, (1, 0)), (1, (1, 1))), strict=((0, 1), (1, 1))),
    Case("hets at bit 63, at bit 0, at the last site of a step and the first of the next", 8,
         TWO_STEPS, min_sites=200, bridge=64,
         plants=((0, 100, 600), (1, 100, 600), (2, S - 200, S + 200), (3, S - 200, S + 200)),
         hets=((0, 319), (1, 320), (2, S - 1), (3, S)), tight=False,
         want=tuple((k, (1, 1)) for k in range(4))),
    Case("five hets 70 sites apart: 64 sites bridge them all", 6, 700, min_sites=150, bridge=64,
         plants=((0, 100, 600),), hets=tuple((0, s) for s in (200, 270, 340, 410, 480)),
         want=((0, (1, 5)),), strict=((0, 0),)),
    Case("five hets 70 sites apart: 80 sites link nothing", 6, 700, min_sites=150, bridge=80,
         plants=((0, 100, 600),), hets=tuple((0, s) for s in (200, 270, 340, 410, 480)),
         want=((0, (0, 0)),)),
    Case("a missing site beside a bridged het, a missing would-be het", 6, 900, min_sites=150,
         bridge=64, plants=((0, 236, 600), (1, 100, 700)), hets=((0, 300), (1, 500), (1, 600)),
         missing=((0, 299), (0, 301), (1, 600)), want=((0, (1, 1)), (1, (1, 1)))),
    Case("hets at site 0 and at the last site", 6, 700, min_sites=150, bridge=64,
         plants=((0, 0, 300), (1, 400, 699)), hets=((0, 0), (1, 699)),
         want=((0, (1, 0)), (1, (1, 0)))),
    Case("a chain pending at the end of one step", 6, S, min_sites=200, bridge=100,
         plants=((0, S - 300, S - 1),), hets=((0, S - 150),), want=((0, (1, 1)),)),
]

FUZZ_SEEDS = range(40)


def fuzz_case(seed: int) -> Case:
    """A small random case over the same parameters."""
    rng = np.random.default_rng(7000 + seed)
    samples = int(rng.integers(4, 21))
    sites = int(rng.choice([int(rng.integers(65, 700)), int(rng.integers(700, 2 * S + 200))]))
    min_sites = int(rng.integers(64, 200)) if sites < 700 else int(rng.integers(150, 300))
    bounds = tuple(sorted({int(b) for b in rng.integers(1, sites, size=int(rng.integers(0, 4)))}))
    plants, hets = [], []
    for k in range(int(rng.integers(1, min(samples, 5) + 1))):
        length = int(rng.integers(max(1, min_sites - 20), max(min_sites + 1, sites // 2)))
        first = int(rng.integers(0, max(1, sites - length)))
        last = min(sites - 1, first + length - 1)
        plants.append((k, first, last))
        hets += [(k, int(s)) for s in rng.integers(first, last + 1, size=int(rng.integers(0, 6)))]
    missing = tuple((int(rng.integers(0, samples)), int(rng.integers(0, sites)))
                    for _ in range(20))
    pos = None if rng.random() < 0.4 else int(rng.integers(1, 9))
    min_length = 0 if pos is None or rng.random() < 0.5 else int(rng.integers(100, 600))
    bridge = 0 if rng.random() < 0.25 else int(rng.integers(64, 151))
    return Case(f"fuzz {seed}", samples, sites, min_sites, min_length, bridge, tuple(plants),
                tuple(hets), missing, bounds=bounds, pos=pos, tight=bool(rng.random() < 0.5),
                listed=bool(rng.random() < 0.7), seed=9000 + seed)


def check_fuzz_case(case: Case):
    """The fuzz states less about itself: samples without a plant are quiet."""
    inp = inputs(case)
    rows, segments = reference(case)
    for sample in np.flatnonzero(~inp.planted):
        assert not rows_of(inp, rows, sample)["segments"].any()
    assert len(segments) == int(rows["segments"].sum())


# ---- the refusals through the raw ABI ------------------------------------------------------------
# name -> (the arguments replaced (see raw_arguments), the status, a word of the message)
REFUSALS = {
    "words_per_sample zero": (dict(wps=0), "INVALID", "positive even"),
    "words_per_sample odd": (dict(wps=3), "INVALID", "positive even"),
    "sites beyond the planes": (dict(num_sites=64 * 3 + 1), "INVALID", "do not fit"),
    "min_sites below 64": (dict(min_sites=63), "INVALID", "min_sites (63) must be at least 64"),
    "bridge_sites 1": (dict(bridge=1), "INVALID", "bridge_sites (1) must be 0 or at least 64"),
    "bridge_sites 63": (dict(bridge=63), "INVALID", "bridge_sites (63) must be 0 or at least 64"),
    "null bits": (dict(bits=None), "INVALID", "null bits pointer"),
    "null out": (dict(out=None), "INVALID", "null out pointer"),
    "null segments with room asked": (dict(segments=None), "INVALID", "null segments pointer"),
    "segments without a counter": (dict(found=None), "INVALID", "needs a num_segments pointer"),
    "pos decreases inside a group": (dict(pos="decreasing"), "PRECONDITION",
                                     "pos must not decrease inside a group, but pos[100] = 5 "
                                     "follows pos[99] = 99"),
}
REFUSAL_CASE = Case("refusals", 6, 180, plants=((0, 20, 150),))


def raw_arguments(inp, pointers, **over):
    """The argument list of cuking_roh_samples_host (the device call adds ctx and stream around
    it): ``pointers`` holds bits, group, pos, samples, out, segments, found."""
    count = inp.case.samples if inp.listed is None else len(inp.listed)
    a = dict(pointers, num_stored=inp.case.samples, wps=inp.wps, num_sites=inp.case.sites,
             min_sites=inp.case.min_sites, min_length=inp.case.min_length,
             bridge=inp.case.bridge, num_samples=count, max_segments=16)
    a.update(over)
    return (a["bits"], a["num_stored"], a["wps"], a["num_sites"], a["group"], a["pos"],
            a["min_sites"], a["min_length"], a["bridge"], a["samples"], a["num_samples"],
            a["out"], a["segments"], a["max_segments"], a["found"])


# ---- the end-to-end cohort -----------------------------------------------------------------------
# 24 samples x 6000 sites in 3 groups of 2000, het rate about 0.3 and 1 % missing; six samples get
# an autozygous stretch of 600 .. 2000 sites inside one group (its hets replaced by a homozygote,
# the site in front of and behind it made het); then one planted genotype in 400 is flipped to
# het: the genotyping errors that split a true run.
E2E_SAMPLES, E2E_SITES, E2E_GROUPS, E2E_PLANTED = 24, 6000, 3, 6
E2E_MIN_SITES, E2E_BRIDGE, E2E_ERROR_RATE = 256, 64, 1 / 400
# Chosen on the CPU as the first seed from 0 at which the host twin meets the three conditions of
# check_e2e: at seed 2 the strict call finds 1 of the 6 stretches and bridge_sites = 64 all 6,
# with 12 bridged hets.  (At seeds 0 and 1 bridging finds 4 and 3 of the 6: one het per bridge
# does not forgive errors that lie closer than 64 sites to each other.)
E2E_SEED = 2


@lru_cache(maxsize=None)
def e2e_cohort(seed=E2E_SEED):
    """``(code, group, stretches)``: codes uint8 [24, 6000], int32 groups, and the planted
    (sample, first, last)."""
    rng = np.random.default_rng(seed)
    n, m = E2E_SAMPLES, E2E_SITES
    code = np.where(rng.random((n, m)) < 0.3, 1, 2 * rng.integers(0, 2, size=(n, m))) \
        .astype(np.uint8)
    code[rng.random((n, m)) < 0.01] = 3
    per_group = m // E2E_GROUPS
    group = (np.arange(m) // per_group).astype(np.int32)
    stretches = []
    for sample in rng.permutation(n)[:E2E_PLANTED]:
        length = int(rng.integers(600, per_group - 1))
        first = int(rng.integers(0, E2E_GROUPS)) * per_group + \
            int(rng.integers(1, per_group - length))
        plant(code, sample, first, first + length - 1, rng)
        stretches.append((int(sample), first, first + length - 1))
    for sample, first, last in stretches:
        errors = first + np.flatnonzero(rng.random(last - first + 1) < E2E_ERROR_RATE)
        code[sample, errors] = 1
    return code, group, tuple(stretches)


def e2e_found(got, stretches):
    """How many planted stretches ``got`` (a ROHSamples of all samples with its segment list)
    finds: a segment of the sample inside the planted bounds that covers all of the stretch but
    fewer than 64 sites at either end (a het closer than bridge_sites to an end of a stretch has
    too short a run beside it to be bridged)."""
    found = 0
    for sample, first, last in stretches:
        mine = got.segment_list[got.segment_list["pair"] == sample]
        found += any(first <= int(s["first_site"]) < first + 64 and
                     last - 64 < int(s["last_site"]) <= last for s in mine)
    return found


def check_e2e(strict, bridged, stretches):
    """The three conditions of the end-to-end check, on the ROHSamples of the null list."""
    planted = np.zeros(E2E_SAMPLES, dtype=bool)
    planted[[s[0] for s in stretches]] = True
    assert e2e_found(strict, stretches) < len(stretches) == E2E_PLANTED
    assert e2e_found(bridged, stretches) == len(stretches)
    for got in (strict, bridged):
        assert not got.segments[~planted].any() and not got.length[~planted].any()
        # (every segment of a planted sample lies inside its stretch)
        for sample, first, last in stretches:
            mine = got.segment_list[got.segment_list["pair"] == sample]
            assert (mine["first_site"] >= first).all() and (mine["last_site"] <= last).all()
    assert bridged.bridged[planted].sum() > 0 and not strict.bridged.any()
    assert (bridged.froh()[planted] > strict.froh()[planted]).any()
