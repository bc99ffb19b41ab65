"""IBD segments for listed pairs: the cases the host and the GPU tests share, and the NAIVE
restatement both are compared with -- decode to codes, walk the sites one by one; it knows no
words and nothing of csrc/king_ibd.h.

Genotypes are drawn independently per sample with allele frequencies in 0.2 .. 0.5, so that a
pair of unrelated samples meets opposite homozygotes every ten sites or so and its runs stay far
below the case's ``min_sites``: every case asserts that from the naive restatement (``check_case``).
Planted intervals either copy i's genotypes to j (kind 2) or turn j het wherever the pair would
be ``opp`` (kind 1 only); the site in front of and behind a planted interval is made an ``opp``
site, so the planted run is exactly the interval.
"""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import cuking_amd
from cuking_amd.ibd import IBD_PAIR_DTYPE, IBD_SEGMENT_DTYPE, sort_segments

STEP = 4096            # sites of one wavefront step: 64 lanes x 64 sites (king_ibd.hip)
MIN = 64               # CUKING_IBD_MIN_SITES


# ---- the naive restatement -----------------------------------------------------------------------
def naive(code, num_sites, index, group, pos, min_sites, min_length):
    """``(rows, segments)`` from codes uint8 ``[samples, >= num_sites]`` (0 hom-ref, 1 het, 2
    hom-var, 3 missing), pairs uint32 ``[P, 2]``, ``group`` / ``pos`` arrays or None."""
    num_stored = code.shape[0]
    rows = np.zeros(len(index), dtype=IBD_PAIR_DTYPE)
    segments = []
    for p, (i, j) in enumerate(index):
        rows[p]["sample_i"], rows[p]["sample_j"] = i, j
        if i >= num_stored or j >= num_stored:
            continue
        ci, cj = code[i, :num_sites].astype(int), code[j, :num_sites].astype(int)
        called = (ci != 3) & (cj != 3)
        breaks = {1: called & (np.abs(ci - cj) == 2), 2: called & (ci != cj)}
        for kind in (1, 2):
            runs, first = [], None
            for s in range(num_sites):
                if first is not None and group is not None and group[s] != group[s - 1]:
                    runs.append((first, s - 1))   # a boundary ends a run, the site stays
                    first = None
                if breaks[kind][s]:
                    if first is not None:
                        runs.append((first, s - 1))
                    first = None
                elif first is None:
                    first = s
            if first is not None:
                runs.append((first, num_sites - 1))
            count = total = longest = 0
            for a, b in runs:
                length = int(pos[b]) - int(pos[a]) if pos is not None else b - a
                if b - a + 1 >= min_sites and length >= min_length:
                    count, total, longest = count + 1, total + length, max(longest, length)
                    segments.append((p, kind, a, b))
            rows[p][f"segments{kind}"], rows[p][f"length{kind}"] = count, total
            rows[p][f"longest{kind}"] = longest
    return rows, sort_segments(np.array(segments, dtype=IBD_SEGMENT_DTYPE))


# ---- inputs --------------------------------------------------------------------------------------
def pack_codes(code, plane_words, ones_padding=False):
    """The sample-major bitset uint64 ``[samples, 2 plane_words]`` of codes ``[samples, sites]``:
    het plane then hom_var plane, site s at bit s & 63 of word s >> 6; the bits from ``sites`` on
    are all clear, or all set."""
    n, m = code.shape
    planes = np.full((n, 2, plane_words * 64), 1 if ones_padding else 0, dtype=np.uint8)
    planes[:, 0, :m] = code & 1
    planes[:, 1, :m] = code >> 1
    packed = np.packbits(planes, axis=2, bitorder="little")
    return np.ascontiguousarray(packed).view("<u8").reshape(n, 2 * plane_words)


@dataclass(frozen=True)
class Case:
    """``plants``: (i, j, first, last, kind); ``opps`` / ``missing``: (sample_i, sample_j, site)
    made an opp site / (sample, site) made missing, after the plants; ``bounds``: the sites
    that start a new group; ``pos``: None (the index) or the largest step between neighbours;
    ``tight``: plane_words = ceil(sites / 64), else the library's padded width; ``expect``:
    list position -> (segments1, segments2) the case is built to give; ``crowd``: every pair
    of the first ``crowd`` samples is listed (fewer where min_sites is small: the chance that
    an unrelated pair has a run of 64 sites is 0.9^64 per start); ``slow``: (first, last) ranges
    of sites whose positions advance by one, whatever ``pos`` says."""
    name: str
    samples: int
    sites: int
    min_sites: int = MIN
    min_length: int = 0
    plants: tuple = ()
    opps: tuple = ()
    missing: tuple = ()
    bounds: tuple = ()
    pos: object = None
    tight: bool = True
    stride: int = 8
    seed: int = 1
    expect: tuple = ()
    crowd: int = 8
    slow: tuple = ()


@dataclass
class Inputs:
    case: Case
    code: np.ndarray
    wps: int
    index: np.ndarray     # uint32 [P, 2]
    planted: np.ndarray   # bool [P]: planted, self or out of range (may have segments)
    group: object
    pos: object

    def bits(self, ones_padding=False):
        return pack_codes(self.code, self.wps // 2, ones_padding)

    @property
    def pairs(self):
        """The list in the case's stride: uint32 [P, 2], or KING_RESULT_DTYPE records."""
        if self.case.stride == 8:
            return self.index
        recs = np.zeros(len(self.index), dtype=cuking_amd.KING_RESULT_DTYPE)
        recs["sample_i"], recs["sample_j"] = self.index[:, 0], self.index[:, 1]
        recs["kin"] = 0.25
        return recs


def draw_codes(rng, samples, sites, missing=0.02):
    af = rng.uniform(0.2, 0.5, size=sites)
    code = ((rng.random((samples, sites)) < af).astype(np.uint8) +
            (rng.random((samples, sites)) < af).astype(np.uint8))
    code[rng.random((samples, sites)) < missing] = 3
    return code


def make_opp(code, i, j, s):
    code[i, s], code[j, s] = 0, 2


def plant(code, i, j, first, last, kind):
    seg = slice(first, last + 1)
    if kind == 2:
        code[j, seg] = code[i, seg]
    else:
        ci, cj = code[i, seg].astype(int), code[j, seg]
        cj[(ci != 3) & (cj != 3) & (np.abs(ci - cj) == 2)] = 1
    for s in (first - 1, last + 1):
        if 0 <= s < code.shape[1]:
            make_opp(code, i, j, s)


@lru_cache(maxsize=None)
def inputs(case: Case) -> Inputs:
    rng = np.random.default_rng(case.seed)
    code = draw_codes(rng, case.samples, case.sites)
    for i, j, first, last, kind in case.plants:
        plant(code, i, j, first, last, kind)
    for i, j, s in case.opps:
        make_opp(code, i, j, s)
    for sample, s in case.missing:
        code[sample, s] = 3
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
    # the list: planted pairs, swapped, every pair of the first `crowd` samples, self pairs, a
    # repeat, indices outside the stored samples
    n = case.samples
    listed = [(i, j) for i, j, *_ in case.plants] + [(j, i) for i, j, *_ in case.plants]
    special = len(listed)
    crowd = min(n, case.crowd)
    listed += [(i, j) for i in range(crowd) for j in range(i + 1, crowd)]
    own = {(min(i, j), max(i, j)) for i, j, *_ in case.plants}
    planted = [k < special or pair in own for k, pair in enumerate(listed)]
    extra = [(0, 0), (n - 1, n - 1), (n, 0), (1, 0xFFFFFFFF), listed[0] if listed else (0, 0)]
    listed += extra
    planted += [True] * len(extra)
    index = np.array(listed, dtype=np.uint64).astype(np.uint32).reshape(-1, 2)
    return Inputs(case, code, wps, index, np.array(planted, dtype=bool), group, pos)


@lru_cache(maxsize=None)
def reference(case: Case):
    inp = inputs(case)
    return naive(inp.code, case.sites, inp.index, inp.group, inp.pos, case.min_sites,
                 case.min_length)


def check_case(case: Case):
    """What the case states about itself, from the naive restatement alone."""
    inp = inputs(case)
    rows, _ = reference(case)
    quiet = rows[~inp.planted]
    assert not quiet["segments1"].any() and not quiet["segments2"].any(), \
        f"{case.name}: an unplanted pair has a segment at min_sites = {case.min_sites}"
    for at, want in case.expect:
        got = (int(rows[at]["segments1"]), int(rows[at]["segments2"]))
        assert got == want, (case.name, at, got, want)
    assert (rows["length2"] <= rows["length1"]).all()
    if inp.pos is not None and inp.group is None:
        assert (np.diff(inp.pos.astype(np.int64)) >= 0).all()


def run_host(case: Case, ones_padding=False, max_segments=None):
    from cuking_amd.ibd import ibd_segments_raw_host
    inp = inputs(case)
    return ibd_segments_raw_host(inp.bits(ones_padding), inp.wps, case.sites, inp.pairs,
                                 inp.group, inp.pos, case.min_sites, case.min_length,
                                 segments=True, max_segments=max_segments)


def check_against(case: Case, rows, segments, what="rows"):
    """A backend's rows and segment list against the naive restatement, bytewise."""
    want_rows, want_segments = reference(case)
    assert rows.dtype == IBD_PAIR_DTYPE
    for name in IBD_PAIR_DTYPE.names:
        assert np.array_equal(rows[name], want_rows[name]), (case.name, what, name)
    assert rows.tobytes() == want_rows.tobytes(), (case.name, what)
    assert sort_segments(segments).tobytes() == want_segments.tobytes(), (case.name, what)


S = STEP
CASES = [
    # ---- the shapes: one word, a word edge, one step, the carry between steps
    Case("1 site", 8, 1),
    Case("63 sites", 8, 63, plants=((0, 1, 0, 62, 2),)),
    Case("64 sites: one whole word, closed beyond the plane", 8, 64,
         plants=((0, 1, 0, 63, 2),), expect=((0, (1, 1)),)),
    Case("64 sites, padded planes", 8, 64, plants=((0, 1, 0, 63, 1),), tight=False,
         expect=((0, (1, 0)),)),
    Case("65 sites", 9, 65, plants=((0, 1, 1, 64, 2), (2, 3, 0, 63, 1)),
         expect=((0, (1, 1)), (1, (1, 0)))),
    Case("4096 sites: one step, the close bit in the next", 10, S, min_sites=200,
         plants=((0, 1, 0, S - 1, 2), (2, 3, 3000, S - 1, 1)),
         expect=((0, (1, 1)), (1, (1, 0)))),
    Case("4097 sites", 10, S + 1, min_sites=200,
         plants=((0, 1, 3800, S, 1), (2, 3, 100, 4000, 2)), expect=((0, (1, 0)), (1, (1, 1)))),
    Case("two steps and 37 sites: the carry", 12, 2 * S + 37, min_sites=200,
         plants=((0, 1, 4000, 2 * S + 36, 2), (2, 3, 17, 2 * S + 5, 1), (4, 5, S - 100, S + 100, 2)),
         expect=((0, (1, 1)), (1, (1, 0)), (2, (1, 1))), stride=24),
    # ---- runs at word and step edges
    Case("a run ends at bit 63, another starts at bit 0", 8, 700, min_sites=150,
         plants=((0, 1, 100, 319, 2), (2, 3, 320, 600, 2)),
         expect=((0, (1, 1)), (1, (1, 1)))),
    Case("a whole step without a break", 8, 3 * S, min_sites=200,
         plants=((0, 1, S - 1, 2 * S, 2), (2, 3, S, 2 * S - 1, 1)),
         expect=((0, (1, 1)), (1, (1, 0)))),
    Case("exactly min_sites, and one less", 8, 1000, min_sites=150,
         plants=((0, 1, 101, 250, 2), (2, 3, 101, 249, 2), (4, 5, 500, 649, 1), (6, 7, 500, 648, 1)),
         expect=((0, (1, 1)), (1, (0, 0)), (2, (1, 0)), (3, (0, 0)))),
    Case("exactly 64 sites over a word edge and in one word, and 63", 8, 400, crowd=4,
         plants=((0, 1, 30, 93, 2), (2, 3, 30, 92, 2), (4, 5, 128, 191, 2), (6, 7, 128, 190, 2)),
         expect=((0, (1, 1)), (1, (0, 0)), (2, (1, 1)), (3, (0, 0)))),
    # ---- positions
    Case("min_length: sites pass and length fails, and the other way round", 8, 1500,
         min_sites=150, min_length=500, pos=12, slow=((90, 300),),
         plants=((0, 1, 100, 290, 2), (2, 3, 400, 1200, 2), (4, 5, 301, 446, 2))),
    Case("positions with groups", 8, 2000, min_sites=150, min_length=300, pos=4,
         bounds=(640, 1301), plants=((0, 1, 500, 900, 2), (2, 3, 1301, 1999, 1)), stride=24),
    # ---- breaks at the ends
    Case("breaks at site 0 and at the last site", 8, 500, min_sites=150,
         plants=((0, 1, 1, 498, 2), (2, 3, 1, 498, 1)), expect=((0, (1, 1)), (1, (1, 0)))),
    # ---- groups
    Case("group boundaries mid-word, on a word edge and on a step edge", 8, S + 900,
         min_sites=160, bounds=(200, 448, S),
         plants=((0, 1, 10, S + 800, 2), (2, 3, 150, 447, 1)),
         expect=((0, (4, 4)), (1, (1, 0)))),
    Case("a group shorter than min_sites", 8, 900, min_sites=150, bounds=(300, 390, 391),
         plants=((0, 1, 0, 899, 2),), expect=((0, (2, 2)),)),
    Case("every word a group", 8, 640, bounds=tuple(range(64, 640, 64)), crowd=4,
         plants=((0, 1, 0, 639, 2), (2, 3, 64, 300, 1)), expect=((0, (10, 10)), (1, (3, 0)))),
    # ---- missing sites
    Case("missing inside a run and at its ends", 8, 900, min_sites=150,
         plants=((0, 1, 200, 500, 2), (2, 3, 600, 899, 1)),
         missing=((0, 200), (1, 200), (1, 350), (0, 351), (1, 351), (0, 500), (3, 600), (2, 899),
                  (3, 899), (2, 700)),
         expect=((0, (1, 1)), (1, (1, 0)))),
    Case("missing over a whole word inside a run", 8, 600, min_sites=150,
         plants=((0, 1, 100, 400, 2),),
         missing=tuple((0, s) for s in range(192, 256)), expect=((0, (1, 1)),)),
    # ---- more samples, padded width, records
    Case("sixteen samples, padded width, records", 16, 3000, min_sites=180, tight=False,
         stride=24, plants=((0, 9, 0, 2999, 2), (2, 11, 500, 2500, 1), (4, 15, 1000, 1179, 2))),
]

FUZZ_SEEDS = range(40)


def fuzz_case(seed: int) -> Case:
    """A small random case over the same parameters."""
    rng = np.random.default_rng(1000 + seed)
    samples = int(rng.integers(8, 17))
    sites = int(rng.choice([int(rng.integers(65, 700)), int(rng.integers(700, 2 * S + 200))]))
    # (an unrelated run of 120 sites has a chance of 0.9^120: enough for a few hundred sites)
    min_sites = int(rng.integers(120, 200)) if sites < 700 else int(rng.integers(200, 300))
    bounds = tuple(sorted({int(b) for b in rng.integers(1, sites, size=int(rng.integers(0, 4)))}))
    plants = []
    for k in range(int(rng.integers(1, 5))):
        length = int(rng.integers(min_sites - 20, max(min_sites + 1, sites // 2)))
        first = int(rng.integers(0, max(1, sites - length)))
        plants.append((2 * k, 2 * k + 1, first, min(sites - 1, first + length - 1),
                       int(rng.integers(1, 3))))
    missing = tuple((int(rng.integers(0, 8)), int(rng.integers(0, sites))) for _ in range(20))
    pos = None if rng.random() < 0.4 else int(rng.integers(1, 9))
    min_length = 0 if pos is None or rng.random() < 0.5 else int(rng.integers(100, 600))
    return Case(f"fuzz {seed}", samples, sites, min_sites, min_length, tuple(plants), (), missing,
                bounds, pos, bool(rng.random() < 0.5), int(rng.choice([8, 24])), 2000 + seed)


# ---- the refusals through the raw ABI ------------------------------------------------------------
# name -> the arguments replaced (see raw_arguments)
REFUSALS = {
    "words_per_sample zero": dict(wps=0),
    "words_per_sample odd": dict(wps=3),
    "sites beyond the planes": dict(num_sites=64 * 3 + 1),
    "min_sites below 64": dict(min_sites=63),
    "stride below 8": dict(stride=4),
    "stride not a multiple of 4": dict(stride=10),
    "null bits": dict(bits=None),
    "null pairs": dict(pairs=None),
    "null out": dict(out=None),
    "null segments with room asked": dict(segments=None),
    "segments without a counter": dict(found=None),
}
REFUSAL_CASE = Case("refusals", 8, 180, plants=((0, 1, 20, 150, 2),))


def raw_arguments(inp, pointers, **over):
    """The argument list of cuking_ibd_pairs_host (the device call adds ctx and stream around
    it): ``pointers`` holds bits, group, pos, pairs, out, segments, found."""
    a = dict(pointers, num_stored=inp.case.samples, wps=inp.wps, num_sites=inp.case.sites,
             min_sites=inp.case.min_sites, min_length=inp.case.min_length,
             num_pairs=len(inp.index), stride=inp.case.stride, max_segments=16)
    a.update(over)
    return (a["bits"], a["num_stored"], a["wps"], a["num_sites"], a["group"], a["pos"],
            a["min_sites"], a["min_length"], a["pairs"], a["num_pairs"], a["stride"], a["out"],
            a["segments"], a["max_segments"], a["found"])
