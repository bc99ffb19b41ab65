"""The cases of the PC-Relate sweep (fuzz_cases.run_pcrelate, tools/fuzz_pcrelate.py): the three
device calls -- pcrelate_matrix, pcrelate_records, pcrelate_pairs -- over one bitset and one
model, at drawn shapes, d, blocks, pitches, bounds, launch caps, streams, call orders and pair
lists.  No GPU and no test of its own: tests/test_pcrelate_fuzz_cases.py holds the committed
seeds to the conditions the sweep rests on from the generator, the float64 references and the
host twins alone.

The cohort of a case is built by pcrelate_pairs_cases.cohort (which builds on
pcrelate_cases.inputs): genotypes that follow the model, so that unrelated pairs lie below the
k0 switch, the planted relatives, an all-missing sample, sites around the bounds (one in 7 + d
around each), NaN in every pitch.

Size classes, each the smallest shapes at which the kernels can go wrong:
  "small"  n 1 .. 300, sites 1 .. 800, d 1 .. 32; half the cases the whole cohort, half a block
           from BLOCK_MENU with drawn begins.
  "tiles"  n, sites and d from the edges of the 128 x 128 tile, the site steps of 32 and 64 and
           the D buckets (TILE_N, TILE_SITES, TILE_D); at 385 samples the record call's triangle
           has 4 tiles a side (10 tiles) and the matrix 16.
  "exact"  the integer construction of the exact cases (x = 1, beta in {0, 1, 2}, the planted
           pair without a jointly valid site, the all-missing sample) at drawn n, sites and
           block: checked on bytes, so no margin condition.

The margin condition.  A called element whose float64 mu lies within e of a bound may be valid
in float32 and not in float64, and a listed pair whose kin lies within its tolerance of the k0
switch may take the other k0 formula.  A delivered case has none (Reference.margin_violations()
== 0 for the block's matrix reference and the list's reference): the offending sites' allele
frequency is redrawn well inside the bounds, and the offending list entries are redrawn, from a
sub-seed of the case, in at most MAX_ROUNDS rounds; a case that still has one is not delivered
but raised.  tag["rounds"] says how many rounds the case took.
"""
from dataclasses import dataclass

import numpy as np

import pcrelate_cases as pc
import pcrelate_pairs_cases as pp
import pcrelate_records_cases as rc

SIZE_CLASSES = ("small", "tiles", "exact")
KINDS = ("matrix", "records", "pairs")
BLOCK_MENU = ("diagonal sub-block", "rectangle", "one row", "one column", "one entry",
              "wide rectangle")
TILE_N = (127, 128, 129, 255, 256, 257, 384, 385)
TILE_SITES = (31, 32, 33, 63, 64, 65, 95, 96, 97, 128, 129)
TILE_D = (3, 4, 5, 8, 9, 16, 17, 32)
PADS = (0, 1, 5)
LOS = (0.0, 0.01, 0.05)
LAUNCH_CAPS = (0, 0, 1, 2, 5)
PAIR_LENGTHS = (1, 63, 511, 512, 513, 1025)
MAX_ROUNDS = 4
TILE = 128              # kPcrTile
PAIR_WORKGROUP = 512    # kPairThreads


def bucket(d: int) -> int:
    """The D of pcrelate_dispatch_columns."""
    return 4 if d <= 4 else 8 if d <= 8 else 16 if d <= 16 else 32


def _inside(u, lo, hi):
    """An integer in [lo, hi) from u in [0, 1); lo where the range is empty."""
    return lo + int(u * max(hi - lo, 0)) if hi > lo else lo


def _range(u0, u1, lo, hi):
    """A non-empty [begin, end) inside [lo, hi), hi > lo."""
    begin = _inside(u0, lo, hi)
    return begin, _inside(u1, begin + 1, hi + 1)


def draw_block(n: int, kind, u) -> tuple:
    """The block of a case: `kind` None = the whole cohort, otherwise an entry of BLOCK_MENU
    with begins from the uniforms `u`.  Valid by the rule of the calls: ranges identical, or
    disjoint with the rows first.  A cohort too small for the kind gives the whole cohort."""
    whole = (0, n, 0, n)
    if kind is None or n < 2:
        return whole
    if kind == "diagonal sub-block":
        i0, i1 = _range(u[0], u[1], 0, n)
        return (i0, i1, i0, i1)
    if kind == "one entry" and u[3] < 0.5:
        i = _inside(u[0], 0, n)
        return (i, i + 1, i, i + 1)
    split = _inside(u[0], 1, n)                # rows in [0, split), columns in [split, n)
    i0, i1 = _range(u[1], u[2], 0, split)
    j0, j1 = _range(u[3], u[4], split, n)
    if kind == "rectangle":
        return (i0, i1, j0, j1)
    if kind == "one row":
        return (i0, i0 + 1, j0, j1)
    if kind == "one column":
        return (i0, i1, j0, j0 + 1)
    if kind == "one entry":
        return (i0, i0 + 1, j0, j0 + 1)
    # columns that span two tiles more than the rows, where the cohort has them
    rows = 1 + int(u[1] * 40)
    i0 = int(u[2] * 6)
    j0 = i0 + rows + int(u[3] * 3)
    if j0 >= n:
        return whole
    return (i0, i0 + rows, j0, n)


def draw_sub_block(block, u) -> tuple:
    """The block of the second matrix call: inside `block`, of the same kind."""
    i0, i1, j0, j1 = block
    a0, a1 = _range(u[0], u[1], i0, i1)
    if rc.is_diagonal(block):
        return (a0, a1, a0, a1)
    b0, b1 = _range(u[2], u[3], j0, j1)
    return (a0, a1, b0, b1)


@dataclass
class SweepInputs:
    code: np.ndarray      # uint8 [n, S]
    bits: np.ndarray      # uint64 [n, wps]
    x: np.ndarray         # float32 [n, d], a view with the pitch of the tag
    beta: np.ndarray      # float32 [S, d], likewise
    f: object             # float32 [n] or None
    lo: float
    hi: float
    wps: int
    block: tuple
    sub_block: tuple
    index: np.ndarray     # uint32 [P, 2]
    pairs: np.ndarray     # what the call takes (pcrelate_pairs_cases.pair_list)
    part: np.ndarray      # positions of the list, reordered: the second pairs call
    ref: object           # pcrelate_cases.Reference of `block` (None in the class "exact")
    pair_ref: object      # pcrelate_pairs_cases.Reference of the list (likewise)


def _pair_index(rng, n, block, length, mix_specials):
    """uint32 [length, 2]: six in ten inside the block (repeats, self pairs and reversed pairs
    among them), the others anywhere in the cohort; the special entries at drawn positions."""
    i0, i1, j0, j1 = block
    index = rng.integers(0, n, size=(length, 2))
    inside = rng.random(length) < 0.6
    index[inside, 0] = rng.integers(i0, i1, size=int(inside.sum()))
    index[inside, 1] = rng.integers(j0, j1, size=int(inside.sum()))
    index = index.astype(np.uint32)
    special = pp.specials(n)
    if mix_specials and length >= 2 * len(special):
        at = rng.choice(length, size=len(special), replace=False)
        for k, pair in zip(at, special):
            index[k] = index[(k + 1) % length] if pair is None else pair
    return np.ascontiguousarray(index)


def _build(tag) -> SweepInputs:
    n, sites, d, exact = tag["n"], tag["sites"], tag["d"], tag["size_class"] == "exact"
    case = pp.Case(f"sweep {tag['seed']}/{tag['case']}", tag["pairs"], sites, d,
                   stride=tag["stride"], f=tag["f"], seed=tag["cohort_seed"], exact=exact,
                   edge_every=7 + d, n=n, lo=tag["lo"], extra_word=tag["extra_word"],
                   pads=tuple(tag["pads"]))
    code, bits, x, beta, lo, hi, _ = pp.cohort(case)
    block = tuple(tag["block"])
    rng = np.random.default_rng(tag["list_seed"])
    index = _pair_index(rng, n, block, tag["pairs"], tag["specials"])
    f = rng.uniform(-0.1, 0.3, size=n).astype(np.float32) if tag["f"] else None
    ref = pair_ref = None
    rounds = 0
    if not exact:
        beta = pc._padded(np.array(beta), tag["pads"][1])     # (a copy: the sites are redrawn)
        sub = np.random.default_rng(tag["list_seed"] + 1)
        while True:
            ref = pc.Reference(code, x, beta, lo, hi, block)
            pair_ref = pp.Reference.of(code, x, beta, f, lo, hi, index)
            if ref.margin_violations() == 0 and pair_ref.margin_violations() == 0:
                break
            if rounds == MAX_ROUNDS:
                raise AssertionError(f"{tag}: margin violations after {MAX_ROUNDS} rounds")
            rounds += 1
            near = (np.abs(ref.mu - lo) <= ref.e) | (np.abs(ref.mu - hi) <= ref.e)
            for s in np.flatnonzero((ref.called & near).any(axis=0)):
                beta[s, 0] = np.float32(2.0 * sub.uniform(0.25, 0.75))
            kin, tol = pair_ref.value["kin"], pair_ref.tol["kin"]
            with np.errstate(invalid="ignore"):
                at_switch = np.flatnonzero(np.abs(kin - float(pp.SWITCH)) <= tol)
            index[at_switch] = sub.integers(0, n, size=(at_switch.size, 2))
    tag["rounds"] = rounds
    pairs = pp.pair_list(index, tag["stride"], rng)
    length = tag["pairs"]
    part = np.random.default_rng(tag["list_seed"] + 2).permutation(length)[:max(1, length // 3)]
    for a in (index, pairs, beta, part):
        a.setflags(write=False)
    return SweepInputs(code, bits, x, beta, f, lo, hi, bits.shape[1], block,
                       tuple(tag["sub_block"]), index, pairs, part, ref, pair_ref)


def pcrelate_sweep_cases(seed: int, cases: int, first_case: int = 0, size_class=None):
    """Yields (tag, inputs): the reproducer (every parameter of the case) and its SweepInputs.
    Every random number of a case is drawn before the `first_case` skip: a seed names the same
    cases whatever is skipped (what is built after the skip draws from sub-seeds in the tag)."""
    size_class = size_class or "small"
    assert size_class in SIZE_CLASSES, size_class
    rng = np.random.default_rng(seed)
    for case in range(cases):
        n, sites, d = int(rng.integers(1, 301)), int(rng.integers(1, 801)), int(rng.integers(1, 33))
        tile = int(rng.choice(TILE_N)), int(rng.choice(TILE_SITES)), int(rng.choice(TILE_D))
        whole = bool(rng.random() < 0.5)
        kind = BLOCK_MENU[int(rng.integers(0, len(BLOCK_MENU)))]
        u, v = rng.random(5).tolist(), rng.random(4).tolist()
        pads = [int(p) for p in rng.choice(PADS, size=3)]
        lo = float(rng.choice(LOS))
        extra_word = bool(rng.random() < 0.3)
        cap = int(rng.choice(LAUNCH_CAPS))
        side_stream = bool(rng.random() < 0.3)
        order = [KINDS[int(k)] for k in rng.permutation(3)]
        order.insert(int(rng.integers(0, 4)), "matrix_sub")
        length = int(rng.choice(PAIR_LENGTHS))
        stride = int(rng.choice([8, 24]))
        f = bool(rng.random() < 0.5)
        specials = bool(rng.random() < 0.7)
        short_buffer = bool(rng.random() < 0.2)
        cohort_seed, list_seed = int(rng.integers(1, 1 << 20)), int(rng.integers(1, 1 << 30))
        if case < first_case:
            continue
        if size_class == "tiles":
            n, sites, d = tile
        elif size_class == "exact":
            d, f = 1, False
        block = draw_block(n, None if whole else kind, u)
        # the list: capped by the block's pairs (repeats are allowed, so the cap is a choice)
        length = max(1, min(length, rc.num_pairs(block)))
        tag = dict(fuzzer="run_pcrelate", seed=seed, case=case, size_class=size_class, n=n,
                   sites=sites, d=d, block=list(block), kind="whole" if whole else kind,
                   sub_block=list(draw_sub_block(block, v)), pads=pads, lo=lo,
                   extra_word=extra_word, max_launch_blocks=cap, side_stream=side_stream,
                   calls=order, pairs=length, stride=stride, f=f, specials=specials,
                   short_buffer=short_buffer, cohort_seed=cohort_seed, list_seed=list_seed)
        yield tag, _build(tag)


def split_launches(tag) -> dict:
    """Per kind, whether the case's launch cap really splits the call: more workgroups than
    the cap."""
    cap = tag["max_launch_blocks"]
    if cap == 0:
        return dict(matrix=False, matrix_sub=False, records=False, pairs=False)

    def tiles(block, triangle):
        rows, cols = -(-(block[1] - block[0]) // TILE), -(-(block[3] - block[2]) // TILE)
        return rows * (rows + 1) // 2 if triangle and rc.is_diagonal(block) else rows * cols
    return dict(matrix=tiles(tag["block"], False) > cap,
                matrix_sub=tiles(tag["sub_block"], False) > cap,
                records=tiles(tag["block"], True) > cap,
                pairs=-(-tag["pairs"] // PAIR_WORKGROUP) > cap)
