"""The filter kernel's offset code (king_filter.hip, "Offset code"), replayed in float32.

A T2 nibble holds two sites: set B (bits 2-3) as T in fp4 sign / magnitude, +-2.0, set A
(bits 0-1) as 1 + T in plain binary, i.e. the fp4 values (1 + T) / 2.  The set-B products
go through the scaled MFMA (2^-2 on either operand), so one float32 accumulator holds
    acc = (q + n_A + S_i + S_j) / 4,
and with u~ = u + 2 S + n_A per sample the kernel tests (u~_i - 8 acc) + u~_j, which must be
the very float u_i + u_j - 2 q that the kernel tested before the low field changed its code.
CPU only: numpy stands in for the matrix pipe (every fp4 product and every sum of a 64-site
slice is exact there as well; the slices are then added one by one in float32).

This file imports nothing from the project: the nibbles, the u~ tables and the range
differences below are a restatement of what prepare_nibbles_kernel, sample_stats_kernel and
prefix_u_of() are specified to do, in the same order of float operations -- it checks the
ARITHMETIC of the scheme, not the kernels (the GPU parity tests compare those with the oracle).
"""
import numpy as np
import pytest

F = np.float32
E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=np.float32)
HOM_REF, HET, HOM_ALT, MISSING = 0, 1, 2, 3
STEP = 256  # sites per k-step: 4 units of 64, the high 32 of each are set A


def fp4(nibbles):
    mag = E2M1[nibbles & 7]
    return np.where(nibbles & 8, -mag, mag).astype(np.float32)


def random_calls(rng, samples, stored_sites, sites, missing_rate):
    g = rng.choice([HOM_REF, HET, HOM_ALT], p=[0.5, 0.3, 0.2], size=(samples, sites))
    g[rng.random((samples, sites)) < missing_rate] = MISSING
    g[:, stored_sites:] = MISSING  # padding sites are missing calls (cuking.cu:513-523)
    return g


def t2_nibbles(g):
    """(samples, sites / 2) nibbles as the T2 layout specifies them (king_common.h): site
    64 u + t in bits 2-3 (hom-alt, hom), site 64 u + 32 + t in bits 0-1 (hom-ref, het or
    missing)."""
    u = g.reshape(g.shape[0], -1, 2, 32)
    lo, hi = u[:, :, 0, :], u[:, :, 1, :]
    hom = (lo == HOM_REF) | (lo == HOM_ALT)
    nib = ((lo == HOM_ALT).astype(np.uint8) << 3) | (hom.astype(np.uint8) << 2) | \
          ((hi == HOM_REF).astype(np.uint8) << 1) | ((hi == HET) | (hi == MISSING)).astype(np.uint8)
    return nib.reshape(g.shape[0], -1)


def set_a_mask(sites):
    return (np.arange(sites) % 64) >= 32


def per_step_counts(g):
    """Per sample and k-step: u = |Y| - |M|, S = sum of T over set A; n_A per k-step is 128."""
    t = (g == HOM_REF).astype(np.int64) - (g == HOM_ALT)
    y = (g == HOM_REF) | (g == HOM_ALT)
    a = set_a_mask(g.shape[1])
    steps = g.shape[1] // STEP
    u = (y.astype(np.int64) - (g == MISSING)).reshape(len(g), steps, STEP).sum(2)
    s = (t * a).reshape(len(g), steps, STEP).sum(2)
    return t, u, s


def kernel_acc(nib_i, nib_j, slices):
    """float32 accumulator over the given slices (unit, set: 32 sites, half of what one MFMA
    adds) in order: what the MFMAs of one pair leave.  Set B: (x 2^-2) on either operand; set
    A as it is."""
    acc = F(0)
    scale = F(0.25)
    for unit, is_a in slices:
        ni, nj = nib_i[32 * unit:32 * unit + 32], nib_j[32 * unit:32 * unit + 32]
        if is_a:
            prod = fp4(ni & 0x3) * fp4(nj & 0x3)
        else:
            prod = (fp4(ni & 0xC) * scale) * (fp4(nj & 0xC) * scale)
        # (the products of a slice: multiples of 1/4 of magnitude <= 1, their sum is exact)
        acc = F(acc + F(prod.astype(np.float64).sum()))
    return acc


def slices_of_steps(step_list):
    # k-step s = units 4 s .. 4 s + 3; the kernel alternates set B and set A of each unit
    return [(4 * s + c, is_a) for s in step_list for c in range(4) for is_a in (False, True)]


def range_value_f32(cum, total, lo, hi, n):
    """u~ over boundaries [lo, hi) of a cumulative float32 table with n intervals (cum[x] = in
    front of boundary x, cum[0] = 0; total = cum[n]), hi > n: the range goes around the end.
    The order of the float operations is prefix_u_of()'s: (total - front of lo) + wrapped end."""
    if hi <= n:
        return F(cum[hi] - cum[lo])
    return F(F(total - cum[lo]) + cum[hi - n])


def cumulative_f32(per_step):
    """Cumulative per-sample values in front of every k-step boundary, as float32 tables."""
    c = np.concatenate([np.zeros((per_step.shape[0], 1), np.int64), np.cumsum(per_step, 1)], 1)
    assert np.all(np.abs(c) < 2 ** 24)
    return c.astype(np.float32)


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("missing_rate", [0.0, 0.05, 0.4])
def test_offset_code_equals_plain_bound(seed, missing_rate):
    rng = np.random.default_rng(seed)
    steps = 12
    sites = steps * STEP
    stored = sites - int(rng.integers(0, 300))  # padding sites in the last k-steps
    g = random_calls(rng, 6, stored, sites, missing_rate)
    g[4] = MISSING  # a padding sample: T = 0 everywhere
    g[5, :stored] = HOM_REF
    nib = t2_nibbles(g)
    # the layout says what the issue says: & 0xC -> +-2 T ... & 0x3 -> (1 + T) / 2
    t, u_step, s_step = per_step_counts(g)
    a = set_a_mask(sites)
    dec_b = fp4(nib & 0xC).reshape(len(g), -1, 32)
    dec_a = fp4(nib & 0x3).reshape(len(g), -1, 32)
    tt = t.reshape(len(g), -1, 2, 32)
    assert np.array_equal(dec_b, 2.0 * tt[:, :, 0, :])
    assert np.array_equal(dec_a, (1.0 + tt[:, :, 1, :]) / 2.0)
    assert np.array_equal(t[4], np.zeros(sites, np.int64)) and np.all((nib[4] & 0x3) == 1)

    ut_step = u_step + 2 * s_step + STEP // 2  # u~ per k-step: n_A = 128
    cum_u, cum_ut = cumulative_f32(u_step), cumulative_f32(ut_step)

    # ranges of k-steps: all, prefixes, inner ranges, wrapped ranges (start, run to the end,
    # go on from the first k-step), single pieces of a split
    ranges = [list(range(steps)), list(range(0, 7)), list(range(3, 9)), list(range(11, 12)),
              list(range(5, steps)) + list(range(0, 5)),      # a rotated tile, all sites
              list(range(9, steps)) + list(range(0, 2)),      # ... at a check point
              list(range(steps - 1, steps)) + list(range(0, 1))]
    for _ in range(4):
        lo = int(rng.integers(0, steps))
        n = int(rng.integers(1, steps + 1))
        ranges.append([(lo + k) % steps for k in range(n)])

    def range_value(cum, idx, rg):
        # differences of the cumulative table, as prefix_u_of() forms them: contiguous part(s)
        return range_value_f32(cum[idx], cum[idx, steps], rg[0], rg[0] + len(rg), steps)

    pairs = [(i, j) for i in range(len(g)) for j in range(len(g))]
    for rg in ranges:
        sel = np.zeros(sites, bool)
        for s in rg:
            sel[s * STEP:(s + 1) * STEP] = True
        for i, j in pairs:
            q = int((t[i] * t[j])[sel].sum())
            n_a = int((a & sel).sum())
            s_i, s_j = int((t[i] * a)[sel].sum()), int((t[j] * a)[sel].sum())
            acc = kernel_acc(nib[i], nib[j], slices_of_steps(rg))
            assert float(acc) * 4 == q + n_a + s_i + s_j
            ui, uj = range_value(cum_u, i, rg), range_value(cum_u, j, rg)
            uti, utj = range_value(cum_ut, i, rg), range_value(cum_ut, j, rg)
            assert int(uti) == int(ui) + 2 * s_i + n_a
            # today's test value and the one before the change, both in float32
            new = F(F(F(-8) * acc + uti) + utj)
            old = F(F(-0.5) * F(4 * q) + F(ui + uj))
            assert new == old
            assert int(new) == int(u_step[i, rg].sum() + u_step[j, rg].sum()) - 2 * q


def test_split_pieces_add_up():
    """The k-pieces of a split remainder: their accumulators are added in float32, the u~ are
    those of the whole range."""
    rng = np.random.default_rng(7)
    steps = 16
    g = random_calls(rng, 2, steps * STEP - 77, steps * STEP, 0.03)
    nib = t2_nibbles(g)
    t, u_step, s_step = per_step_counts(g)
    q = int((t[0] * t[1]).sum())
    ut = (u_step + 2 * s_step + STEP // 2).sum(1)
    for parts in (2, 3, 5, 8):
        bounds = [p * steps // parts for p in range(parts + 1)]
        acc = F(0)
        for p in range(parts):
            acc = F(acc + kernel_acc(nib[0], nib[1], slices_of_steps(range(bounds[p], bounds[p + 1]))))
        new = F(F(F(-8) * acc + F(ut[0])) + F(ut[1]))
        assert int(new) == int(u_step[0].sum() + u_step[1].sum()) - 2 * q


@pytest.mark.parametrize("other", [HOM_REF, HOM_ALT])
def test_partial_sums_exact_at_widest_bitset(other):
    """2^22 sites (kMfmaN4MaxSites), all hom-ref against all hom-ref / all hom-alt: every
    partial sum of the accumulator, u~_i - 8 acc and the value tested are exact floats."""
    sites = 1 << 22
    slices = sites // 64  # 64-site slices, alternately set B and set A
    t_i, t_j = 1, (1 if other == HOM_REF else -1)
    # in quarters: a set-B site adds T_i T_j, a set-A site (1 + T_i) (1 + T_j)
    quarters = np.empty(slices, np.int64)
    quarters[0::2] = 64 * t_i * t_j
    quarters[1::2] = 64 * (1 + t_i) * (1 + t_j)
    exact = np.cumsum(quarters)                                    # 4 acc after every slice
    acc = np.cumsum((quarters / 4.0).astype(np.float32), dtype=np.float32)  # sequential float32 adds
    assert np.array_equal(acc.astype(np.float64) * 4, exact.astype(np.float64))
    n_a = sites // 2
    q = sites * t_i * t_j
    s_i, s_j = n_a * t_i, n_a * t_j
    assert int(exact[-1]) == q + n_a + s_i + s_j
    assert np.max(np.abs(exact)) <= 10 * sites // 4 and np.max(np.abs(exact)) < 2 ** 24
    u_i = u_j = sites
    ut_i, ut_j = u_i + 2 * s_i + n_a, u_j + 2 * s_j + n_a
    assert abs(ut_i) < 2 ** 24 and abs(ut_j) < 2 ** 24
    first = F(F(-8) * acc[-1] + F(ut_i))
    assert int(first) == u_i - n_a - 2 * s_j - 2 * q and abs(int(first)) <= 7 * sites // 2
    new = F(first + F(ut_j))
    assert int(new) == u_i + u_j - 2 * q
    # the same along the way, at every k-step boundary (a check point may sit at any of them)
    k = np.arange(3, slices, 4)                                    # last slice of every k-step
    sites_k = (k + 1) * 64
    ut_k = (sites_k + 2 * (sites_k // 2) * t_i + sites_k // 2).astype(np.float32)
    utj_k = (sites_k + 2 * (sites_k // 2) * t_j + sites_k // 2).astype(np.float32)
    val = (F(-8) * acc[k] + ut_k).astype(np.float32) + utj_k
    assert np.array_equal(val.astype(np.int64), 2 * sites_k - 2 * sites_k * t_i * t_j)


def test_wrapped_ranges_exact_at_widest_bitset():
    """2^22 sites, 128 phases, ranges that start late and go around the end of the sites (a
    rotated tile at its check point: phases 64 .. 127, shares 56 / 60 / 62 of 64), samples that
    are nearly all hom-ref with a few odd counts: u~ runs at up to 2.5 per site, so the range
    value is exact only if no partial of the difference is larger than u~ over a set of sites --
    (total - front) + wrapped end; total + wrapped end first passes 2^24 and rounds."""
    rng = np.random.default_rng(11)
    phases, steps = 128, (1 << 22) // STEP
    per_phase = steps // phases
    samples = 6
    # per k-step counts (256 sites, 128 of them set A): a few het / missing / hom-alt calls
    het_a, het_b = rng.integers(0, 3, (2, samples, steps))
    mis_a, mis_b = rng.integers(0, 2, (2, samples, steps))
    alt_a, alt_b = rng.integers(0, 2, (2, samples, steps))
    het_a[0] = het_b[0] = mis_a[0] = mis_b[0] = alt_a[0] = alt_b[0] = 0  # all hom-ref
    mis_b[0, ::97] = 1                                                   # ... but for odd counts
    u = (STEP - het_a - het_b - mis_a - mis_b) - (mis_a + mis_b)         # |Y| - |M|
    s_a = (STEP // 2 - het_a - mis_a - alt_a) - alt_a                    # sum of T over set A
    ut = u + 2 * s_a + STEP // 2
    exact = np.concatenate([np.zeros((samples, 1), np.int64),
                            np.cumsum(ut.reshape(samples, phases, per_phase).sum(2), 1)], 1)
    assert np.all(np.abs(exact) < 2 ** 24) and exact[0, -1] > 2.49 * (1 << 22)
    cum = exact.astype(np.float32)  # cum[x]: in front of phase boundary x; cum[phases] = total
    wrapped = rounds_the_other_way = 0
    for share in (56, 60, 62):
        for phase in range(64, phases):
            hi = phase + 2 * share  # (two phases per 64th)
            assert hi > phases
            for i in range(samples):
                want = int(exact[i, phases] - exact[i, phase] + exact[i, hi - phases])
                got = range_value_f32(cum[i], cum[i, phases], phase, hi, phases)
                assert int(got) == want and abs(want) <= 10 * (1 << 22) // 4
                wrapped += 1
                # (why the order matters: total + wrapped end first is rounded to an even number)
                other = F(F(cum[i, phases] + cum[i, hi - phases]) - cum[i, phase])
                rounds_the_other_way += int(other) != want
    assert wrapped == 3 * 64 * samples and rounds_the_other_way > 0
    # ... and the value the kernel tests for the all-hom-ref sample against itself and the
    # others over such a range: (u~_i - 8 acc) + u~_j with acc = (q + n_A + S_i + S_j) / 4, q
    # bounded by the sites of the range (the largest partial sums: q = the sites, T_i = T_j = 1)
    phase, hi = 100, 100 + 2 * 62
    sites = 2 * 62 * per_phase * STEP
    ut_i = range_value_f32(cum[0], cum[0, phases], phase, hi, phases)
    sel = np.r_[phase * per_phase:steps, 0:(hi - phases) * per_phase]
    s_i, u_i = int(s_a[0, sel].sum()), int(u[0, sel].sum())
    for j in range(samples):
        ut_j = range_value_f32(cum[j], cum[j, phases], phase, hi, phases)
        s_j, u_j = int(s_a[j, sel].sum()), int(u[j, sel].sum())
        q = int(min(u_i, u_j))  # (as large as the counts allow: every shared hom site agrees)
        quarters = q + sites // 2 + s_i + s_j
        assert quarters < 2 ** 24
        acc = F(quarters / 4.0)
        first = F(F(-8) * acc + ut_i)
        assert int(first) == u_i - sites // 2 - 2 * s_j - 2 * q
        assert int(F(first + ut_j)) == u_i + u_j - 2 * q
