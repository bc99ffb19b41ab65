"""Site order (king_sort.hip, "filter_site_order") replayed in numpy for the three cohort
models of the synthetic generator at 512 samples x 4,096 sites: the weight per site, the
stable order, the cumulative table at the phase boundaries, the share rule -- and the fact
everything rests on: one permutation of the sites applied to every sample leaves the
reference's six sums of every pair as they are."""
import numpy as np
import pytest

from cuking_amd.synth import plan_cohort
import synth_models_twin as twin

N, M, SEED = 512, 4096, 5
NUM_PHASES = 128                 # king_common.h kNumPhases
MODELS = ("baseline", "exome", "admixed")


@pytest.fixture(scope="module", params=MODELS)
def cohort(request):
    c = plan_cohort(N, SEED)
    g = twin.genotypes(request.param, SEED, c.kind, c.pa, c.pb, 0, N, M)
    return request.param, g


def site_counts(g):
    return [(g == k).sum(axis=0).astype(np.int64) for k in (0, 1, 2, 3)]


def weights(g):
    r, h, a, _ = site_counts(g)
    return r * h + h * a + 4 * r * a


def cum_table(w_sorted, all_steps):
    """Weight in front of phase boundary x + 1, x = 0 .. 127 (king_common.h SiteCurve)."""
    run = np.concatenate([[0], np.cumsum(w_sorted)])
    ends = [min(256 * (all_steps * (x + 1) // NUM_PHASES), len(w_sorted)) for x in range(NUM_PHASES)]
    return run[ends]


def sigma_of(g):
    r, h, a, mis = (c.astype(np.float64) for c in site_counts(g))
    n = r + h + a + mis
    pairs = 0.5 * n * (n - 1)
    p1, p4 = (r * h + h * a) / pairs, r * a / pairs
    var = p1 + 16 * p4 - (p1 + 4 * p4) ** 2
    return np.sqrt(var.sum()) / (4 * (h / n).sum())


def need_of(g, thr):
    """(1 - 2 thr) / (1 - 2 kappa): king_filter.hip bound_level with the counts' sigma."""
    sites = 256 * ((M + 255) // 256)
    m = ((g == 3).sum() + N * (sites - M)) / (N * sites)
    h = (g == 1).sum() / (N * sites)
    kappa = m * (1 + m / (2 * h * (1 - m))) + 4.6 * sigma_of(g) + 0.003
    return (1 - 2 * thr) / (1 - 2 * kappa) if kappa < 0.5 else np.inf


def share_of(cum, need):
    for s in range(32, 63):
        if cum[2 * s - 1] >= need * cum[-1]:
            return s
    return 0


def test_weight_is_the_sum_of_squared_differences_over_the_pairs(cohort):
    _, g = cohort
    w = weights(g)
    t = np.where(g == 3, 0, g.astype(np.int64))
    d = (g != 3)
    for s in np.random.default_rng(1).choice(M, 48, replace=False):
        diff = (t[:, s][:, None] - t[:, s][None, :]) ** 2 * (d[:, s][:, None] & d[:, s][None, :])
        assert np.triu(diff, 1).sum() == w[s], s


def test_order_is_stable_and_descending(cohort):
    _, g = cohort
    w = weights(g)
    order = np.argsort(-w, kind="stable")
    assert np.array_equal(np.sort(order), np.arange(M))
    ws = w[order]
    assert np.all(ws[:-1] >= ws[1:])
    ties = ws[:-1] == ws[1:]
    assert np.all(order[:-1][ties] < order[1:][ties])      # ties keep stored order


@pytest.mark.parametrize("thr", [0.05, 0.0884])
def test_share_from_the_curve_never_exceeds_the_linear_rule(cohort, thr):
    """The cumulative table is concave in the sorted order, so the share it gives is at most
    the linear rule's; and it is the FIRST 64th that holds `need` of the weight."""
    model, g = cohort
    w = weights(g)
    all_steps = (M + 255) // 256
    cum = cum_table(np.sort(w)[::-1], all_steps)
    assert cum[-1] == w.sum() and np.all(np.diff(cum) >= 0)
    # concave: every phase holds at most the weight of the one before it
    per_phase = np.diff(np.concatenate([[0], cum]))
    steps = np.diff([all_steps * x // NUM_PHASES for x in range(NUM_PHASES + 1)])
    full = steps == steps.max()
    assert np.all(np.diff(per_phase[full]) <= 0)
    need = need_of(g, thr)
    s = share_of(cum, need)
    linear = int(np.ceil(64 * need)) if need <= 62 / 64 else 0
    if linear:
        assert 32 <= s <= max(linear, 32), (model, s, linear)
    if s > 32:
        assert cum[2 * (s - 1) - 1] < need * cum[-1]


def test_permuted_bitset_gives_the_reference_sums(cohort, oracle):
    _, g = cohort
    n = 96                                        # every pair of a sub-block
    order = np.argsort(-weights(g), kind="stable")
    bits = twin.bitset_from_genotypes(g[:n])
    perm = twin.bitset_from_genotypes(g[:n][:, order])
    sm = oracle.submatrix(n)
    a, b = oracle.all_pairs(sm, bits), oracle.all_pairs(sm, perm)
    for x, y in zip(a, b):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
