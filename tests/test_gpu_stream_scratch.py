"""The per-stream scratch cache of a context (csrc/king_abi.hip) as its newest users see it:
cuking_unrelated_set's workspace, cuking_compact_sites' table and cuking_ld_edges' counter.

cuking_ctx_reserve promises "no allocation, no host wait afterwards", so the two counters
behind it -- "workspace_allocations" and "host_syncs" -- are part of the contract.  Every
delta asserted here is read off the library's code: an entry of the cache is created without
an allocation; a stream-owned buffer is allocated once (+1), kept while it is large enough
(+0) and replaced when a call needs more (+1, behind ONE wait for its stream: an earlier call
may still use the old one); at most 8 streams have an entry, the oldest makes room (one wait
for its stream).  The results are checked against the host functions at every step."""
import numpy as np
import pytest

from conftest import random_genotypes
from ld_cases import ld_cohort, same_records
from site_qc_cases import pack
from unrelated_cases import family_graph, records

import cuking_amd
from cuking_amd import api

pytestmark = pytest.mark.gpu

MAX_STREAMS = 8                      # kMaxStreams of csrc/king_abi.hip


@pytest.fixture
def fresh():
    """A context of its own: the counters start at zero, the cache is empty."""
    c = cuking_amd.KingContext(0)
    yield c
    c.close()


class Counters:
    """deltas() = (workspace_allocations, host_syncs) since the last call."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.last = self.read()

    def read(self):
        return (self.ctx.get_option("workspace_allocations"), self.ctx.get_option("host_syncs"))

    def deltas(self):
        now = self.read()
        out = (now[0] - self.last[0], now[1] - self.last[1])
        self.last = now
        return out


def device_records(recs):
    import torch
    words = np.ascontiguousarray(recs).view(np.int32).reshape(-1, 6)
    return torch.from_numpy(words.copy()).to("cuda:0")


def unrelated_like_host(ctx, recs, n):
    got = ctx.unrelated_set(device_records(recs), len(recs), n)
    keep, family = api.unrelated_set_host(recs, n)
    assert got.keep.cpu().numpy().tobytes() == keep.tobytes()
    assert got.family.cpu().numpy().view(np.uint32).tobytes() == family.tobytes()


def compact_like_host(ctx, bits, m):
    """Every other site kept: compact_sites equals compact_sites_host."""
    import torch
    wps = bits.shape[1]
    keep = cuking_amd.site_mask_words(np.arange(m) % 2 == 0)
    want, want_wps, want_kept = cuking_amd.compact_sites_host(bits, wps, keep, m)
    got, got_wps, got_kept = ctx.compact_sites(ctx.upload_bitset(bits), wps, keep, m)
    torch.cuda.synchronize()
    assert (got_wps, got_kept) == (want_wps, want_kept)
    assert np.array_equal(got.cpu().numpy().view(np.uint64), want)


class LdCase:
    """4 sites x 8 samples: the site-major bitset on the device and the host's edges."""

    def __init__(self, ctx, n=8, m=4, seed=3):
        bits = pack(ld_cohort(seed, n, m))
        site_bits = cuking_amd.transpose_sites_host(bits, bits.shape[1], m)
        self.n, self.m = n, m
        self.want, self.count = cuking_amd.ld_edges_host(site_bits, m, n, 50, 0.0)
        self.site_bits = ctx.upload_bitset(site_bits.reshape(m, -1)).view(m, 2, -1)

    def check(self, ctx):
        records_, count = ctx.ld_edges(self.site_bits, self.m, self.n, 50, 0.0)
        host = records_[:count].cpu().numpy().view(np.uint32).reshape(-1)
        got = cuking_amd.sort_results(host.view(cuking_amd.KING_RESULT_DTYPE).copy())
        assert count == self.count and same_records(got, self.want)


def test_unrelated_set_workspace_grows_behind_one_wait(fresh):
    small = records([0, 2, 5], [1, 3, 7], [0.3, 0.2, 0.1])
    c = Counters(fresh)
    unrelated_like_host(fresh, small, 8)
    assert c.deltas()[0] == 1                    # the workspace; the entry itself costs nothing
    unrelated_like_host(fresh, small, 8)
    allocations, repeat_syncs = c.deltas()
    assert allocations == 0
    unrelated_like_host(fresh, small, 8)
    assert c.deltas() == (0, repeat_syncs)       # no wait is due to the buffer
    # a larger workspace on the same stream: one allocation, one wait more than a repeat
    n = 4096
    large = records(*family_graph(5, n=n, num_edges=300))
    unrelated_like_host(fresh, large, n)
    allocations, grow_syncs = c.deltas()
    assert allocations == 1
    unrelated_like_host(fresh, large, n)
    allocations, large_syncs = c.deltas()
    assert allocations == 0 and grow_syncs == large_syncs + 1
    # and a small call afterwards fits into the large buffer
    unrelated_like_host(fresh, small, 8)
    assert c.deltas() == (0, repeat_syncs)


def test_compact_sites_table_grows_behind_one_wait(fresh):
    rng = np.random.default_rng(17)
    narrow = pack(random_genotypes(rng, 5, 50))      # words_per_sample 2
    wide = pack(random_genotypes(rng, 5, 250))       # words_per_sample 8: a larger table
    assert (narrow.shape[1], wide.shape[1]) == (2, 8)
    c = Counters(fresh)
    compact_like_host(fresh, narrow, 50)
    assert c.deltas() == (1, 1)                  # the table; the wait for its upload
    compact_like_host(fresh, narrow, 50)
    assert c.deltas() == (0, 1)
    compact_like_host(fresh, wide, 250)
    assert c.deltas() == (1, 2)                  # replaced behind a wait for the stream
    compact_like_host(fresh, wide, 250)
    assert c.deltas() == (0, 1)
    compact_like_host(fresh, narrow, 50)
    assert c.deltas() == (0, 1)


def test_ld_edges_counter_is_allocated_once(fresh):
    case = LdCase(fresh)
    assert case.count > 0
    c = Counters(fresh)
    case.check(fresh)
    assert c.deltas() == (1, 1)                  # the counter word; the wait for the count
    case.check(fresh)
    assert c.deltas() == (0, 1)


def test_the_oldest_stream_makes_room(fresh):
    import torch
    case = LdCase(fresh)
    streams = [torch.cuda.Stream("cuda:0") for _ in range(MAX_STREAMS + 1)]
    assert len({s.cuda_stream for s in streams}) == len(streams)
    torch.cuda.synchronize()
    c = Counters(fresh)

    def on(stream):
        with torch.cuda.stream(stream):
            case.check(fresh)
        return c.deltas()

    for s in streams[:MAX_STREAMS]:
        assert on(s) == (1, 1)
    assert on(streams[MAX_STREAMS]) == (1, 2)    # the first stream's entry goes: one wait for it
    assert on(streams[0]) == (1, 2)              # it was the one evicted (the second goes now)
    assert on(streams[MAX_STREAMS]) == (0, 1)    # the ninth kept its entry
    assert on(streams[2]) == (0, 1)
    torch.cuda.synchronize()


def test_one_entry_serves_every_user_of_a_stream(fresh):
    """relative_counts (split slab and filter scratch), unrelated_set, compact_sites and
    ld_edges on one stream share the stream's entry; each keeps its own buffer."""
    rng = np.random.default_rng(23)
    n, m = 300, 512
    bits = pack(random_genotypes(rng, n, m))
    d_bits = fresh.upload_bitset(bits)
    sm = cuking_amd.Submatrix(n)
    small = records([0, 2, 5], [1, 3, 7], [0.3, 0.2, 0.1])
    narrow = pack(random_genotypes(rng, 5, 50))
    case = LdCase(fresh)

    def every_user():
        counts = fresh.relative_counts(sm, bits.shape[1], d_bits).bands()
        unrelated_like_host(fresh, small, 8)
        compact_like_host(fresh, narrow, 50)
        case.check(fresh)
        return counts

    c = Counters(fresh)
    first = every_user()
    assert c.deltas()[0] >= 4                    # (the pair kernels' workspace as well)
    second = every_user()
    assert c.deltas()[0] == 0
    assert np.array_equal(first, second)
