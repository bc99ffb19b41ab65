"""The Hardy-Weinberg exact test on the GPU: hwe_sites against the host twin bit for bit (every
case of hwe_cases.py, both forms; launch sizes around the wavefront; a second stream; a reused
output), and filter_sites with the rule end to end on a small cohort with planted sites."""
import numpy as np
import pytest
import torch

import cuking_amd

import hwe_cases as hc
from site_qc_cases import pack, site_counts_numpy

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case_counts():
    """(host uint32 [rows, 4], the same on the device as int32) of every case."""
    host = hc.counts_array(hc.all_tables())
    return host, torch.from_numpy(host.view(np.int32)).to("cuda:0")


def host_bits(counts, num_sites, midp):
    return hc.bits(cuking_amd.hwe_sites_host(counts, num_sites, midp=midp))


def device_bits(p):
    return hc.bits(p.cpu().numpy())


@pytest.mark.parametrize("midp", [False, True])
def test_every_case_equals_host_twin_bitwise(ctx, case_counts, midp):
    host, dev = case_counts
    rows = host.shape[0]
    got = ctx.hwe_sites(dev, rows, midp=midp)
    assert got.dtype == torch.float64 and tuple(got.shape) == (rows,)
    got, want = device_bits(got), host_bits(host, rows, midp)
    differ = np.flatnonzero(got != want)
    assert differ.size == 0, [(host[k, :3].tolist(), hex(got[k]), hex(want[k]))
                              for k in differ[:5]]
    # ... which is the Python restatement (test_hwe_host.py has shown that for the host twin)
    assert (got == hc.bits(hc.expected(midp))).all()


@pytest.mark.parametrize("num_sites", [1, 63, 64, 65, 1000])
def test_sizes_around_the_wavefront(ctx, case_counts, num_sites):
    host, dev = case_counts
    # rows from the small tables on into the paper's and the edge rows, and from the fuzz
    for first in (len(hc.small_tables()) - 40, len(host) - 1000):
        rows, d_rows = host[first:first + num_sites], dev[first:first + num_sites]
        big = torch.full((num_sites + 64,), -7.0, dtype=torch.float64, device="cuda:0")
        out = ctx.hwe_sites(d_rows, num_sites, midp=True, out=big[:num_sites])
        assert out.data_ptr() == big.data_ptr()
        assert (device_bits(out) == host_bits(rows, num_sites, True)).all()
        assert (big[num_sites:] == -7.0).all()          # nothing past p[num_sites - 1]
    # fewer sites than the tensor has rows: only those are read and written
    out = ctx.hwe_sites(dev, num_sites)
    assert tuple(out.shape) == (num_sites,)
    assert (device_bits(out) == host_bits(host, num_sites, False)).all()


def test_second_stream_and_reused_output(ctx, case_counts):
    host, dev = case_counts
    first = len(host) - 300                               # the near-equilibrium rows
    rows, d_rows = host[first:], dev[first:]
    out = torch.zeros(300, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    got = ctx.hwe_sites(d_rows, 300, out=out, stream=side)
    side.synchronize()
    assert got is out and (device_bits(out) == host_bits(rows, 300, False)).all()
    # the same tensor again, the other form, then other rows: overwritten each time
    ctx.hwe_sites(d_rows, 300, midp=True, out=out, stream=side)
    side.synchronize()
    assert (device_bits(out) == host_bits(rows, 300, True)).all()
    ctx.hwe_sites(dev, 300, out=out)
    torch.cuda.synchronize()
    assert (device_bits(out) == host_bits(host, 300, False)).all()
    assert ctx.hwe_sites(dev, 0).numel() == 0


def test_refused_before_the_device(ctx, case_counts):
    host, dev = case_counts
    with pytest.raises(ValueError, match="counts"):
        ctx.hwe_sites(torch.from_numpy(host.view(np.int32)), 4)          # a host tensor
    with pytest.raises(ValueError, match="counts"):
        ctx.hwe_sites(dev[:4], 5)
    with pytest.raises(ValueError, match="counts"):
        ctx.hwe_sites(dev.to(torch.int64), 4)
    with pytest.raises(ValueError, match="out"):
        ctx.hwe_sites(dev, 4, out=torch.empty(5, dtype=torch.float64, device="cuda:0"))
    with pytest.raises(ValueError, match="out"):
        ctx.hwe_sites(dev, 4, out=torch.empty(4, dtype=torch.float32, device="cuda:0"))
    p = torch.empty(4, dtype=torch.float64, device="cuda:0")
    assert ctx.lib.cuking_hwe_sites(ctx.handle, dev.data_ptr(), 4, 2, p.data_ptr(), None) == 1
    assert b"unknown flags" in ctx.lib.cuking_last_error()
    assert ctx.lib.cuking_hwe_sites(ctx.handle, dev.data_ptr() + 4, 4, 0, p.data_ptr(), None) == 1
    assert b"aligned" in ctx.lib.cuking_last_error()
    assert ctx.lib.cuking_hwe_sites(ctx.handle, None, 4, 0, p.data_ptr(), None) == 1
    bits = torch.zeros((2, 2), dtype=torch.int64, device="cuda:0")
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="min_hwe_p"):
            ctx.filter_sites(bits, 2, 64, min_hwe_p=bad)
    with pytest.raises(ValueError, match="hwe_counts"):
        ctx.filter_sites(bits, 2, 64, hwe_counts=torch.zeros((64, 4), dtype=torch.int32,
                                                             device="cuda:0"))
    with pytest.raises(ValueError, match="hwe_counts"):
        ctx.filter_sites(bits, 2, 64, min_hwe_p=0.5,
                         hwe_counts=torch.zeros((32, 4), dtype=torch.int32, device="cuda:0"))


N, M = 200, 700
ALL_HET, NO_HET, ALL_MISSING, SUBSET_ONLY = 5, 321, 699, 64


@pytest.fixture(scope="module")
def planted():
    """200 x 700 genotypes in Hardy-Weinberg proportions with planted sites: every sample het;
    no het at frequency 0.5; all missing; and one in equilibrium among the first 120 samples
    whose other 80 are all het."""
    rng = np.random.default_rng(11)
    af = rng.uniform(0.05, 0.5, size=M)
    geno = ((rng.random((N, M)) < af).astype(np.int8) + (rng.random((N, M)) < af).astype(np.int8))
    geno[rng.random((N, M)) < 0.02] = -1
    geno[:, ALL_HET] = 1
    geno[:, NO_HET] = np.where(np.arange(N) % 2 == 0, 0, 2)
    geno[:, ALL_MISSING] = -1
    geno[:120, SUBSET_ONLY] = np.repeat([0, 1, 2], [30, 60, 30])
    geno[120:, SUBSET_ONLY] = 1
    bits = pack(geno)
    return geno, bits, bits.shape[1]


def test_filter_sites_end_to_end(ctx, planted):
    geno, bits, wps = planted
    d_bits = ctx.upload_bitset(bits)
    counts = site_counts_numpy(geno, wps // 2)
    p = cuking_amd.hwe_sites_host(counts, M)
    hwe = cuking_amd.hwe_site_mask(p, 1e-6)
    assert not hwe[ALL_HET] and not hwe[NO_HET] and not hwe[SUBSET_ONLY] and hwe[ALL_MISSING]
    assert p[ALL_MISSING] == 1.0 and hwe.sum() == M - 3
    keep, kept = cuking_amd.site_mask_host(counts, M, also=hwe)
    assert kept == M - 4                                  # (the rule drops the all-missing site)
    qc = ctx.filter_sites(d_bits, wps, M, min_hwe_p=1e-6)
    torch.cuda.synchronize()
    assert qc.keep().tolist() == cuking_amd.site_mask_bool(keep, M).tolist()
    assert qc.num_sites == kept and hc.bits(qc.hwe_p()).tolist() == hc.bits(p).tolist()
    want_bits, want_wps, _ = cuking_amd.compact_sites_host(bits, wps, keep, M)
    assert qc.words_per_sample == want_wps
    assert qc.bits.cpu().numpy().view(np.uint64).tobytes() == want_bits.tobytes()
    # the mid-p form, together with the other rules and a caller's mask
    also = np.arange(M) % 7 != 0
    p_mid = cuking_amd.hwe_sites_host(counts, M, midp=True)
    keep_mid, kept_mid = cuking_amd.site_mask_host(
        counts, M, 0.9, 0.1, 1, also=cuking_amd.hwe_site_mask(p_mid, 0.05, also))
    qc = ctx.filter_sites(d_bits, wps, M, 0.9, 0.1, 1, also=also, min_hwe_p=0.05, hwe_midp=True)
    assert qc.keep_words.tolist() == keep_mid.tolist() and 0 < kept_mid < kept
    assert hc.bits(qc.hwe_p()).tolist() == hc.bits(p_mid).tolist()
    # without the keyword: the bytes of the path as it was, and no p-values
    plain_keep, _ = cuking_amd.site_mask_host(counts, M)
    plain_bits, plain_wps, _ = cuking_amd.compact_sites_host(bits, wps, plain_keep, M)
    qc = ctx.filter_sites(d_bits, wps, M)
    assert qc.hwe_p() is None and qc.keep_words.tolist() == plain_keep.tolist()
    assert qc.words_per_sample == plain_wps
    assert qc.bits.cpu().numpy().view(np.uint64).tobytes() == plain_bits.tobytes()
    assert ctx.filter_sites(d_bits, wps, M, hwe_midp=True).hwe_p() is None


def test_hwe_counts_from_a_row_subset(ctx, planted):
    geno, bits, wps = planted
    d_bits = ctx.upload_bitset(bits)
    sub = ctx.site_counts(d_bits[:120], wps)
    sub_host = site_counts_numpy(geno[:120], wps // 2)
    assert sub.cpu().numpy().view(np.uint32).tolist() == sub_host.tolist()
    p_sub = cuking_amd.hwe_sites_host(sub_host, M)
    qc = ctx.filter_sites(d_bits, wps, M, min_hwe_p=1e-6, hwe_counts=sub)
    assert hc.bits(qc.hwe_p()).tolist() == hc.bits(p_sub).tolist()
    # the rule's own counts stay the whole cohort's; only the test looks at the subset
    counts = site_counts_numpy(geno, wps // 2)
    assert qc.counts().tolist() == counts[:M].tolist()
    keep, kept = cuking_amd.site_mask_host(counts, M,
                                           also=cuking_amd.hwe_site_mask(p_sub, 1e-6))
    assert qc.keep_words.tolist() == keep.tolist()
    # the site that is out of equilibrium only in the other 80 samples now stays
    assert qc.keep()[SUBSET_ONLY] and not qc.keep()[ALL_HET] and kept == M - 3
