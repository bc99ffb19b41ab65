"""PC-Relate for listed pairs on the GPU: pcrelate_pairs_kernel bytewise against the host twin
for every case of pcrelate_pairs_cases.py, the integer formula, the float64 reference, the
output rules (position, length, stride, stream, swapped indices), the refusals through the raw
ABI, kin against the matrix kernel's entries, and the end-to-end fixture through ctx.pca ->
ctx.pcrelate_pairs on the records of compute_king."""
from functools import lru_cache

import numpy as np
import pytest

import pcrelate_cases as pc
import pcrelate_pairs_cases as pp

import cuking_amd
from cuking_amd import _lib
from cuking_amd import pcrelate as pcr

pytestmark = pytest.mark.gpu

_CTX = []


def _upload(ctx, inp):
    import torch
    dev = f"cuda:{ctx.device}"
    bits = ctx.upload_bitset(inp.bits.copy())

    def padded(a):   # the same pitch as on the host, NaN between the columns and the pitch
        pitch = a.strides[0] // 4
        wide = np.full((a.shape[0], pitch), np.float32(np.nan), dtype=np.float32)
        wide[:, :a.shape[1]] = a
        return torch.from_numpy(wide).to(dev)[:, :a.shape[1]]
    f = None if inp.f is None else torch.from_numpy(inp.f).to(dev)
    return bits, padded(inp.x), padded(inp.beta), f


def _device_list(ctx, inp):
    import torch
    pairs = np.ascontiguousarray(inp.pairs)
    words = pairs.view(np.int32).reshape(inp.case.pairs, inp.case.stride // 4)
    return torch.from_numpy(words.copy()).to(f"cuda:{ctx.device}")


@lru_cache(maxsize=None)
def device_backend(case):
    import torch
    ctx = _CTX[0]
    inp = pp.inputs(case)
    bits, x, beta, f = _upload(ctx, inp)
    rows = ctx.pcrelate_pairs_raw(bits, inp.wps, case.sites, x, beta, inp.lo, inp.hi,
                                  _device_list(ctx, inp), f)
    torch.cuda.synchronize()
    return pcr.pairs_to_host(rows)


@lru_cache(maxsize=None)
def host_backend(case):
    inp = pp.inputs(case)
    return pcr.pcrelate_pairs_raw_host(inp.bits, inp.wps, case.sites, inp.x, inp.beta, inp.lo,
                                       inp.hi, inp.pairs, inp.f)


@pytest.fixture(autouse=True)
def _context(ctx):
    if not _CTX:
        _CTX.append(ctx)


@pytest.mark.parametrize("case", pp.CASES, ids=lambda c: c.name)
def test_device_rows_are_the_host_twins_bytes(case):
    assert device_backend(case).tobytes() == host_backend(case).tobytes()


@pytest.mark.parametrize("case", pp.EXACT_CASES, ids=lambda c: c.name)
def test_device_exact(case):
    pp.check_exact(case, device_backend)


@pytest.mark.parametrize("case", pp.REAL_CASES, ids=lambda c: c.name)
def test_device_against_float64_reference(case):
    pp.check_reference(case, device_backend, "device")


@pytest.mark.parametrize("d", range(1, 33))
def test_ladder_device_against_float64_reference(d):
    """Every d from 1 to 32 -- each instantiation of pcrelate_pairs_kernel at its width, below
    it and at the first d of the next -- at 130 samples x 97 sites, 513 pairs, both strides,
    with and without f; and the host twin's bytes."""
    for case in pp.ladder(d):
        pp.check_reference(case, device_backend, "device")
        assert device_backend(case).tobytes() == host_backend(case).tobytes()


def test_the_same_pair_gives_the_same_bytes(ctx):
    import torch
    case = next(c for c in pp.CASES if c.name == "P513 S129 d11")
    inp, whole = pp.inputs(case), device_backend(case)
    bits, x, beta, f = _upload(ctx, inp)
    args = (bits, inp.wps, case.sites, x, beta, inp.lo, inp.hi)

    def run(index, **kw):
        if isinstance(index, np.ndarray):
            index = np.ascontiguousarray(index)
        rows = ctx.pcrelate_pairs_raw(*args, index, f, **kw)
        torch.cuda.synchronize()
        return pcr.pairs_to_host(rows)
    # another position, a list of another length (one workgroup instead of two)
    order = np.random.default_rng(5).permutation(case.pairs)[:100]
    assert run(inp.index[order]).tobytes() == whole[order].tobytes()
    assert run(inp.index[512:513]).tobytes() == whole[512:513].tobytes()
    # the other stride, as a device record tensor with num_records
    recs = np.zeros(case.pairs, dtype=cuking_amd.KING_RESULT_DTYPE)
    recs["sample_i"], recs["sample_j"] = inp.index[:, 0], inp.index[:, 1]
    d_recs = torch.from_numpy(recs.view(np.int32).reshape(-1, 6)).to(bits.device)
    assert run(d_recs, num_records=case.pairs).tobytes() == whole.tobytes()
    assert run(d_recs, num_records=70).tobytes() == whole[:70].tobytes()
    # another stream
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    assert run(inp.index, stream=stream).tobytes() == whole.tobytes()
    # the indices swapped
    swapped = run(inp.index[:, ::-1])
    assert np.array_equal(swapped["sample_i"], whole["sample_j"])
    for name in pp.FLOATS + ("ibs0", "sites"):
        assert swapped[name].tobytes() == whole[name].tobytes(), name
    # an int64 [P, 2] tensor, and `out`
    out = torch.full((case.pairs, 8), -7, dtype=torch.int32, device=bits.device)
    got = ctx.pcrelate_pairs_raw(*args, torch.from_numpy(inp.index.astype(np.int64)).to(
        bits.device), f, out=out)
    torch.cuda.synchronize()
    assert got is out and pcr.pairs_to_host(out).tobytes() == whole.tobytes()


def test_launches_are_split(ctx):
    """A cap of one workgroup per launch sends a list of 1300 pairs (512 to a workgroup) out in
    three launches, two of them with a pair base above 0: the bytes of the one launch."""
    import torch
    case = next(c for c in pp.CASES if c.name == "P513 S129 d11")
    inp = pp.inputs(case)
    bits, x, beta, f = _upload(ctx, inp)
    index = np.ascontiguousarray(np.concatenate([inp.index, inp.index[::-1], inp.index])[:1300])

    def run():
        rows = ctx.pcrelate_pairs_raw(bits, inp.wps, case.sites, x, beta, inp.lo, inp.hi, index, f)
        torch.cuda.synchronize()
        return pcr.pairs_to_host(rows)
    whole = run()
    ctx.set_option("max_launch_blocks", 1)
    try:
        split = run()
    finally:
        ctx.set_option("max_launch_blocks", 0)
    assert whole[:513].tobytes() == device_backend(case).tobytes()
    assert np.array_equal(split.view(np.uint8), whole.view(np.uint8))


def test_out_of_range_rows_no_site_rows_and_zero_sites(ctx):
    import torch
    case = next(c for c in pp.CASES if c.name == "exact P513 S65 stride 24")
    got = device_backend(case)
    for k in (5, 6, 7, 8):   # all-missing, no jointly valid site, out of range twice
        assert all(got[name][k:k + 1].view(np.uint32)[0] == 0x7FC00000 for name in pp.FLOATS), k
        assert got["ibs0"][k] == 0 and got["sites"][k] == 0
    assert got["sample_i"][7] == pp.N and got["sample_j"][8] == 0xFFFFFFFF
    inp = pp.inputs(case)
    bits, x, beta, f = _upload(ctx, inp)
    rows = ctx.pcrelate_pairs_raw(bits, inp.wps, 0, x, beta, inp.lo, inp.hi,
                                  _device_list(ctx, inp))
    torch.cuda.synchronize()
    rows = pcr.pairs_to_host(rows)
    pp.check_rows(case, rows)
    assert all(np.isnan(rows[name]).all() for name in pp.FLOATS) and not rows["sites"].any()
    empty = ctx.pcrelate_pairs_raw(bits, inp.wps, case.sites, x, beta, inp.lo, inp.hi,
                                   np.zeros((0, 2), dtype=np.uint32))
    assert tuple(empty.shape) == (0, 8)


@pytest.mark.parametrize("name", pp.REFUSALS)
def test_device_refusals_leave_out_untouched(ctx, name):
    import torch
    inp = pp.inputs(pp.REFUSAL_CASE)
    bits, x, beta, f = _upload(ctx, inp)
    pairs = _device_list(ctx, inp)
    out = torch.full((inp.case.pairs, 8), -7, dtype=torch.int32, device=bits.device)
    pointers = dict(bits=bits.data_ptr(), x=x.data_ptr(), ldx=x.stride(0), beta=beta.data_ptr(),
                    ldbeta=beta.stride(0), f=None, pairs=pairs.data_ptr(), out=out.data_ptr())
    st = ctx.lib.cuking_pcrelate_pairs(
        ctx.handle, *pp.raw_arguments(inp, pointers, **pp.REFUSALS[name]),
        int(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert st == _lib.ERR_INVALID_ARGUMENT, name
    assert (out == -7).all()


def test_kin_against_the_matrix_kernel(ctx):
    import torch
    case = next(c for c in pp.CASES if c.name == "P257 S700 d3")
    inp, got = pp.inputs(case), device_backend(case)
    bits, x, beta, f = _upload(ctx, inp)
    matrix = ctx.pcrelate_matrix(bits, inp.wps, case.sites, x, beta, inp.lo, inp.hi)
    torch.cuda.synchronize()
    matrix = matrix.cpu().numpy()
    tol = pc.Reference(inp.code, inp.x, inp.beta, inp.lo, inp.hi,
                       (0, pp.N, 0, pp.N)).twin_tolerance()
    ok = (inp.index < pp.N).all(axis=1)
    i, j = inp.index[ok, 0], inp.index[ok, 1]
    want, kin = matrix[i, j], got["kin"][ok]
    assert np.array_equal(np.isnan(want), np.isnan(kin))
    fin = ~np.isnan(want)
    ratio = (np.abs(kin.astype(np.float64) - want)[fin] / tol[i, j][fin]).max()
    differ = int((kin.view(np.uint32) != want.view(np.uint32))[fin].sum())
    print(f"kin against pcrelate_matrix: largest error / twin tolerance {ratio:.3g}; {differ} of "
          f"{int(fin.sum())} entries differ in bytes")
    assert ratio <= 1.0


def test_wrapper_errors(ctx):
    inp = pp.inputs(pp.REFUSAL_CASE)
    bits, x, beta, f = _upload(ctx, inp)
    scores = np.ascontiguousarray(inp.x[:, 1:3])
    with pytest.raises(ValueError, match="outside the 40 stored"):
        ctx.pcrelate_pairs(bits, inp.wps, 65, _device_list(ctx, inp), scores=scores)
    with pytest.raises(ValueError, match="either scores or model"):
        ctx.pcrelate_pairs(bits, inp.wps, 65, np.array([[0, 1]]))
    with pytest.raises(ValueError):
        ctx.pcrelate_pairs_raw(bits, inp.wps, 65, x, beta, inp.lo, inp.hi, inp.index.astype(float))
    with pytest.raises(ValueError):
        ctx.pcrelate_pairs_raw(bits, inp.wps, 65, x, beta, inp.lo, inp.hi, inp.index,
                               f=np.zeros(40, dtype=np.float32))
    with pytest.raises(cuking_amd.CukingError):
        ctx.pcrelate_pairs_raw(bits, inp.wps, 65, x, beta, 0.5, 0.5, inp.index)


def test_end_to_end_on_the_device(ctx):
    import torch
    from site_qc_cases import pack
    from test_pcrelate_pairs_host import check_e2e, e2e_pairs
    geno, fit, parent_child, siblings = pp.e2e_cohort()
    host_bits = pack(np.asarray(geno))
    wps = host_bits.shape[1]
    code = np.where(geno < 0, 3, geno).astype(np.uint8)
    bits = ctx.upload_bitset(host_bits)
    n = geno.shape[0]
    # the records of compute_king at the 2nd-degree cut-off: the planted first-degree pairs
    recs = ctx.run(cuking_amd.Submatrix(n), wps, bits, 0.0884, 1 << 16)
    found = {(int(r["sample_i"]), int(r["sample_j"])) for r in recs}
    planted = {(min(p), max(p)) for p in parent_child + siblings}
    assert planted <= found
    pca = ctx.pca(bits, wps, pp.E2E_SITES, k=pc.E2E_K, fit=fit)
    scores = np.ascontiguousarray(pca.scores[:, :pc.E2E_K])
    on_records = ctx.pcrelate_pairs(bits, wps, pp.E2E_SITES, recs, scores=scores, fit=pca.fit)
    torch.cuda.synchronize()
    codes = on_records.relationship()
    for k, r in enumerate(recs):
        pair = (int(r["sample_i"]), int(r["sample_j"]))
        if pair in {(min(p), max(p)) for p in siblings}:
            assert codes[k] == pcr.FULL_SIBLING, pair
        elif pair in planted:
            assert codes[k] == pcr.PARENT_CHILD, pair
    # bytewise the host twin fed with the device's x, beta and f
    twin = cuking_amd.pcrelate_pairs_host(host_bits, wps, pp.E2E_SITES, recs, model=on_records,
                                          inbreeding=on_records.inbreeding)
    assert twin.rows.tobytes() == on_records.rows.tobytes()
    # the fixture's own list: the conditions, the float64 reference, the codes
    index, _, _ = e2e_pairs()
    listed = ctx.pcrelate_pairs(bits, wps, pp.E2E_SITES, index, model=on_records)
    assert listed.inbreeding.tobytes() == on_records.inbreeding.tobytes()
    check_e2e(listed, code)
