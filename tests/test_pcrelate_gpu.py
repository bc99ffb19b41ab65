"""PC-Relate on the GPU: pcrelate_matrix_kernel against the integer formula, the host twin and
the float64 reference of pcrelate_cases.py, the output rules (symmetry, block independence,
streams, pitch), the refusals through the raw ABI and the wrapper, and the end-to-end fixture
through ctx.pca -> ctx.pcrelate."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import pcrelate_cases as pc

import cuking_amd
from cuking_amd import _lib
from cuking_amd.pcrelate import pcrelate_matrix_host

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
    return bits, padded(inp.x), padded(inp.beta)


@lru_cache(maxsize=None)
def device_backend(case):
    import torch
    ctx = _CTX[0]
    inp = pc.inputs(case)
    bits, x, beta = _upload(ctx, inp)
    rows, cols = case.block[1] - case.block[0], case.block[3] - case.block[2]
    wide = torch.full((rows, cols + case.pad), float("nan"), dtype=torch.float32,
                      device=f"cuda:{ctx.device}")
    out = ctx.pcrelate_matrix(bits, inp.wps, case.sites, x, beta, inp.lo, inp.hi,
                              block=case.block, out=wide[:, :cols])
    torch.cuda.synchronize()
    assert torch.isnan(wide[:, cols:]).all()   # the pitch keeps its NaNs
    return out.cpu().numpy().copy()


@lru_cache(maxsize=None)
def host_backend(case):
    inp = pc.inputs(case)
    return pcrelate_matrix_host(inp.bits, inp.wps, case.sites, np.ascontiguousarray(inp.x),
                                np.ascontiguousarray(inp.beta), inp.lo, inp.hi, block=case.block)


@pytest.fixture(autouse=True)
def _context(ctx):
    if not _CTX:
        _CTX.append(ctx)


@pytest.mark.parametrize("case", pc.EXACT_CASES, ids=lambda c: c.name)
def test_device_exact(case):
    pc.check_exact(case, device_backend)
    assert device_backend(case).tobytes() == host_backend(case).tobytes()


@pytest.mark.parametrize("case", pc.REAL_CASES, ids=lambda c: c.name)
def test_device_against_host_twin(case):
    pc.check_twin(case, device_backend, host_backend)


@pytest.mark.parametrize("case", pc.REAL_CASES, ids=lambda c: c.name)
def test_device_against_float64_reference(case):
    pc.check_reference(case, device_backend, "device")


@pytest.mark.parametrize("d", range(1, 33))
def test_ladder_device_against_float64_reference_and_host_twin(d):
    """Every d from 1 to 32 -- each instantiation of pcrelate_matrix_kernel at its width, below
    it and at the first d of the next -- at 130 samples x 97 sites, the whole block and (5, 70,
    97, 130)."""
    for block in pc.LADDER_BLOCKS:
        case = pc.ladder_case(d, block)
        pc.check_reference(case, device_backend, "device")
        pc.check_twin(case, device_backend, host_backend)
    whole = device_backend(pc.ladder_case(d)).view(np.uint32)
    assert np.array_equal(whole, whole.T)
    i0, i1, j0, j1 = pc.LADDER_BLOCKS[1]
    part = device_backend(pc.ladder_case(d, pc.LADDER_BLOCKS[1])).view(np.uint32)
    assert np.array_equal(part, whole[i0:i1, j0:j1])


@pytest.mark.parametrize("case", [c for c in pc.CASES if c.block == (0, c.n, 0, c.n)],
                         ids=lambda c: c.name)
def test_diagonal_block_is_bytewise_symmetric(case):
    got = device_backend(case).view(np.uint32)
    assert np.array_equal(got, got.T)


def test_block_equals_the_whole_call_and_streams_agree(ctx):
    import torch
    case = next(c for c in pc.CASES if c.name == "257x700 d11 block")
    inp = pc.inputs(case)
    bits, x, beta = _upload(ctx, inp)
    whole = ctx.pcrelate_matrix(bits, inp.wps, case.sites, x, beta, inp.lo, inp.hi)
    torch.cuda.synchronize()
    i0, i1, j0, j1 = case.block
    want = whole[i0:i1, j0:j1].cpu().numpy()
    assert want.tobytes() == device_backend(case).tobytes()
    one = ctx.pcrelate_matrix(bits, inp.wps, case.sites, x, beta, inp.lo, inp.hi,
                              block=(200, 201, 200, 201))
    torch.cuda.synchronize()
    assert one.cpu().numpy().tobytes() == whole[200:201, 200:201].cpu().numpy().tobytes()
    outs = []
    for _ in range(2):
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        outs.append(ctx.pcrelate_matrix(bits, inp.wps, case.sites, x, beta, inp.lo, inp.hi,
                                        block=case.block, stream=stream))
        stream.synchronize()
    assert outs[0].cpu().numpy().tobytes() == outs[1].cpu().numpy().tobytes() == want.tobytes()


def test_launches_are_split(ctx):
    """A cap of two workgroups per launch sends the 3 x 3 tiles of 257 samples out in five
    launches, four of them with block_base != 0: the bytes of the one launch."""
    import torch
    case = next(c for c in pc.CASES if c.name == "257x700 d3")
    inp = pc.inputs(case)
    bits, x, beta = _upload(ctx, inp)
    whole = device_backend(case)
    ctx.set_option("max_launch_blocks", 2)
    try:
        split = ctx.pcrelate_matrix(bits, inp.wps, case.sites, x, beta, inp.lo, inp.hi,
                                    block=case.block)
        torch.cuda.synchronize()
    finally:
        ctx.set_option("max_launch_blocks", 0)
    assert np.array_equal(split.cpu().numpy().view(np.uint8), whole.view(np.uint8))


def test_zero_sites_write_nan_and_an_empty_block_is_ok(ctx):
    import torch
    inp = pc.inputs(pc.CASES[4])
    bits, x, beta = _upload(ctx, inp)
    out = ctx.pcrelate_matrix(bits, inp.wps, 0, x, beta, inp.lo, inp.hi)
    torch.cuda.synchronize()
    assert out.shape == (33, 33) and torch.isnan(out).all()
    out = ctx.pcrelate_matrix(bits, inp.wps, 63, x, beta, inp.lo, inp.hi, block=(4, 4, 9, 20))
    assert tuple(out.shape) == (0, 11)


@pytest.mark.parametrize("name", pc.REFUSALS)
def test_device_refusals_leave_out_untouched(ctx, name):
    import torch
    inp = pc.inputs(pc.CASES[4])
    case = inp.case
    bits, x, beta = _upload(ctx, inp)
    out = torch.full((case.n, case.n), -7.0, dtype=torch.float32, device=f"cuda:{ctx.device}")
    a = dict(bits=bits.data_ptr(), num_stored=case.n, wps=inp.wps, sites=case.sites,
             x=x.data_ptr(), ldx=x.stride(0), beta=beta.data_ptr(), ldbeta=beta.stride(0),
             d=case.d, lo=inp.lo, hi=inp.hi, block=(0, case.n, 0, case.n), ldo=case.n,
             out=out.data_ptr())
    a.update(pc.REFUSALS[name])
    block = _lib.CSubmatrix(*a["block"])
    st = ctx.lib.cuking_pcrelate_matrix(
        ctx.handle, a["bits"], a["num_stored"], a["wps"], a["sites"], a["x"], a["ldx"],
        a["beta"], a["ldbeta"], a["d"], a["lo"], a["hi"], C.byref(block), a["out"], a["ldo"],
        int(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert st == _lib.ERR_INVALID_ARGUMENT, name
    assert (out == -7.0).all()


def test_wrapper_refusals(ctx):
    import torch
    inp = pc.inputs(pc.CASES[4])
    bits, x, beta = _upload(ctx, inp)
    out = torch.full((33, 33), -7.0, dtype=torch.float32, device=f"cuda:{ctx.device}")
    with pytest.raises(cuking_amd.CukingError):
        ctx.pcrelate_matrix(bits, inp.wps, 63, x, beta, 0.5, 0.5, out=out)
    with pytest.raises(cuking_amd.CukingError):
        ctx.pcrelate_matrix(bits, inp.wps, 129, x, torch.zeros((129, 3), device=beta.device),
                            inp.lo, inp.hi, out=out)
    with pytest.raises(ValueError):
        ctx.pcrelate_matrix(bits, inp.wps, 63, x, beta[:, :2], inp.lo, inp.hi, out=out)
    with pytest.raises(ValueError):
        ctx.pcrelate_matrix(bits, inp.wps, 63, x, beta, inp.lo, inp.hi, out=out[:, :20])
    with pytest.raises(ValueError):
        ctx.pcrelate_matrix(bits, inp.wps, 63, x.cpu(), beta, inp.lo, inp.hi, out=out)
    torch.cuda.synchronize()
    assert (out == -7.0).all()
    inp = pc.inputs(pc.CASES[5])
    bits, x, beta = _upload(ctx, inp)
    with pytest.raises(ValueError, match="rank"):
        ctx.pcrelate(bits, 2, 64, np.zeros((130, 2), dtype=np.float32))
    with pytest.raises(ValueError, match="min_maf"):
        ctx.pcrelate(bits, 2, 64, x[:, 1:].contiguous(), min_maf=-0.1)


def test_end_to_end_on_the_device(ctx, naive):
    import torch
    from site_qc_cases import pack
    geno, population, fit, _ = pc.e2e_cohort()
    host_bits = pack(np.asarray(geno))
    wps = host_bits.shape[1]
    bits = ctx.upload_bitset(host_bits)
    pca = ctx.pca(bits, wps, pc.E2E_SITES, k=pc.E2E_K, fit=fit)
    result = ctx.pcrelate(bits, wps, pc.E2E_SITES, pca.scores[:, :pc.E2E_K], fit=pca.fit)
    torch.cuda.synchronize()
    assert result.kin.is_cuda and tuple(result.kin.shape) == (132, 132)
    result.kin = result.kin.cpu().numpy()
    pc.check_e2e(result, host_bits, naive)
    # a block of the same fit equals the whole matrix's entries
    part = ctx.pcrelate(bits, wps, pc.E2E_SITES, pca.scores[:, :pc.E2E_K], fit=pca.fit,
                        block=(3, 50, 60, 132))
    torch.cuda.synchronize()
    assert part.kin.cpu().numpy().tobytes() == result.kin[3:50, 60:132].tobytes()
