"""Genotype matrix products on the GPU: the f32-input MFMA kernel against the dense float64
reference over the case list the host twin runs -- exact for integer operands, within the
accumulation bound for real ones --, its output rules (plain stores into [r][c < num_rhs] only,
garbage beyond num_cols ignored, the same bytes on every call and stream) and both layouts
against one reference."""
import numpy as np
import pytest
import torch

from geno_cases import (CASES, Case, check_both_layouts, check_bound, check_exact, codes_of,
                        bits_of, dense, real_table, refusals)

pytestmark = pytest.mark.gpu


def device(a):
    a = np.array(a, order="C")      # (a writable copy: the shared inputs are read-only)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to("cuda:0")


@pytest.fixture(scope="module")
def run_device(ctx):
    def run(bits, words_per_row, num_cols, table, per_row, b_full, num_rhs, out_full, stream=None):
        d_out = device(out_full)
        ctx.geno_matmul(device(bits), words_per_row, num_cols, device(table),
                        device(b_full)[:, :num_rhs], per_row=per_row, out=d_out[:, :num_rhs],
                        stream=stream)
        (stream or torch.cuda.current_stream()).synchronize()
        return d_out.cpu().numpy()
    return run


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_exact_for_integer_operands(run_device, case):
    check_exact(run_device, case)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_within_the_accumulation_bound(run_device, case):
    check_bound(run_device, case)


def test_both_layouts_against_one_reference(ctx, run_device):
    def transpose(bits, wps, m):
        return ctx.transpose_sites(device(bits), wps, m).cpu().numpy().view(np.uint64).reshape(m, -1)
    check_both_layouts(run_device, transpose)


def test_same_bytes_on_two_streams_and_no_columns(ctx, run_device):
    case = Case(257, 700, 33, False, 2, 3)
    rng = np.random.default_rng(77)
    codes = codes_of(rng, case.rows, case.cols)
    bits, words = bits_of(codes, False)
    table = real_table(rng, case.cols)
    b = rng.standard_normal((case.cols, case.rhs + case.ldb_pad)).astype(np.float32)
    blank = np.full((case.rows, case.rhs + case.ldo_pad), np.nan, dtype=np.float32)
    first = run_device(bits, words, case.cols, table, False, b, case.rhs, blank)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    second = run_device(bits, words, case.cols, table, False, b, case.rhs, blank, stream=side)
    assert first.tobytes() == second.tobytes()
    assert np.isnan(first[:, case.rhs:]).all() and np.isfinite(first[:, :case.rhs]).all()
    z, b64 = dense(codes, table, False), b[:, :case.rhs].astype(np.float64)
    assert (np.abs(first[:, :case.rhs] - z @ b64) <=
            (case.cols + 2) * 2.0 ** -24 * (np.abs(z) @ np.abs(b64))).all()
    # no columns: zeros into [r][c < num_rhs], the pad untouched; no rows: nothing
    empty = run_device(bits, words, 0, table[:0], False, b[:0], case.rhs, blank)
    assert (empty[:, :case.rhs] == 0).all() and np.isnan(empty[:, case.rhs:]).all()
    out = ctx.geno_matmul(device(bits)[:0], words, case.cols, device(table), device(b))
    assert tuple(out.shape) == (0, case.rhs + case.ldb_pad)


def test_launches_are_split(ctx, run_device):
    """A cap of one workgroup per launch sends the 257 rows (128 to a workgroup) out in three
    launches, two of them with block_base != 0: the bytes of the one launch, in both layouts
    and with one and two column blocks of B."""
    rng = np.random.default_rng(78)
    for case in (Case(257, 700, 33, False, 2, 3), Case(257, 65, 31, True, 0, 1)):
        codes = codes_of(rng, case.rows, case.cols)
        bits, words = bits_of(codes, case.per_row)
        table = real_table(rng, case.rows if case.per_row else case.cols)
        b = rng.standard_normal((case.cols, case.rhs + case.ldb_pad)).astype(np.float32)
        blank = np.full((case.rows, case.rhs + case.ldo_pad), np.nan, dtype=np.float32)
        args = (bits, words, case.cols, table, case.per_row, b, case.rhs, blank)
        whole = run_device(*args)
        ctx.set_option("max_launch_blocks", 1)
        try:
            split = run_device(*args)
        finally:
            ctx.set_option("max_launch_blocks", 0)
        assert np.isfinite(whole[:, :case.rhs]).all()
        assert np.array_equal(split.view(np.uint8), whole.view(np.uint8))


def test_refused_arguments_on_a_live_context(ctx):
    """Every refusal of the contract through cuking_geno_matmul with a context: INVALID_ARGUMENT
    and a message, the output of the refused calls untouched."""
    from cuking_amd import _lib
    bits = torch.zeros((5, 4), dtype=torch.int64, device="cuda:0")
    table = torch.ones((70, 4), dtype=torch.float32, device="cuda:0")
    b = torch.ones((70, 3), dtype=torch.float32, device="cuda:0")
    out = torch.full((5, 3), 7.0, dtype=torch.float32, device="cuda:0")
    stream = torch.cuda.current_stream()
    valid = []

    def device_call(**kw):
        a = dict(bits=bits.data_ptr(), num_rows=5, words_per_row=4, num_cols=70,
                 table=table.data_ptr(), axis=_lib.GENO_TABLE_PER_COLUMN, b=b.data_ptr(), ldb=3,
                 num_rhs=3, out=out.data_ptr(), ldo=3)
        a.update(kw)
        out.fill_(7.0)
        status = ctx.lib.cuking_geno_matmul(
            ctx.handle, a["bits"], a["num_rows"], a["words_per_row"], a["num_cols"], a["table"],
            a["axis"], a["b"], a["ldb"], a["num_rhs"], a["out"], a["ldo"], int(stream.cuda_stream))
        stream.synchronize()
        if status != _lib.OK:       # a refused call has launched nothing
            assert (out == 7.0).all().item(), kw
        else:
            valid.append((kw, out.cpu().numpy().copy()))
        return status, ctx.lib.cuking_last_error().decode()
    refusals(device_call)
    # the valid calls of the list: the product, no rows (nothing), no columns (zeros; both axes)
    assert [v[1].tolist() for v in valid] == [[[70.0] * 3] * 5, [[7.0] * 3] * 5,
                                              [[0.0] * 3] * 5, [[0.0] * 3] * 5]
    # no columns with a table per ROW: bits, table and B may be null there too; zeros
    for rows in (5, 130):
        wide = torch.full((rows, 4), 7.0, dtype=torch.float32, device="cuda:0")
        assert ctx.lib.cuking_geno_matmul(ctx.handle, None, rows, 2, 0, None,
                                          _lib.GENO_TABLE_PER_ROW, None, 3, 3, wide.data_ptr(), 4,
                                          int(stream.cuda_stream)) == _lib.OK
        stream.synchronize()
        assert (wide[:, :3] == 0).all().item() and (wide[:, 3] == 7.0).all().item()


def test_wrapper_refusals(ctx):
    bits = torch.zeros((5, 4), dtype=torch.int64, device="cuda:0")
    table = torch.ones((70, 4), dtype=torch.float32, device="cuda:0")
    b = torch.ones((70, 3), dtype=torch.float32, device="cuda:0")
    assert ctx.geno_matmul(bits, 4, 70, table, b).cpu().tolist() == [[70.0] * 3] * 5
    with pytest.raises(ValueError, match="table"):
        ctx.geno_matmul(bits, 4, 70, table[:69], b)
    with pytest.raises(ValueError, match="rhs"):
        ctx.geno_matmul(bits, 4, 70, table, b.double())
    with pytest.raises(ValueError, match="rhs"):
        ctx.geno_matmul(bits, 4, 70, table, b.cpu())
    with pytest.raises(ValueError, match="out"):
        ctx.geno_matmul(bits, 4, 70, table, b, out=torch.zeros((5, 2), device="cuda:0"))
    import cuking_amd
    with pytest.raises(cuking_amd.CukingError, match="num_rhs"):
        ctx.geno_matmul(bits, 4, 70, table, torch.ones((70, 65), device="cuda:0"))
    with pytest.raises(cuking_amd.CukingError, match="columns"):
        ctx.geno_matmul(bits, 2, 70, table, b)
