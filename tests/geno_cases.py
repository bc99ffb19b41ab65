"""What the host and the GPU tests of the genotype matrix product share (no GPU, no test of
its own): the case list, the seeded inputs, the dense float64 reference and the checks, each
written against a `run` callable so that the host twin and the kernel meet the same code.

    run(bits, words_per_row, num_cols, table, per_row, b_full, num_rhs, out_full) -> out_full

`b_full` is float32 [num_cols, ldb], `out_full` float32 [rows, ldo] (both numpy; the product
reads / writes their first num_rhs columns)."""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import cuking_amd
from cuking_amd.pca import hwe_table
from site_qc_cases import pack

EPS = 2.0 ** -24


@dataclass(frozen=True)
class Case:
    rows: int
    cols: int
    rhs: int
    per_row: bool
    ldb_pad: int = 0
    ldo_pad: int = 0

    @property
    def id(self):
        return (f"{self.rows}x{self.cols}x{self.rhs}-{'row' if self.per_row else 'col'}"
                f"-ldb+{self.ldb_pad}-ldo+{self.ldo_pad}")


# rows in {1, 33, 128, 130, 257}, cols in {1, 63, 64, 65, 700, 4100}, rhs in {1, 31, 32, 33, 64},
# both table axes, pitches equal to and above num_rhs: every value with every table axis, not
# the full product.  The kernel does not split the k range, so there is no threshold to bracket.
CASES = (
    Case(1, 1, 1, False), Case(1, 63, 31, True, 3, 0), Case(1, 4100, 64, False, 0, 5),
    Case(1, 700, 33, True), Case(33, 64, 32, False, 1, 1), Case(33, 65, 33, True, 0, 7),
    Case(33, 1, 64, True), Case(33, 700, 1, False, 2, 0), Case(128, 63, 64, False),
    Case(128, 700, 31, True, 5, 5), Case(128, 4100, 32, True), Case(128, 65, 1, True, 0, 3),
    Case(130, 64, 33, False, 31, 0), Case(130, 4100, 1, True, 1, 0), Case(130, 1, 31, False),
    Case(130, 700, 64, True, 0, 64), Case(130, 65, 32, False, 0, 32), Case(257, 65, 64, True, 3, 3),
    Case(257, 700, 32, False), Case(257, 4100, 33, False, 4, 4), Case(257, 63, 1, False, 0, 2),
    Case(257, 64, 31, True), Case(257, 1, 33, False, 2, 2), Case(128, 64, 64, True, 1, 0),
    Case(33, 4100, 31, False, 0, 1), Case(1, 64, 32, True), Case(1, 65, 1, False, 7, 0),
    Case(257, 63, 32, True, 0, 9),
)
assert len(CASES) <= 30 and len({c.id for c in CASES}) == len(CASES)


def codes_of(rng, rows, cols, missing=0.10):
    """uint8 [rows, cols] codes: 0 hom-ref, 1 het, 2 hom-var, 3 missing (10 %)."""
    codes = rng.integers(0, 3, size=(rows, cols)).astype(np.uint8)
    codes[rng.random((rows, cols)) < missing] = 3
    return codes


def bits_of(codes, per_row):
    """(bits uint64 [rows, words_per_row], words_per_row) of the codes [rows, cols] in the
    layout of the table axis: per column the sample-major bitset (cuking_pack_host), per row
    the site-major planes of its transpose (the tail reads as missing)."""
    geno = np.where(codes == 3, -1, codes).astype(np.int8)
    rows, cols = codes.shape
    if not per_row:
        bits = pack(geno)
        assert bits.shape[1] == cuking_amd.words_per_sample(cols)
        return bits, bits.shape[1]
    sample_major = pack(np.ascontiguousarray(geno.T))        # [cols samples, sites = rows]
    site_bits = cuking_amd.transpose_sites_host(sample_major, sample_major.shape[1], rows)
    words = 2 * cuking_amd.ld_site_words(cols)
    return np.ascontiguousarray(site_bits.reshape(rows, words)), words


@lru_cache(maxsize=None)
def inputs(case: Case):
    rng = np.random.default_rng(7919 * case.rows + 31 * case.cols + case.rhs
                                + (1 << 20) * case.per_row)
    codes = codes_of(rng, case.rows, case.cols)
    bits, words = bits_of(codes, case.per_row)
    bits.setflags(write=False)
    codes.setflags(write=False)
    return codes, bits, words, int(rng.integers(1 << 30))


def real_table(rng, entries):
    """float32 [entries, 4] from hwe_table on drawn site counts (100 samples, ~4 % unused)."""
    called = rng.integers(1, 101, size=entries)
    het = rng.integers(0, called + 1)
    hom_var = rng.integers(0, called - het + 1)
    counts = np.stack([called - het - hom_var, het, hom_var, 100 - called], axis=1)
    return hwe_table(counts.astype(np.uint32), entries)[0]


def dense(codes, table, per_row):
    """The decoded float64 matrix: Z[r, k] = table[r or k, code(r, k)]."""
    t64 = table.astype(np.float64)
    if per_row:
        return np.take_along_axis(t64, codes.astype(np.int64), axis=1)
    return t64[np.arange(codes.shape[1])[None, :], codes.astype(np.int64)]


def padded(values, pad, fill=np.nan):
    """float32 [rows, cols + pad] holding `values`, the pad columns `fill`."""
    full = np.full((values.shape[0], values.shape[1] + pad), fill, dtype=np.float32)
    full[:, :values.shape[1]] = values
    return full


def call(run, case, bits, words, table, b):
    """One product of the case; checks that every [r][c < num_rhs] is finite and every pad
    element of the NaN-filled output still NaN."""
    b_full = padded(b, case.ldb_pad, fill=1e30)     # (a pad column that would be noticed)
    out_full = np.full((case.rows, case.rhs + case.ldo_pad), np.nan, dtype=np.float32)
    got = run(bits, words, case.cols, table, case.per_row, b_full, case.rhs, out_full)
    assert got.shape == out_full.shape
    assert np.isfinite(got[:, :case.rhs]).all(), case.id
    assert np.isnan(got[:, case.rhs:]).all(), case.id
    return got[:, :case.rhs]


def check_exact(run, case):
    """Integer tables and integer B: bit-equal to the int64 product."""
    codes, bits, words, seed = inputs(case)
    rng = np.random.default_rng(seed)
    entries = case.rows if case.per_row else case.cols
    for table in (np.tile(np.float32([0, 1, 2, 0]), (entries, 1)),
                  rng.integers(-3, 4, size=(entries, 4)).astype(np.float32)):
        b = rng.integers(-8, 9, size=(case.cols, case.rhs)).astype(np.float32)
        z = dense(codes, table, case.per_row)
        assert (np.abs(z) @ np.abs(b.astype(np.float64))).max(initial=0) < 2 ** 24   # condition
        want = z.astype(np.int64) @ b.astype(np.int64)
        got = call(run, case, bits, words, table, b)
        assert np.array_equal(got.astype(np.float64), want.astype(np.float64)), case.id
        # garbage beyond num_cols changes nothing; a second call gives the same bytes
        dirty = bits.copy()
        plane = words // 2
        mask = np.zeros(plane * 64, dtype=np.uint8)
        mask[case.cols:] = 1
        beyond = np.packbits(mask, bitorder="little").view("<u8").astype(np.uint64)
        noise = rng.integers(0, 1 << 63, size=(case.rows, words), dtype=np.uint64) * np.uint64(2) \
            + rng.integers(0, 2, size=(case.rows, words), dtype=np.uint64)
        noise[:, :plane] = ~np.uint64(0)           # (het plane: every bit beyond flips)
        dirty ^= noise & np.concatenate([beyond, beyond])[None, :]
        if case.cols < plane * 64:
            assert not np.array_equal(dirty, bits)
        assert call(run, case, dirty, words, table, b).tobytes() == got.tobytes(), case.id
        assert call(run, case, bits, words, table, b).tobytes() == got.tobytes(), case.id


def check_bound(run, case):
    """hwe_table tables and normal B: |out - Z64 @ B64| <= (num_cols + 2) 2^-24 |Z64| @ |B64|,
    elementwise -- the bound of a float32 accumulation of num_cols terms in any order."""
    codes, bits, words, seed = inputs(case)
    rng = np.random.default_rng(seed + 1)
    table = real_table(rng, case.rows if case.per_row else case.cols)
    b = rng.standard_normal((case.cols, case.rhs)).astype(np.float32)
    z, b64 = dense(codes, table, case.per_row), b.astype(np.float64)
    got = call(run, case, bits, words, table, b).astype(np.float64)
    bound = (case.cols + 2) * EPS * (np.abs(z) @ np.abs(b64))
    err = np.abs(got - z @ b64)
    print(f"{case.id}: largest error / bound = "
          f"{(err / np.where(bound > 0, bound, 1)).max(initial=0):.3g}")
    assert (err <= bound).all(), case.id


def check_both_layouts(run, transpose):
    """One cohort, one per-site table: the per-row call on transpose_sites(bits) (Z^T A) and
    the per-column call on bits (Z B) against the same dense Z, each within its bound.
    `transpose(bits, words_per_sample, num_sites)` -> uint64 [num_sites, 2 Q]."""
    n, m, width = 130, 700, 33
    rng = np.random.default_rng(20)
    codes = codes_of(rng, n, m)
    bits, wps = bits_of(codes, False)
    table = real_table(rng, m)
    z = dense(codes, table, False)                           # [n, m]
    site_bits = transpose(bits, wps, m)
    assert site_bits.shape == (m, 2 * cuking_amd.ld_site_words(n))
    a = rng.standard_normal((n, width)).astype(np.float32)
    b = rng.standard_normal((m, width)).astype(np.float32)
    zt_a = run(site_bits, site_bits.shape[1], n, table, True, a, width,
               np.full((m, width), np.nan, dtype=np.float32)).astype(np.float64)
    z_b = run(bits, wps, m, table, False, b, width,
              np.full((n, width), np.nan, dtype=np.float32)).astype(np.float64)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    assert (np.abs(zt_a - z.T @ a64) <= (n + 2) * EPS * (np.abs(z.T) @ np.abs(a64))).all()
    assert (np.abs(z_b - z @ b64) <= (m + 2) * EPS * (np.abs(z) @ np.abs(b64))).all()


def refusals(call_abi):
    """Every refusal of the contract: `call_abi(**overrides)` makes the raw ABI call with the
    arguments of a valid 5 x 70 x 3 product, some replaced, and returns (status, message)."""
    from cuking_amd import _lib
    status, _ = call_abi()
    assert status == _lib.OK
    for what, kw in {"null bits": dict(bits=None), "null table": dict(table=None),
                     "null B": dict(b=None), "null out": dict(out=None),
                     "odd words_per_row": dict(words_per_row=3),
                     "zero words_per_row": dict(words_per_row=0),
                     "num_cols beyond the words": dict(words_per_row=2, num_cols=65),
                     "num_rhs 0": dict(num_rhs=0), "num_rhs 65": dict(num_rhs=65, ldb=65, ldo=65),
                     "ldb below num_rhs": dict(ldb=2), "ldo below num_rhs": dict(ldo=2),
                     "unknown table axis": dict(axis=2), "negative table axis": dict(axis=-1)}.items():
        status, message = call_abi(**kw)
        assert status == _lib.ERR_INVALID_ARGUMENT, what
        assert message.startswith("geno matmul:"), (what, message)
    # nothing to do: no rows needs no pointers; no columns needs only out
    assert call_abi(num_rows=0, bits=None, table=None, b=None, out=None)[0] == _lib.OK
    assert call_abi(num_cols=0, bits=None, table=None, b=None)[0] == _lib.OK
    assert call_abi(num_cols=0, bits=None, table=None, b=None,
                    axis=_lib.GENO_TABLE_PER_ROW)[0] == _lib.OK
