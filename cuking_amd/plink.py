"""PLINK 1 binary genotypes (`PREFIX.bed / .bim / .fam`): reader and writer (numpy only).

The `.bed` is variant-major and dense, 2 bits per genotype (include/cuking_amd.h holds the
format and the mapping to the bitset); `.fam` has one line per sample (FID IID father mother
sex phenotype), `.bim` one line per variant.  `open_bed` hands out chunks of rows for
`pack_bed_host` / `KingContext.pack_bed`; `write_plink` is the counterpart of
`inputs.write_input_tables` for tests and tools.

Out of scope: `.pgen`, VCF, sample-major `.bed`, site or sample filtering.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

from . import _lib
from ._lib import check

MAGIC = bytes([0x6C, 0x1B, 0x01])
# n_alt (A1 counted) -> the 2-bit code; missing (negative) -> 1
_CODE_OF_ALT = np.array([3, 2, 0], dtype=np.uint8)


def _path(prefix, suffix: str) -> Path:
    return Path(str(prefix) + suffix)


def read_fam(prefix) -> list:
    """The sample ids of `PREFIX.fam`, in file order: the IIDs when they are all distinct,
    else `FID_IID`; ValueError if those are not distinct either."""
    fids, iids = [], []
    with open(_path(prefix, ".fam")) as f:
        for number, line in enumerate(f, 1):
            fields = line.split()
            if not fields:
                continue
            if len(fields) < 2:
                raise ValueError(f"{_path(prefix, '.fam')}:{number}: expected FID and IID")
            fids.append(fields[0])
            iids.append(fields[1])
    if len(set(iids)) == len(iids):
        return iids
    ids = [f"{a}_{b}" for a, b in zip(fids, iids)]
    if len(set(ids)) != len(ids):
        raise ValueError(f"{_path(prefix, '.fam')}: sample ids are not distinct, neither as IID "
                         "nor as FID_IID")
    return ids


def read_fam_parents(prefix) -> np.ndarray:
    """The parents `PREFIX.fam` declares, as `int64 [n, 2]`: the row index (file order, the order
    of `read_fam`) of each sample's father and mother, -1 for "0" and for an id that is not in
    the file.  Ids are matched by IID when the IIDs are all distinct, else within the sample's
    FID -- the rule by which `read_fam` makes ids distinct (and its ValueError if they are not).
    `mendel.trios_from_parents` turns the result into a list of trios."""
    rows = []
    with open(_path(prefix, ".fam")) as f:
        for number, line in enumerate(f, 1):
            fields = line.split()
            if not fields:
                continue
            if len(fields) < 4:
                raise ValueError(f"{_path(prefix, '.fam')}:{number}: expected FID, IID, father "
                                 "and mother")
            rows.append(fields[:4])
    by_iid = len({r[1] for r in rows}) == len(rows)
    key = (lambda fid, iid: iid) if by_iid else (lambda fid, iid: (fid, iid))
    index = {key(r[0], r[1]): k for k, r in enumerate(rows)}
    if len(index) != len(rows):
        raise ValueError(f"{_path(prefix, '.fam')}: sample ids are not distinct, neither as IID "
                         "nor as FID_IID")
    parents = np.full((len(rows), 2), -1, dtype=np.int64)
    for k, (fid, _, father, mother) in enumerate(rows):
        for column, who in enumerate((father, mother)):
            if who != "0":
                parents[k, column] = index.get(key(fid, who), -1)
    return parents


def count_sites(prefix) -> int:
    """The number of lines (variants) of `PREFIX.bim`."""
    n = 0
    with open(_path(prefix, ".bim"), "rb") as f:
        for line in f:
            n += 1 if line.strip() else 0
    return n


def read_bim_chromosomes(prefix) -> np.ndarray:
    """One int32 group id per variant of `PREFIX.bim`, in file order: the index of the first
    appearance of its chromosome string (column 1) -- what `ld_edges` / `ld_prune` take as
    `group`, so that no LD window reaches across a chromosome boundary."""
    ids, out = {}, []
    with open(_path(prefix, ".bim")) as f:
        for line in f:
            fields = line.split()
            if fields:
                out.append(ids.setdefault(fields[0], len(ids)))
    return np.asarray(out, dtype=np.int32)


def read_bim_positions(prefix) -> np.ndarray:
    """The base-pair coordinate (column 4) of every variant of `PREFIX.bim`, in file order, as
    uint32 -- what `ibd_segments` takes as `pos`; ValueError names a line without one or with
    one outside [0, 2^32)."""
    out = []
    with open(_path(prefix, ".bim")) as f:
        for number, line in enumerate(f, 1):
            fields = line.split()
            if not fields:
                continue
            try:
                value = int(fields[3])
                if not 0 <= value <= 0xFFFFFFFF:
                    raise ValueError
            except (IndexError, ValueError):
                raise ValueError(f"{_path(prefix, '.bim')}:{number}: expected a base-pair "
                                 "coordinate in [0, 2^32) in column 4") from None
            out.append(value)
    return np.asarray(out, dtype=np.uint32)


class BedFile:
    """An open variant-major `.bed`: `num_samples`, `num_sites`, `row_bytes`, `sample_ids`
    and `read_rows`.  A context manager; `close()` releases the file."""

    def __init__(self, prefix):
        self.path = _path(prefix, ".bed")
        self.sample_ids = read_fam(prefix)
        self.num_samples = len(self.sample_ids)
        self.num_sites = count_sites(prefix)
        lib = _lib.load()
        self.row_bytes = int(lib.cuking_bed_row_bytes(self.num_samples))
        self._fd = os.open(self.path, os.O_RDONLY)
        try:
            magic = os.pread(self._fd, 3, 0).ljust(3, b"\0")
            size = os.fstat(self._fd).st_size
            check(lib.cuking_bed_check((C.c_uint8 * 3)(*magic), size, self.num_samples,
                                       self.num_sites))
        except Exception:
            self.close()
            raise

    def read_rows(self, site_begin: int, site_end: int, out: np.ndarray) -> np.ndarray:
        """Rows [site_begin, site_end) into `out` (uint8, contiguous, at least that many
        bytes); returns the filled part of `out` as a flat view."""
        if not 0 <= site_begin <= site_end <= self.num_sites:
            raise ValueError(f"sites [{site_begin}, {site_end}) outside the file's "
                             f"{self.num_sites}")
        if out.dtype != np.uint8 or not out.flags.c_contiguous:
            raise ValueError("out must be a contiguous uint8 array")
        need = (site_end - site_begin) * self.row_bytes
        flat = out.reshape(-1)
        if flat.size < need:
            raise ValueError(f"out holds {flat.size} bytes, the rows need {need}")
        view = memoryview(flat[:need])
        offset, done = 3 + site_begin * self.row_bytes, 0
        while done < need:
            got = os.preadv(self._fd, [view[done:]], offset + done)
            if got <= 0:
                raise OSError(f"{self.path}: short read at byte {offset + done}")
            done += got
        return flat[:need]

    def close(self) -> None:
        if getattr(self, "_fd", None) is not None:
            os.close(self._fd)
            self._fd = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def open_bed(prefix) -> BedFile:
    """Opens `PREFIX.bed` with its `.bim` and `.fam`; validates magic bytes and size through
    `cuking_bed_check` (CukingError names what is wrong)."""
    return BedFile(prefix)


def encode_rows(geno: np.ndarray) -> np.ndarray:
    """int8 `[samples, sites]` genotypes (the value is n_alt, negative = missing) -> the
    `.bed` rows, uint8 `[sites, ceil(samples / 4)]`; unused high bits are zero."""
    geno = np.asarray(geno)
    n, m = geno.shape
    if n and m and geno.max() > 2:
        raise ValueError("n_alt must be 0, 1 or 2 (negative = missing)")
    codes = np.ones((m, (n + 3) // 4 * 4), dtype=np.uint8)
    block = geno.T
    codes[:, :n] = np.where(block < 0, np.uint8(1), _CODE_OF_ALT[np.clip(block, 0, 2)])
    codes[:, n:] = 0
    quads = codes.reshape(m, -1, 4)
    return (quads[:, :, 0] | quads[:, :, 1] << 2 | quads[:, :, 2] << 4 |
            quads[:, :, 3] << 6).astype(np.uint8)


def write_plink(prefix, geno: np.ndarray, sample_ids=None, chunk_sites: int = 4096,
                chromosomes=None, positions=None) -> None:
    """Writes `PREFIX.bed / .bim / .fam` for int8 `[samples, sites]` genotypes (the value is
    n_alt with A1 counted, negative = missing).  `chromosomes`: one name per site for the
    `.bim` (default: all on "1"); `positions`: one base-pair coordinate per site (default:
    the site's number from 1)."""
    geno = np.asarray(geno)
    n, m = geno.shape
    if sample_ids is None:
        sample_ids = [f"S{k:07d}" for k in range(n)]
    if len(sample_ids) != n:
        raise ValueError(f"{len(sample_ids)} sample ids for {n} samples")
    if any(len(str(s).split()) != 1 for s in sample_ids):
        raise ValueError("a sample id must be one word")
    _path(prefix, ".bed").parent.mkdir(parents=True, exist_ok=True)
    with open(_path(prefix, ".fam"), "w") as f:
        f.writelines(f"{s} {s} 0 0 0 -9\n" for s in sample_ids)
    if chromosomes is None:
        chromosomes = ["1"] * m
    if len(chromosomes) != m or any(len(str(c).split()) != 1 for c in chromosomes):
        raise ValueError(f"chromosomes must be {m} names of one word each")
    if positions is None:
        positions = range(1, m + 1)
    if len(positions) != m or any(not 0 <= int(p) <= 0xFFFFFFFF for p in positions):
        raise ValueError(f"positions must be {m} coordinates in [0, 2^32)")
    with open(_path(prefix, ".bim"), "w") as f:
        f.writelines(f"{chromosomes[k]}\tv{k}\t0\t{int(positions[k])}\tA\tC\n" for k in range(m))
    with open(_path(prefix, ".bed"), "wb") as f:
        f.write(MAGIC)
        for lo in range(0, m, chunk_sites):
            f.write(encode_rows(geno[:, lo:lo + chunk_sites]).tobytes())
