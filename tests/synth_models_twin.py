"""CPU twin of the synthetic generator's cohort models.  TEST INFRASTRUCTURE ONLY.

Vectorised numpy on uint64, written from the specification in the header comment of
cuking_amd/csrc/synth.hip (restated below, not imported); it shares no code with
cuking_amd/.  Model 0 is pinned by something older than this file: oracle/synth_oracle.c
must equal it bit for bit (tests/test_synth_models.py).

Specification (integers only; "p %" on the u32 scale is floor(p / 100 * 2^32)):

    mix64(x)         splitmix64 finaliser
    hash3(s,t,a,b)   mix64(mix64(s + t * GOLD + a) ^ (b * 0xD1B54A32D192ED03))   (mod 2^64)
    spectrum(h)      (2^31 | (lo32(h) >> 1)) >> k,  k = 1 + ((hi32(h) * 12) >> 32)
    founder          two alleles: lo32 / hi32 of hash3(seed, 2, founder, site) < AF of the
                     site in the founder's ancestry
    missing          lo32(hash3(seed, 3, sample, site)) < the sample's missing threshold
    duplicate        its founder's genotype, own missing draw
    child            one allele from each founder parent (each parent's genotype drawn in
                     that parent's ancestry); a het parent transmits bit 0 / bit 1 of
                     hash3(seed, 4, child, site)

    model 0 baseline AF = 5 % + ((hi32(hash3(seed, 1, site, 0)) * 45 %) >> 32); one
                     ancestry; every sample misses 1 %
    model 1 exome    AF = spectrum(hash3(seed, 1, site, 0)); one ancestry; 1 %
    model 2 admixed  ancestry of a founder: bit 0 of hash3(seed, 5, founder, 0);
                     AF in ancestry A: the exome value; in B the same, except where
                     lo32(hash3(seed, 8, site, 0)) < 2^30: spectrum(hash3(seed, 6, site, 0));
                     missing threshold from h = hash3(seed, 7, sample, 0): lo32(h) < 1 %
                     -> 10 % + ((hi32(h) * 20 %) >> 32), else 0.5 % + ((hi32(h) * 3 %) >> 32)

Layout: the reference's bitset, per sample [het plane | hom_var plane], site s -> bit
s & 63 of word s >> 6, both bits = missing, padding sites of the last word missing.
"""
from __future__ import annotations

import numpy as np

MODELS = ("baseline", "exome", "admixed")
BASELINE, EXOME, ADMIXED = 0, 1, 2

_M64 = (1 << 64) - 1
_GOLD = 0x9E3779B97F4A7C15
_U = np.uint64

TAG_SITE, TAG_GENO, TAG_MISS, TAG_TRANS, TAG_ANCESTRY, TAG_SITE_B, TAG_CALL, TAG_DIVERGED = \
    1, 2, 3, 4, 5, 6, 7, 8


def _pct(p):
    """floor(p * 2^32) for a decimal fraction given as (numerator, denominator)."""
    return (p[0] << 32) // p[1]


AF_LO, AF_SPAN = _pct((5, 100)), _pct((45, 100))
MISS_1PCT = _pct((1, 100))
TAIL_SHARE = _pct((1, 100))
TAIL_LO, TAIL_SPAN = _pct((10, 100)), _pct((20, 100))
CALL_LO, CALL_SPAN = _pct((5, 1000)), _pct((3, 100))
DIVERGED = 1 << 30
OCTAVES = 12


def model_number(model) -> int:
    return MODELS.index(model) if isinstance(model, str) else int(model)


def mix64(x: np.ndarray) -> np.ndarray:
    x = x ^ (x >> _U(30))
    x = x * _U(0xBF58476D1CE4E5B9)
    x = x ^ (x >> _U(27))
    x = x * _U(0x94D049BB133111EB)
    return x ^ (x >> _U(31))


def hash3(seed: int, tag: int, a, b) -> np.ndarray:
    """a, b: integer arrays that broadcast against each other (values < 2^32)."""
    base = _U((seed + tag * _GOLD) & _M64)
    a = np.asarray(a).astype(np.uint64)
    b = np.asarray(b).astype(np.uint64)
    with np.errstate(over="ignore"):
        return mix64(mix64(base + a) ^ (b * _U(0xD1B54A32D192ED03)))


def lo32(h):
    return h & _U(0xFFFFFFFF)


def hi32(h):
    return h >> _U(32)


def spectrum(h: np.ndarray) -> np.ndarray:
    k = _U(1) + ((hi32(h) * _U(OCTAVES)) >> _U(32))
    return (_U(1 << 31) | (lo32(h) >> _U(1))) >> k


def site_thresholds(model, seed: int, num_sites: int):
    """(AF threshold in ancestry A, in ancestry B), u32 scale, as uint64 arrays [num_sites]."""
    model = model_number(model)
    sites = np.arange(num_sites, dtype=np.uint64)
    h = hash3(seed, TAG_SITE, sites, 0)
    if model == BASELINE:
        a = _U(AF_LO) + ((hi32(h) * _U(AF_SPAN)) >> _U(32))
        return a, a.copy()
    a = spectrum(h)
    if model == EXOME:
        return a, a.copy()
    diverged = lo32(hash3(seed, TAG_DIVERGED, sites, 0)) < _U(DIVERGED)
    b = np.where(diverged, spectrum(hash3(seed, TAG_SITE_B, sites, 0)), a)
    return a, b


def ancestry(model, seed: int, samples) -> np.ndarray:
    """Ancestry (0 = A, 1 = B) the sample indices would have as founders."""
    samples = np.asarray(samples)
    if model_number(model) != ADMIXED:
        return np.zeros(samples.shape, dtype=np.uint8)
    return (hash3(seed, TAG_ANCESTRY, samples, 0) & _U(1)).astype(np.uint8)


def missing_thresholds(model, seed: int, samples) -> np.ndarray:
    """Missing threshold of each sample index, u32 scale (uint64 array)."""
    samples = np.asarray(samples)
    if model_number(model) != ADMIXED:
        return np.full(samples.shape, MISS_1PCT, dtype=np.uint64)
    h = hash3(seed, TAG_CALL, samples, 0)
    tail = _U(TAIL_LO) + ((hi32(h) * _U(TAIL_SPAN)) >> _U(32))
    body = _U(CALL_LO) + ((hi32(h) * _U(CALL_SPAN)) >> _U(32))
    return np.where(in_tail(model, seed, samples), tail, body)


def in_tail(model, seed: int, samples) -> np.ndarray:
    samples = np.asarray(samples)
    if model_number(model) != ADMIXED:
        return np.zeros(samples.shape, dtype=bool)
    return lo32(hash3(seed, TAG_CALL, samples, 0)) < _U(TAIL_SHARE)


def _founder_genotypes(seed, founders, sites, thr_a, thr_b, anc):
    """founders [r] x sites [m] -> genotype 0/1/2 (uint8 [r, m])."""
    h = hash3(seed, TAG_GENO, founders[:, None], sites[None, :])
    thr = np.where(anc[:, None] != 0, thr_b[None, :], thr_a[None, :])
    return ((lo32(h) < thr).astype(np.uint8) + (hi32(h) < thr).astype(np.uint8))


def genotypes(model, seed: int, kind, pa, pb, sample_begin: int, sample_end: int,
              num_sites: int, chunk_rows: int = 128) -> np.ndarray:
    """uint8 [sample_end - sample_begin, num_sites]: alt-allele count, 3 = missing."""
    model = model_number(model)
    kind, pa, pb = (np.asarray(x).astype(np.uint64) for x in (kind, pa, pb))
    thr_a, thr_b = site_thresholds(model, seed, num_sites)
    sites = np.arange(num_sites, dtype=np.uint64)
    out = np.empty((sample_end - sample_begin, num_sites), dtype=np.uint8)
    for r0 in range(sample_begin, sample_end, chunk_rows):
        s = np.arange(r0, min(r0 + chunk_rows, sample_end), dtype=np.uint64)
        k = kind[s]
        src_a = np.where(k == 0, s, pa[s])
        src_b = np.where(k == 2, pb[s], src_a)
        g = _founder_genotypes(seed, src_a, sites, thr_a, thr_b, ancestry(model, seed, src_a))
        children = np.flatnonzero(k == 2)
        if len(children):
            c = s[children]
            ga = g[children]
            gb = _founder_genotypes(seed, src_b[children], sites, thr_a, thr_b,
                                    ancestry(model, seed, src_b[children]))
            ht = hash3(seed, TAG_TRANS, c[:, None], sites[None, :])
            coin_a = (ht & _U(1)).astype(np.uint8)
            coin_b = ((ht >> _U(1)) & _U(1)).astype(np.uint8)
            g[children] = np.where(ga == 1, coin_a, ga >> 1) + np.where(gb == 1, coin_b, gb >> 1)
        miss = lo32(hash3(seed, TAG_MISS, s[:, None], sites[None, :])) < \
            missing_thresholds(model, seed, s)[:, None]
        g[miss] = 3
        out[r0 - sample_begin:r0 - sample_begin + len(s)] = g
    return out


def words_per_sample(num_sites: int) -> int:
    padded = (num_sites + 31) // 32 * 32       # cuking.cu:498-500
    return 2 * ((padded + 63) // 64)           # cuking.cu:513


def bitset_from_genotypes(g: np.ndarray) -> np.ndarray:
    """uint8 [rows, sites] (3 = missing) -> uint64 [rows, words_per_sample]."""
    rows, num_sites = g.shape
    plane = words_per_sample(num_sites) // 2
    planes = np.ones((rows, 2, plane * 64), dtype=np.uint8)   # padding sites: missing
    planes[:, 0, :num_sites] = (g == 1) | (g == 3)
    planes[:, 1, :num_sites] = (g == 2) | (g == 3)
    packed = np.packbits(planes, axis=2, bitorder="little")    # [rows, 2, plane * 8] bytes
    return np.ascontiguousarray(packed).view("<u8").reshape(rows, 2 * plane).astype(np.uint64)


def synth_bitset(model, seed: int, kind, pa, pb, sample_begin: int, sample_end: int,
                 num_sites: int) -> np.ndarray:
    """Same array as oracle.pyoracle.synth_bitset, for any model."""
    return bitset_from_genotypes(
        genotypes(model, seed, kind, pa, pb, sample_begin, sample_end, num_sites))
